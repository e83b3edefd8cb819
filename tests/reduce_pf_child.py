"""Child process of test_gpu_reduce_edges.py::test_runtime_p_kernels_in_child_process: started
with BAGUA_REDUCE_PF=0 in its environment (the switch is read once per process), it runs the
p = 2 recompute cases of the fused middle step on the runtime-p kernels."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "bagua-core_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

if __name__ == "__main__":
    assert os.environ.get("BAGUA_REDUCE_PF") == "0", "start me with BAGUA_REDUCE_PF=0"
    import test_gpu_reduce_edges as T
    n = T.run_pf_cases()
    print(f"runtime-p cases ok: {n}")

"""Child process of test_gpu_onebit_recv_edges.py::test_per_element_kernel_in_child_process:
started with BAGUA_ONEBIT_LUT=0 in its environment (the switch is read once per process), it
runs the crafted middle-step cases for f32 and f16 at p = 2, 4, 8, 16 on the per-element
kernel (onebit_reduce_encode_kernel, tree widths 2, 4 and 8)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "bagua-core_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

if __name__ == "__main__":
    assert os.environ.get("BAGUA_ONEBIT_LUT") == "0", "start me with BAGUA_ONEBIT_LUT=0"
    import test_gpu_onebit_recv_edges as T
    n = T.run_lut_cases()
    print(f"per-element cases ok: {n}")

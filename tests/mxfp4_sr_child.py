"""Child process of test_gpu_mxfp4_sr.py::test_boundary_table_on_both_decode_paths: started with
BAGUA_MXFP4_HWCVT=0 in its environment, it runs the boundary table through the stochastic encode
and the stochastic middle step with the arithmetic decode (HW = false), checks them against the
reference as the parent does and writes every buffer to the .npz file named on the command line."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "bagua-core_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

if __name__ == "__main__":
    assert os.environ.get("BAGUA_MXFP4_HWCVT") == "0", "start me with BAGUA_MXFP4_HWCVT=0"
    import numpy as np

    import bagua_core
    import test_gpu_mxfp4_sr as T
    out = T.boundary_cases(bagua_core)
    np.savez(sys.argv[1], **out)
    print(f"arithmetic cases ok: {len(out)}")

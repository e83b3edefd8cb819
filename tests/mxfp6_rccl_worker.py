"""Worker of tests/test_gpu_mxfp6_op.py: one rank of a real multi-process RCCL communicator
(all ranks on the one GPU, a distinct NCCL_HOSTID each, as tests/rccl_worker.py) running the
centralized ops with the MXFP6 codec.

usage: python mxfp6_rccl_worker.py <rank> <world> <workdir> <op,op,...>
An op is a piece count of the plain pipelined op, or `ef`: two consecutive error-feedback steps on
one state.  Inputs come from <workdir>/inputs.npz (x<rank>), results go to <workdir>/out<rank>.npz:
t<i> is the tensor after the i-th plain op; ef<s>, worker<s> and server<s> are the tensor and the
two residuals after error-feedback step s.  Every op and step starts from the input again."""
from __future__ import annotations

import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bagua-core_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rccl_worker import _host, _uid  # noqa: E402


def main() -> None:
    rank, world, workdir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    ops = sys.argv[4].split(",")
    import bagua_core as bc
    N = bc._native
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    with np.load(os.path.join(workdir, "inputs.npz"), allow_pickle=False) as z:
        x = z[f"x{rank}"]
    comm = bc.BaguaSingleCommunicatorPy(rank, world, 0, stream.cuda_stream, _uid(workdir, "all", rank == 0, bc))
    t = torch.from_numpy(x.copy()).cuda()
    raw = bc.BaguaTensorPy(t, "g").raw()
    out = {}

    def reset():
        t.copy_(torch.from_numpy(x.copy()).cuda())
        torch.cuda.synchronize()  # the reset (current stream) lands before the next op (comm stream)

    plain = 0
    for op in ops:  # one communicator: its pool, events and side stream are reused
        torch.cuda.synchronize()
        if op == "ef":
            state = bc.MXFP6ErrorFeedbackState(x.size, world, 0)
            sr = [state._raw(s) for s in state.tensors()]
            torch.cuda.synchronize()
            for step in range(2):
                N.check(N.C.bagua_centralized_mxfp6_error_feedback(comm.handle, ctypes.byref(raw), 1, ctypes.byref(sr[0]),
                                                                   ctypes.byref(sr[1])), f"MXFP6 error feedback, step {step}")
                comm.synchronize()
                out[f"ef{step}"] = _host(t)
                out[f"worker{step}"] = _host(state.worker_residual)
                out[f"server{step}"] = _host(state.server_residual)
                reset()
            continue
        N.check(N.C.bagua_centralized_low_precision_pipelined(comm.handle, ctypes.byref(raw), 1, N.COMPRESSION_MXFP6,
                                                              int(op)), f"pipelined MXFP6 op, pieces={op}")
        comm.synchronize()
        out[f"t{plain}"] = _host(t)
        plain += 1
        reset()
    torch.cuda.synchronize()
    comm.barrier()
    np.savez(os.path.join(workdir, f"out{rank}.npz"), **out)


if __name__ == "__main__":
    main()

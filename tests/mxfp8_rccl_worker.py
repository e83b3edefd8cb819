"""Worker of tests/test_gpu_mxfp8_op.py: one rank of a real multi-process RCCL
communicator (all ranks on the one GPU, a distinct NCCL_HOSTID each, as tests/rccl_worker.py)
running the pipelined centralized op with the MXFP8 codec.

usage: python mxfp8_rccl_worker.py <rank> <world> <workdir> <pieces,pieces,...>
Inputs come from <workdir>/inputs.npz (x<rank>), results go to <workdir>/out<rank>.npz: t<i>
is the tensor after the i-th op, each op starting from the input again."""
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
    schedules = [int(v) for v in sys.argv[4].split(",")]
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
    for i, pieces in enumerate(schedules):  # one communicator: its pool, events and side stream are reused
        torch.cuda.synchronize()
        N.check(N.C.bagua_centralized_low_precision_pipelined(comm.handle, ctypes.byref(raw), 1, N.COMPRESSION_MXFP8,
                                                              pieces), f"pipelined MXFP8 op, pieces={pieces}")
        comm.synchronize()
        out[f"t{i}"] = _host(t)
        t.copy_(torch.from_numpy(x.copy()).cuda())
    torch.cuda.synchronize()
    comm.barrier()
    np.savez(os.path.join(workdir, f"out{rank}.npz"), **out)


if __name__ == "__main__":
    main()

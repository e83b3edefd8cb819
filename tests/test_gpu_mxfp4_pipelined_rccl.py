"""The pipelined MXFP4 centralized op (MXFP4.md, "Pipelined op") over real RCCL: every rank
its own process and communicator, all on the one GPU, RCCL's socket transport carrying the
two byte ranges of every piece as grouped send/recv (tests/mxfp4_rccl_worker.py; set up as
tests/test_gpu_rccl_procs.py: fresh child processes, a distinct NCCL_HOSTID each, a timeout
on every child).  Every rank's bytes must equal the numpy reference of the op."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

import mxfp4_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "mxfp4_rccl_worker.py")
F32 = 0
TIMEOUT_S = 90


@pytest.mark.parametrize("world", [2, 4])
def test_pipelined_mxfp4_over_rccl(tmp_path, world):
    """3 pieces, then the automatic count (pieces = 0) on the same communicator.  The chunk's
    segment is 10880 bytes, so BAGUA_PIPELINE_MIN_PIECE=4096 (read at the communicator's
    creation) makes the automatic schedule two pieces: both ops run pieced."""
    cs = 5 * 4096
    rng = np.random.default_rng(1200 + world)
    mag = np.repeat(10.0 ** rng.uniform(-3, 2, world * cs // 32), 32)
    xs = [(rng.standard_normal(world * cs) * mag * 1e-3).astype(np.float32) for _ in range(world)]
    want = R.centralized(xs, F32, True)
    np.savez(tmp_path / "inputs.npz", **{f"x{r}": x for r, x in enumerate(xs)})
    procs = []
    for r in range(world):
        env = dict(os.environ)
        env.update({"NCCL_HOSTID": f"bagua-test-rank-{r}", "NCCL_SOCKET_IFNAME": "lo", "NCCL_IB_DISABLE": "1",
                    "HSA_ENABLE_IPC_MODE_LEGACY": "0", "BAGUA_PIPELINE_MIN_PIECE": "4096"})
        log = open(tmp_path / f"rank{r}.log", "w")
        procs.append((subprocess.Popen([sys.executable, "-u", WORKER, str(r), str(world), str(tmp_path), "3,0"],
                                       stdout=log, stderr=subprocess.STDOUT, env=env, cwd=ROOT), log))
    failed = []
    for r, (p, log) in enumerate(procs):
        try:
            rc = p.wait(timeout=TIMEOUT_S)
        except subprocess.TimeoutExpired:
            for q, _ in procs:
                q.kill()
            rc = "timeout"
        log.close()
        if rc != 0:
            failed.append(r)
    if failed:
        tails = "\n".join(f"--- rank {r}:\n" + (tmp_path / f"rank{r}.log").read_text()[-1500:] for r in failed)
        pytest.fail(f"ranks {failed} failed:\n{tails}")
    for r in range(world):
        with np.load(tmp_path / f"out{r}.npz", allow_pickle=False) as z:
            for i, pieces in enumerate((3, 0)):
                assert np.array_equal(z[f"t{i}"], want[r].view(np.uint8)), f"rank {r}, pieces={pieces}"

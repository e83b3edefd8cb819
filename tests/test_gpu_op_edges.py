"""GPU tests of the comm ops on hostile gradients, in sum and average mode, on every
dispatch path of csrc/runtime/comm_ops.cpp (tests/op_edge_cases.py PATHS).

One test function per path.  It creates one loopback group, checks once -- on benign data,
from the names of the kernels launched on rank 0's thread (bagua_time_next_kernels) -- that
the op took the path the table says, then runs every input class in both modes: every rank's
result must equal the oracle's simulation of the reference op sequence, NaN at the same
positions and every other value bit for bit (for the error-feedback op after each of two
steps, the four state tensors included; for the ring all four tensors)."""
import ctypes
import time

import numpy as np
import pytest
import torch

import op_edge_cases as E
from op_edge_cases import F32, MINMAX
from test_gpu_codec import assert_float_bits_equal
from test_gpu_multirank import dev, host, run_ranks

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_HIP = 1, 3
HUNG = []  # an op that did not return (or a HIP error): nothing more is started on the GPU


@pytest.fixture(scope="module")
def bc():
    import bagua_core
    return bagua_core


def run_all_ranks(fn, p, what):
    """run_ranks, and a rank that has not returned when its join timed out is a hang"""
    if HUNG:
        pytest.fail(f"not started: {HUNG[0]} did not return")
    returned = [False] * p

    def wrap(r):
        try:
            fn(r)
        finally:
            returned[r] = True

    try:
        run_ranks(wrap, p)
    finally:
        if not all(returned):
            HUNG.append(what)
    assert not HUNG, f"{what}: ranks {[r for r in range(p) if not returned[r]]} did not return"


class KernelNames:
    """the names of the kernels the library launches on this thread while armed"""

    def __init__(self, N, comm):
        self.N = N
        st = torch.cuda.ExternalStream(comm.stream_ptr())
        self.events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(32)]
        for a, b in self.events:
            a.record(st)
            b.record(st)
        self.names = []

    def __enter__(self):
        self.N.time_next_kernels(self.events)
        return self

    def __exit__(self, *exc):
        self.names = self.N.timed_kernel_names()
        self.N.check(self.N.K.bagua_time_next_kernels(None, None, 0), "disarm")
        return False


def check_path_taken(path, names):
    what = f"{path.id}: kernels on rank 0: {names}"
    assert 0 < len(names) < 32, f"{what}: the 32 armed slots must not run out"
    for item in path.must:
        if isinstance(item, tuple) and len(item) == 2 and isinstance(item[1], int):
            assert names.count(item[0]) >= item[1], f"{what}: {item[0]} fewer than {item[1]} times"
        elif isinstance(item, tuple):
            assert any(n in names for n in item), f"{what}: none of {item}"
        else:
            assert item in names, f"{what}: no {item}"
    for n in path.must_not:
        assert n not in names, f"{what}: {n} must not run on this path"


def op_call(N, path, average):
    """rank r's call of the path's entry point: f(comm, tensors by reference) -> status"""
    method = N.COMPRESSION_MINMAX_UINT8 if path.codec == MINMAX else N.COMPRESSION_ONEBIT
    C = N.C
    if path.op == "centralized":
        if path.entry == "synchronous":
            return lambda h, t: C.bagua_centralized_low_precision_synchronous(h, t[0], average, method)
        if path.entry == "unfused":
            return lambda h, t: C.bagua_centralized_low_precision_synchronous_unfused(h, t[0], average, method)
        return lambda h, t: C.bagua_centralized_low_precision_pipelined(h, t[0], average, method, path.pieces)
    if path.op == "ef":
        return lambda h, t: C.bagua_centralized_onebit_error_feedback(h, t[0], average, *t[1:], path.pieces)
    if path.entry == "synchronous":
        return lambda h, t: C.bagua_decentralized_low_precision_synchronous(h, *t, method)
    if path.entry == "unfused":
        return lambda h, t: C.bagua_decentralized_low_precision_synchronous_unfused(h, *t, method)
    return lambda h, t: C.bagua_decentralized_low_precision_pipelined(h, *t, method, path.pieces)


def launch(bc, comms, path, average, tensors, what, num_elem=None, states=None, timed=False):
    """the op on p host threads; tensors[r]: rank r's device tensors in argument order.
    Returns the kernel names of rank 0's thread when `timed`."""
    N = bc._native
    call = op_call(N, path, average)
    torch.cuda.synchronize()
    seen = []

    def rank(r):
        raws = [bc.BaguaTensorPy(t, f"g{r}.{i}").raw() for i, t in enumerate(tensors[r])]
        if num_elem is not None:
            raws[0].num_elem = num_elem
        if states is not None:
            raws += [states[r]._raw(t) for t in states[r].tensors()]
        refs = [ctypes.byref(x) for x in raws]
        if timed and r == 0:
            with KernelNames(N, comms[0]) as k:
                rc = call(comms[r].handle, refs)
            seen.extend(k.names)
        else:
            rc = call(comms[r].handle, refs)
        if rc == ERR_HIP:  # a failed launch or a fault: the device is not used again
            HUNG.append(what)
        N.check(rc, f"{what} rank {r}")

    run_all_ranks(rank, path.p, what)
    return seen


def run_case(bc, oracle_c, comms, path, cls, average, states=None, timed=False):
    what = f"{path.id} {cls} average={average}"
    p, dt = path.p, path.dtype
    data = E.inputs(path, cls)
    want = E.reference(oracle_c, path, cls, average)
    if path.op == "ring":
        dts = {k: [dev(a, dt) for a in data[k]] for k in "twlr"}
        names = launch(bc, comms, path, average, [[dts[k][r] for k in "twlr"] for r in range(p)], what, timed=timed)
        for k, wk in zip("twlr", want):
            for r in range(p):
                assert_float_bits_equal(host(dts[k][r], dt), wk[r], dt, f"{what}: {k} rank {r}")
        return names
    if path.op == "ef":
        for st in states:
            st.zero_()
        names = []
        for step, (xs, (outs_want, states_want)) in enumerate(zip(data, want)):
            ts = [dev(x, dt) for x in xs]
            got = launch(bc, comms, path, average, [[t] for t in ts], f"{what} step {step}", states=states,
                         timed=timed and step == 0)
            names = names or got
            outs = [host(t, dt) for t in ts]
            for r in range(p):
                assert_float_bits_equal(outs[r], outs_want[r], dt, f"{what} step {step}: rank {r}")
                assert_float_bits_equal(outs[r], outs[0], dt, f"{what} step {step}: rank {r} against rank 0")
                for name, t, w in zip(("worker carry", "worker scales", "server carry", "server scale"),
                                      states[r].tensors(), states_want[r]):
                    assert_float_bits_equal(host(t, F32), w, F32, f"{what} step {step}: rank {r} {name}")
        return names
    xs, num_elem = data
    ts = [dev(x, dt) for x in xs]
    names = launch(bc, comms, path, average, [[t] for t in ts], what, num_elem=num_elem, timed=timed)
    outs = [host(t, dt) for t in ts]
    for r in range(p):
        assert_float_bits_equal(outs[r], want[r], dt, f"{what}: rank {r}")
        assert_float_bits_equal(outs[r], outs[0], dt, f"{what}: rank {r} against rank 0")
    return names


@pytest.mark.parametrize("path", E.PATHS, ids=lambda q: q.id)
def test_op_on_hostile_inputs(bc, oracle_c, path, monkeypatch):
    from bagua_core.communicator import loopback_communicators
    if HUNG:
        pytest.fail(f"not started: {HUNG[0]} did not return")
    for k, v in path.env:
        monkeypatch.setenv(k, v)
    t0 = time.perf_counter()
    comms = loopback_communicators(path.p, 0)  # after the switches: the schedule config is read here
    states = None
    if path.op == "ef":
        states = [bc.OneBitErrorFeedbackState(path.p * path.size, path.p, 0) for _ in range(path.p)]
    for cls in path.classes:
        for average in (1, 0) if path.op != "ring" else (1,):
            # the path really is the path: checked once, on the first case (benign data; the
            # partially valid op has tail classes only, and a benign valid part)
            first = cls == path.classes[0] and average == 1
            names = run_case(bc, oracle_c, comms, path, cls, average, states, timed=first)
            if first:
                print(f"[op-edges] {path.id}: {names}")
                check_path_taken(path, names)
    print(f"[op-edges] {path.id}: {time.perf_counter() - t0:.2f} s")


def test_every_virtual_rank_has_its_own_stream(bc):
    """torch's stream pool wraps after 32 streams; two ranks of a loopback group on one
    stream share the ops' per-stream workspace and race on it (found by the p = 33 rows:
    ranks 0 and 32 requantised their chunks with a wrong header now and then)"""
    from bagua_core.communicator import loopback_communicators
    for p in (32, 33, 40):
        comms = loopback_communicators(p, 0)
        assert len({c.stream_ptr() for c in comms}) == p


@pytest.mark.parametrize("dtype", [E.F32, E.BF16])
def test_minmax_shape_with_unaligned_alltoall_is_refused(bc, dtype):
    """MinMax at p = 3, cs = 3076: S % p != 0, the alltoall of the reference asserts
    (communicators/mod.rs:603-607).  Every rank gets INVALID_ARG from every entry point before
    anything is posted, and its gradient is untouched."""
    from bagua_core.communicator import loopback_communicators
    N = bc._native
    p, cs = E.REFUSED_MINMAX_SHAPE
    xs = E.build("benign", p, cs, dtype, E.case_rng("refused", dtype))
    comms = loopback_communicators(p, 0)
    ts = [dev(x, dtype) for x in xs]
    torch.cuda.synchronize()
    rcs = {}

    def rank(r):
        raw = bc.BaguaTensorPy(ts[r], f"g{r}").raw()
        h, t, m = comms[r].handle, ctypes.byref(raw), N.COMPRESSION_MINMAX_UINT8
        rcs[r] = [N.C.bagua_centralized_low_precision_synchronous(h, t, 1, m),
                  N.C.bagua_centralized_low_precision_synchronous_unfused(h, t, 0, m),
                  N.C.bagua_centralized_low_precision_pipelined(h, t, 1, m, 3)]

    run_all_ranks(rank, p, "refused shape")
    assert all(rcs[r] == [ERR_INVALID_ARG] * 3 for r in range(p)), rcs
    for r in range(p):
        assert np.array_equal(host(ts[r], dtype).view(np.uint8), xs[r].view(np.uint8)), f"rank {r} changed"

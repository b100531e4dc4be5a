"""Shared by tests/test_splits_batch_emu.py (CPU driver of the phase bodies) and tests/test_splits_batch.py (the product on
the GPU): the cases of the batched circular split weights and their checks.  The tolerances are
those of tests/test_split_weights.py: 1e-6 * max(1, max|x|) against a second solver, and common.kkt_violation < 1e-9 as the
certificate that needs no solver."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import common
from fastneighbornet_amd import _capi
from oracle import csw_oracle as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "fastneighbornet_amd", "csrc")
EMU_SRCS = [os.path.join(EMU_DIR, "fnn_splits_batch_emu.cpp")] + \
    [os.path.join(CSRC, f) for f in ("fnn_small_splits.h", "fnn_small.h", "fnn_engine.h", "fnn_core.h")] + [os.path.join(ROOT, "include", "fastnn.h")]

ROUTE_CLOSED_FORM, ROUTE_FROM_BELOW = 0, 1
GIVEUP_CAPACITY = 1
SENTINEL = -77.0


def newer(out, srcs):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(s) for s in srcs)


def emu_api():
    """tests/emu/fnn_splits_batch_emu.cpp as a shared library, behind the same ctypes view as the product."""
    out = os.path.join(EMU_DIR, "build", "libfnn_splits_batch_emu.so")
    if newer(out, EMU_SRCS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                               "-o", out, EMU_SRCS[0]])
    a = _capi.bind_splits_batch(_capi.Api(C.CDLL(out), "emu_", engine=False))
    a._fn("split_weights_batch_giveups", C.c_int64, [C.POINTER(C.c_int32), C.c_int64])
    return a


@functools.lru_cache(maxsize=None)
def _oracle_mod():
    from oracle import nnet_oracle
    nnet_oracle.lib()
    return nnet_oracle


@functools.lru_cache(maxsize=None)
def synth_batch(n, B, seed0=40):
    """B problems of n taxa, uniform53 and dec4 in turn, with the order oracle's circular orders.  Computed once."""
    o = _oracle_mod()
    D = np.stack([o.synth(n, seed0 + b, ("uniform53", "dec4")[b % 2]) for b in range(B)])
    if n <= 3:
        orders = np.tile(np.arange(n + 1, dtype=np.int32), (B, 1))
    else:
        orders = np.stack([o.run(D[b])[0] for b in range(B)]).astype(np.int32)
    D.setflags(write=False)
    orders.setflags(write=False)
    return D, orders


def batch_size(n, max_n):
    return 2 if n >= max_n else (4 if n >= 64 else 6)


@functools.lru_cache(maxsize=None)
def circ_batch(sizes, density):
    """One circular metric with known weights per size: [(D, order, weights)] (tests/test_split_weights.py: circ_instance)."""
    from test_split_weights import circ_instance
    return tuple(circ_instance(n, 30 + n, density=density) for n in sizes)


@functools.lru_cache(maxsize=None)
def tree_batch(n, B=3):
    o = _oracle_mod()
    D = np.stack([common.tree_metric(n, 70 + b) for b in range(B)])
    orders = np.stack([o.run(D[b])[0] for b in range(B)]).astype(np.int32)
    D.setflags(write=False)
    return D, orders


@functools.lru_cache(maxsize=None)
def nnls_reference(n, B, seed0=40):
    """scipy's Lawson-Hanson on the live design matrix, once per batch."""
    import scipy.optimize as so
    D, orders = synth_batch(n, B, seed0)
    return tuple(so.nnls(W.live_design_matrix(n, orders[b]), W.packed_distances(D[b]), maxiter=10 ** 7)[0] for b in range(B))


def run(a, D, orders, ld=None, stride=None, **kw):
    B, n = D.shape[0], D.shape[1]
    return _capi.run_splits_batch(a, D.ctypes.data, n, ld or n, stride or n * n, B, orders, **kw)


def assert_kernel_only(st, B):
    """The cases have to exercise the kernel's method, not the fallback behind it."""
    assert st.n_problems == B and st.n_fallback == 0 and st.n_kernel + st.n_closed_form == B, st.as_dict()


def row(sw, b):
    """Problem b's counters, for a message (sw: a record array, or the dict of arrays that split_weights_batch returns)."""
    return {k: sw[k][b] for k in ("route", "certified", "kkt_violation", "outer_iterations", "entered", "departed", "n_set_aside", "free_set_peak")}


def assert_optimal(D, orders, w, sw, tag):
    for b in range(D.shape[0]):
        viol = common.kkt_violation(D[b], orders[b], w[b])
        assert viol < 1e-9, (tag, b, viol, row(sw, b))
        assert sw["certified"][b] == 1 and sw["kkt_violation"][b] <= 1e-9, (tag, b, row(sw, b))
        assert (w[b] >= 0).all(), (tag, b, w[b].min())
        assert sw["nsplits"][b] == int((w[b] > 1e-6).sum()), (tag, b)


# ---- the cases of both suites; `call(D, orders, **kw)` returns (weights, per-problem stats, call stats) --------------

def orders_for(D, orders, orders_of):
    """The orders a test runs under: the order oracle's, or - orders_of given (the product's order batch on the GPU) - what that
    returns, which must be the same orders."""
    if orders_of is None:
        return orders
    got = np.ascontiguousarray(orders_of(np.ascontiguousarray(D)), dtype=np.int32)
    assert (got == orders).all()
    return got


def check_parity(call, n, max_n, with_nnls=True, orders_of=None):
    B = batch_size(n, max_n)
    D, orders = synth_batch(n, B)
    orders = orders_for(D, orders, orders_of)
    w, sw, st = call(D, orders)
    assert_kernel_only(st, B)
    assert_optimal(D, orders, w, sw, ("parity", n))
    assert st.lds_bytes <= 163840 and st.block_threads in (256, 512, 1024) and st.capacity == min(n * (n - 1) // 2, 6 * n)
    below = sw["route"] == ROUTE_FROM_BELOW
    assert (sw["free_set_peak"][below] <= st.capacity).all() and (sw["entered"][below] >= sw["nsplits"][below]).all()
    if with_nnls and n <= 33:
        for b, xs in enumerate(nnls_reference(n, B)):
            assert np.abs(w[b] - xs).max() <= 1e-6 * max(1.0, np.abs(xs).max()), (n, b, np.abs(w[b] - xs).max())
    return w, sw, st


def check_closed_form(call, sizes=(6, 15, 24)):
    for D, order, known in circ_batch(sizes, 1.0):
        w, sw, st = call(D[None], order[None])
        assert_kernel_only(st, 1)
        assert sw["route"][0] == ROUTE_CLOSED_FORM and st.n_closed_form == 1
        assert np.abs(w[0] - known).max() < 1e-9, (D.shape[0], np.abs(w[0] - known).max())


def check_zeros_to_find(call, sizes=(15, 24)):
    for D, order, known in circ_batch(sizes, 0.1):
        w, sw, st = call(D[None], order[None])
        assert_kernel_only(st, 1)
        assert sw["route"][0] == ROUTE_FROM_BELOW and st.n_kernel == 1
        assert np.abs(w[0] - known).max() < 1e-6 * max(1.0, known.max()), (D.shape[0], np.abs(w[0] - known).max())
        assert sw["certified"][0] == 1


def check_tree_metric(call, n, orders_of=None):
    D, orders = tree_batch(n)
    orders = orders_for(D, orders, orders_of)
    w, sw, st = call(D, orders)
    assert_kernel_only(st, D.shape[0])
    assert_optimal(D, orders, w, sw, ("tree", n))
    assert (sw["outer_iterations"] <= 40 * n + 1000).all()
    assert (sw["nsplits"] <= 2 * n - 3).all(), sw["nsplits"]


def padded(D, ld, stride, tail=7):
    """The problems of D inside a larger array that is NaN everywhere else."""
    B, n = D.shape[0], D.shape[1]
    buf = np.full(B * stride + tail, np.nan)
    for b in range(B):
        buf[b * stride: b * stride + n * ld].reshape(n, ld)[:, :n] = D[b]
    return buf


def check_padding(a_run, n, max_n):
    """a_run(ptr_array, n, ld, stride, B, orders) -> (w, sw, st)"""
    B = batch_size(n, max_n)
    D, orders = synth_batch(n, B)
    ld = n + 3
    stride = n * ld + 5
    buf = padded(D, ld, stride)
    w0, _, _ = a_run(np.ascontiguousarray(D), n, n, n * n, B, orders)
    w1, sw, st = a_run(buf, n, ld, stride, B, orders)
    assert_kernel_only(st, B)
    assert w0.tobytes() == w1.tobytes()
    assert np.isfinite(w1).all()


def check_chunking(call, n, monkeypatch):
    D, orders = synth_batch(n, 8, seed0=500)
    w1, sw1, s1 = call(D, orders)
    monkeypatch.setenv("FNN_BATCH_CHUNK", "3")
    w2, sw2, s2 = call(D, orders)
    monkeypatch.delenv("FNN_BATCH_CHUNK")
    assert s1.chunks == 1 and s2.chunks == 3
    assert w1.tobytes() == w2.tobytes()
    assert (sw1["outer_iterations"] == sw2["outer_iterations"]).all()
    assert_kernel_only(s2, 8)
    assert_optimal(D, orders, w2, sw2, ("chunked", n))


def check_determinism(call, n):
    D, orders = synth_batch(n, 4)
    w1, sw1, _ = call(D, orders)
    w2, sw2, _ = call(D, orders)
    assert w1.tobytes() == w2.tobytes()
    assert (sw1["kkt_violation"].view(np.int64) == sw2["kkt_violation"].view(np.int64)).all()

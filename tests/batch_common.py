"""Shared by tests/test_batch_emu.py (CPU driver of the phase bodies) and tests/test_batch.py (the product on the GPU): the
cases of the batched small-problem path and their comparison with the oracle, event by event."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import inputs
from fastneighbornet_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "fastneighbornet_amd", "csrc")
EMU_SRCS = [os.path.join(EMU_DIR, "fnn_batch_emu.cpp")] + [os.path.join(CSRC, f) for f in ("fnn_small.h", "fnn_engine.h", "fnn_core.h")] + \
    [os.path.join(ROOT, "include", "fastnn.h"), os.path.join(EMU_DIR, "fnn_small_emu.h"), os.path.join(CSRC, "fnn_small_splits.h")]

CLASSES = ("uniform53", "dec4", "tree", "treenoise", "dup", "neg", "outgroup")
SMALL_SIZES = (4, 5, 6, 7, 8, 9, 16, 33, 63, 64, 65, 100, 127, 128)   # ... and lds_max_n
INT_FIELDS = ("m_before", "c_before", "cx_id", "cy_id", "x_id", "y_id", "kind", "u_id")
SENTINEL = -77


def newer(out, srcs):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(s) for s in srcs)


def emu_batch_api():
    """tests/emu/fnn_batch_emu.cpp as a shared library, behind the same ctypes view as the product."""
    out = os.path.join(EMU_DIR, "build", "libfnn_batch_emu.so")
    if newer(out, EMU_SRCS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                               "-o", out, EMU_SRCS[0]])
    return _capi.bind_batch(_capi.Api(C.CDLL(out), "emu_", engine=False))


@functools.lru_cache(maxsize=None)
def _oracle_mod():
    from oracle import nnet_oracle
    nnet_oracle.lib()
    return nnet_oracle


@functools.lru_cache(maxsize=None)
def class_batch(n):
    """One batch per n holding all classes (seed 3), with the oracle's (order, events) per problem.  Computed once."""
    o = _oracle_mod()
    D = np.stack([inputs.make(n, c, 3, o) for c in CLASSES])
    D.setflags(write=False)
    return D, tuple(o.run(D[k])[:2] for k in range(len(CLASSES)))


@functools.lru_cache(maxsize=None)
def dec4_batch(n, B, seed0=100):
    o = _oracle_mod()
    D = np.stack([o.synth(n, seed0 + b, "dec4") for b in range(B)])
    D.setflags(write=False)
    return D, tuple(o.run(D[k])[:2] for k in range(B))


def run(a, D, ld=None, stride=None, **kw):
    B, n = D.shape[0], D.shape[1]
    return _capi.run_batch(a, D.ctypes.data, n, ld or n, stride or n * n, B, **kw)


def assert_same_events(ev, nev, ref_ev, tag):
    assert nev == len(ref_ev), (tag, nev, len(ref_ev))
    got = ev[:nev]
    for f in INT_FIELDS:
        assert (got[f] == ref_ev[f]).all(), (tag, f, got[f], ref_ev[f])
    assert (got["best"].view(np.int64) == ref_ev["best"].view(np.int64)).all(), (tag, "best")
    assert (got["entries"] == ref_ev["entries"]).all(), (tag, "entries")


def assert_matches_oracle(orders, ev, nev, refs, tag):
    assert len(refs) == orders.shape[0]
    for b, (o_ref, e_ref) in enumerate(refs):
        assert (orders[b] == o_ref).all(), (tag, b, orders[b], o_ref)
        assert_same_events(ev[b], int(nev[b]), e_ref, (tag, b))


# ---- the cases of both suites; `a` is the bound library ------------------------------------------------------------

def check_parity(a, n):
    D, refs = class_batch(n)
    orders, ev, nev, st = run(a, D, events=True, validate=False)
    assert_matches_oracle(orders, ev, nev, refs, n)
    assert st.n_lds == len(CLASSES) and st.n_fallback == 0 and st.n_problems == len(CLASSES)
    assert st.n_events == sum(len(e) for _, e in refs)
    assert st.lds_bytes <= 163840 and st.block_threads in (256, 512, 1024)


def check_identities(a):
    for n in (1, 2, 3):
        D = np.full((4, n, n), np.nan)   # never read
        orders, ev, nev, st = run(a, D, events=True)
        assert (orders == np.arange(n + 1, dtype=np.int32)[None, :]).all()
        assert (nev == 0).all()
        assert st.t_kernel_s == 0 and st.n_lds == 0 and st.n_fallback == 0 and st.chunks == 0
    orders, _, _, st = run(a, np.zeros((0, 8, 8)))   # batch == 0 is FNN_OK
    assert orders.shape == (0, 9) and st.n_problems == 0


def check_many(a):
    n, B = 24, 1000
    D0, refs = dec4_batch(n, B - 1)
    D = np.concatenate([D0, D0[:1]])             # the matrix of index 0 again at index 999
    orders, ev, nev, st = run(a, D, events=True)
    for b in range(B):
        assert (orders[b] == refs[b % (B - 1)][0]).all(), b
    assert nev[0] == nev[B - 1]
    assert ev[0].tobytes() == ev[B - 1].tobytes()
    assert_same_events(ev[B - 1], int(nev[B - 1]), refs[0][1], "index 999")
    assert st.n_lds == B


def check_padding(a, n):
    D, refs = class_batch(n)
    B, ld = D.shape[0], n + 3
    stride = n * ld + 5
    buf = np.full(B * stride + 7, np.nan)
    for b in range(B):
        rows = buf[b * stride: b * stride + n * ld].reshape(n, ld)
        rows[:, :n] = D[b]
    orders, ev, nev, _ = _capi.run_batch(a, buf.ctypes.data, n, ld, stride, B, events=True, validate=True)
    assert_matches_oracle(orders, ev, nev, refs, ("padded", n))


def check_chunking(a, n, monkeypatch):
    D, refs = dec4_batch(n, 10, seed0=500)
    o1, e1, n1, s1 = run(a, D, events=True)
    monkeypatch.setenv("FNN_BATCH_CHUNK", "3")
    o2, e2, n2, s2 = run(a, D, events=True)
    monkeypatch.delenv("FNN_BATCH_CHUNK")
    assert s1.chunks == 1 and s2.chunks == 4
    assert (o1 == o2).all() and (n1 == n2).all() and e1.tobytes() == e2.tobytes()
    assert_matches_oracle(o2, e2, n2, refs, ("chunked", n))


def check_validation(a, monkeypatch):
    n, B = 16, 5
    good, _ = dec4_batch(n, B, seed0=700)
    for what in ("asymmetric", "asymmetric, chunks of 2", "nan", "diagonal"):
        monkeypatch.delenv("FNN_BATCH_CHUNK", raising=False)
        D = good.copy()
        if what == "asymmetric":
            D[3, 2, 5] += 0.5
        elif what == "asymmetric, chunks of 2":  # problem 3 is chunk 1, local index 1: the failure names the caller's index
            D[3, 2, 5] += 0.5
            monkeypatch.setenv("FNN_BATCH_CHUNK", "2")
        elif what == "nan":
            D[3, 2, 5] = D[3, 5, 2] = np.nan
        else:
            D[3, 4, 4] = 1e-3
        try:
            run(a, D, validate=True, fill=SENTINEL)
        except _capi.FnnError as e:
            assert e.code == -1, e
            assert "3" in str(e) and "problem 3" in str(e), e
            assert (e.orders == SENTINEL).all()
        else:
            raise AssertionError(f"{what}: the call did not fail")
    orders, _, _, _ = run(a, good, validate=True)
    orders2, _, _, _ = run(a, good, validate=False)
    assert (orders == orders2).all()
    D = good.copy()
    D[3, 2, 5] += 0.5                      # finite but asymmetric, no check asked for: the call still runs
    o3, _, _, _ = run(a, D, validate=False)
    assert (o3[[0, 1, 2, 4]] == orders[[0, 1, 2, 4]]).all()
    assert sorted(o3[3, 1:].tolist()) == list(range(1, n + 1))

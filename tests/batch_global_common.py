"""Shared by tests/test_batch_global_emu.py (CPU driver of the phase bodies) and tests/test_batch_global.py (the product on
the GPU): the cases of the batched path above the LDS limit - one workgroup per problem, the matrix in a working copy in
global memory (fnn_small_global.h) - and their comparison with the oracle, event by event."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import batch_common as bc
import inputs
from batch_common import assert_matches_oracle, class_batch, dec4_batch, run
from fastneighbornet_amd import _capi

EMU_SRCS = [os.path.join(bc.EMU_DIR, "fnn_batch_global_emu.cpp")] + \
    [os.path.join(bc.CSRC, f) for f in ("fnn_small_global.h", "fnn_small.h", "fnn_engine.h", "fnn_core.h")] + \
    [os.path.join(bc.ROOT, "include", "fastnn.h"), os.path.join(bc.EMU_DIR, "fnn_small_emu.h"), os.path.join(bc.CSRC, "fnn_small_splits.h")]

# 4: the special finish with no scan before it; 63, 64, 65 straddle a wave in the staging arrays; 141: the first size of the
# default route; 257: more positions than a 256-thread block
FORCED_SIZES = (4, 5, 6, 7, 8, 9, 16, 33, 63, 64, 65, 129, 141, 257)
LDS_CAP = 163840


def emu_global_api():
    """tests/emu/fnn_batch_global_emu.cpp as a shared library, behind the same ctypes view as the product."""
    out = os.path.join(bc.EMU_DIR, "build", "libfnn_batch_global_emu.so")
    if bc.newer(out, EMU_SRCS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                               "-o", out, EMU_SRCS[0]])
    return _capi.bind_batch(_capi.Api(C.CDLL(out), "emu_", engine=False))


@functools.lru_cache(maxsize=None)
def cap_batch(n):
    """uniform53 and tree at the cap, with the oracle's (order, events).  Computed once."""
    o = bc._oracle_mod()
    D = np.stack([inputs.make(n, c, 3, o) for c in ("uniform53", "tree")])
    D.setflags(write=False)
    return D, tuple(o.run(D[k])[:2] for k in range(2))


def assert_global(st, B, refs):
    assert st.n_global == B and st.n_lds == 0 and st.n_fallback == 0 and st.n_problems == B, st.as_dict()
    assert st.n_events == sum(len(e) for _, e in refs)
    assert st.lds_bytes <= LDS_CAP and st.block_threads in (256, 512, 1024)


# ---- the cases of both suites; `a` is the bound library ------------------------------------------------------------

def check_forced_parity(a, n, monkeypatch):
    monkeypatch.setenv("FNN_BATCH_ROUTE", "global")
    D, refs = class_batch(n)
    orders, ev, nev, st = run(a, D, events=True, validate=False)
    assert_matches_oracle(orders, ev, nev, refs, ("global", n))
    assert_global(st, len(bc.CLASSES), refs)


def check_threads(a, threads, monkeypatch):
    n = 300
    monkeypatch.setenv("FNN_BATCH_ROUTE", "global")
    monkeypatch.setenv("FNN_BATCH_THREADS", str(threads))
    D, refs = class_batch(n)
    orders, ev, nev, st = run(a, D, events=True)
    assert st.block_threads == threads
    assert_matches_oracle(orders, ev, nev, refs, ("threads", threads))
    assert_global(st, len(bc.CLASSES), refs)


def check_default_route(a, monkeypatch):
    """No override: 8 problems of 141 taxa take the new kernel.  Returns what the call gave, for the GPU's engine leg."""
    monkeypatch.delenv("FNN_BATCH_ROUTE", raising=False)
    D, refs = dec4_batch(141, 8, seed0=1100)
    assert a.batch_global_min_batch(141) <= 8
    orders, ev, nev, st = run(a, D, events=True)
    assert st.n_global == 8 and st.n_fallback == 0 and st.n_lds == 0
    assert_matches_oracle(orders, ev, nev, refs, "default route")
    return D, orders, ev, nev


def check_cap(a, monkeypatch):
    n = a.batch_global_max_n()
    assert n >= 141
    monkeypatch.setenv("FNN_BATCH_ROUTE", "global")
    D, refs = cap_batch(n)
    orders, ev, nev, st = run(a, D, events=True)
    assert_matches_oracle(orders, ev, nev, refs, ("cap", n))
    assert_global(st, 2, refs)


def above_cap_batch(a):
    """n = cap + 1 and the smallest batch that would take the new route if the cap were higher (the problems: dec4)."""
    n = a.batch_global_max_n() + 1
    B = int(max(a.batch_global_min_batch(n), a.batch_global_min_batch(n - 1), 4))
    o = bc._oracle_mod()
    return np.stack([o.synth(n, 1200 + b, "dec4") for b in range(B)])


def check_many(a, monkeypatch):
    n, B = 24, 600
    monkeypatch.setenv("FNN_BATCH_ROUTE", "global")
    monkeypatch.setenv("FNN_BATCH_CHUNK", "256")
    D0, refs = dec4_batch(n, 999)                # (the batch of batch_common.check_many: its oracle runs are shared)
    D0, refs = D0[:B - 1], refs[:B - 1]
    D = np.concatenate([D0, D0[:1]])             # the matrix of index 0 again at index 599
    orders, ev, nev, st = run(a, D, events=True)
    assert st.chunks == 3 and st.n_global == B
    for b in range(B):
        assert (orders[b] == refs[b % (B - 1)][0]).all(), b
    assert nev[0] == nev[B - 1]
    assert ev[0].tobytes() == ev[B - 1].tobytes()
    bc.assert_same_events(ev[B - 1], int(nev[B - 1]), refs[0][1], "index 599")


def padded(D):
    """The problems of D behind ld = n + 3, stride = n * ld + 5, padding NaN."""
    B, n = D.shape[0], D.shape[1]
    ld = n + 3
    stride = n * ld + 5
    buf = np.full(B * stride + 7, np.nan)
    for b in range(B):
        buf[b * stride: b * stride + n * ld].reshape(n, ld)[:, :n] = D[b]
    return buf, ld, stride


def check_padding(a, n, monkeypatch):
    monkeypatch.setenv("FNN_BATCH_ROUTE", "global")
    D, refs = class_batch(n)
    buf, ld, stride = padded(D)
    before = buf.tobytes()
    orders, ev, nev, st = _capi.run_batch(a, buf.ctypes.data, n, ld, stride, D.shape[0], events=True, validate=True)
    assert_matches_oracle(orders, ev, nev, refs, ("padded", n))
    assert_global(st, D.shape[0], refs)
    assert buf.tobytes() == before               # the caller's array, padding included, is as it was


def check_validation(a, monkeypatch):
    n, B = 141, 5
    monkeypatch.setenv("FNN_BATCH_ROUTE", "global")
    good, _ = dec4_batch(n, B, seed0=1300)
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
            run(a, D, validate=True, fill=bc.SENTINEL)
        except _capi.FnnError as e:
            assert e.code == -1, e
            assert "problem 3" in str(e), e
            assert (e.orders == bc.SENTINEL).all()
        else:
            raise AssertionError(f"{what}: the call did not fail")
    orders, _, _, st = run(a, good, validate=True)
    assert st.n_global == B
    D = good.copy()
    D[3, 2, 5] += 0.5                      # finite but asymmetric, no check asked for: the call still runs
    o3, _, _, _ = run(a, D, validate=False)
    assert (o3[[0, 1, 2, 4]] == orders[[0, 1, 2, 4]]).all()
    assert sorted(o3[3, 1:].tolist()) == list(range(1, n + 1))


def check_asymmetric_like_lds(a, a_lds, monkeypatch):
    """validate off, every problem asymmetric (n = 64, which both routes serve): the same orders and event bytes as the LDS
    route gives - the initial sums take D[j][k] above the diagonal and D[k][j] below it, never the transposed entry."""
    good, _ = class_batch(64)
    D = good.copy()
    rng = np.random.default_rng(5)
    D += np.triu(rng.uniform(0.0, 0.25, D.shape), 1)
    monkeypatch.delenv("FNN_BATCH_ROUTE", raising=False)
    o1, e1, n1, s1 = run(a_lds, D, events=True)
    monkeypatch.setenv("FNN_BATCH_ROUTE", "global")
    o2, e2, n2, s2 = run(a, D, events=True)
    assert s1.n_lds == D.shape[0] and s2.n_global == D.shape[0]
    assert (o1 == o2).all() and (n1 == n2).all() and e1.tobytes() == e2.tobytes()

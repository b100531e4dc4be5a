"""Shared by tests/test_ragged_emu.py (CPU driver of the phase bodies) and tests/test_ragged.py (the product on the GPU): the
cases of the ragged batch calls (problems of different sizes in one call) and their checks.

The order checks are those of tests/batch_common.py (the oracle's order and events per problem, event by event and bit by bit
in `best`), the weight checks those of tests/splits_batch_common.py: certified, common.kkt_violation < 1e-9 recomputed on the
host, 1e-6 * max(1, max|x|) against scipy's Lawson-Hanson on the split-weight oracle's design matrix (n <= 33, where that
module computes it), and bit-equality with the same-size kernel route on the problem alone."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import batch_common as bc
import inputs
import splits_batch_common as sc
from fastneighbornet_amd import _capi

EMU_SRCS = [os.path.join(bc.EMU_DIR, "fnn_ragged_emu.cpp")] + \
    [os.path.join(bc.CSRC, f) for f in ("fnn_small_splits.h", "fnn_small.h", "fnn_engine.h", "fnn_core.h")] + \
    [os.path.join(bc.ROOT, "include", "fastnn.h"), os.path.join(bc.EMU_DIR, "fnn_small_emu.h")]

SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 16, 33, 63, 64, 65, 96, 97, 128)   # ... and lds_max_n
SENTINEL = -77
NO_EVENTS = np.zeros(0, dtype=_capi.EVENT_DTYPE)


def emu_api():
    """tests/emu/fnn_ragged_emu.cpp as a shared library, behind the same ctypes view as the product."""
    out = os.path.join(bc.EMU_DIR, "build", "libfnn_ragged_emu.so")
    if bc.newer(out, EMU_SRCS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                               "-o", out, EMU_SRCS[0]])
    a = _capi.bind_ragged(_capi.Api(C.CDLL(out), "emu_", engine=False))
    a._fn("batch_lds_max_n", C.c_int32, [])
    a._fn("split_weights_batch_max_n", C.c_int32, [])
    a._fn("split_weights_ragged_giveups", C.c_int64, [C.POINTER(C.c_int32), C.c_int64])
    return a


@functools.lru_cache(maxsize=None)
def problem(n, k):
    """Problem number k of a mixed batch: (matrix, (oracle's order, oracle's events)); the input class follows k.  Once."""
    o = bc._oracle_mod()
    if n <= 3:
        D = o.synth(n, 3 + k, "uniform53") if n >= 2 else np.zeros((n, n))
        D.setflags(write=False)
        return D, (np.arange(n + 1, dtype=np.int32), NO_EVENTS)
    D = np.ascontiguousarray(inputs.make(n, bc.CLASSES[k % len(bc.CLASSES)], 3 + k, o))
    D.setflags(write=False)
    return D, tuple(o.run(D)[:2])


def mixed(sizes, seed=11):
    """The sizes in an order shuffled by the seed (None: as given): ([matrix], [(order, events)])."""
    sizes = [int(s) for s in (sizes if seed is None else np.random.default_rng(seed).permutation(np.array(sizes)))]
    got = [problem(n, k) for k, n in enumerate(sizes)]
    return [g[0] for g in got], [g[1] for g in got]


def mixed_sizes(lds_max_n, low=1):
    return tuple(n for n in SIZES + (lds_max_n,) if n >= low)


class Layout:
    """The matrices in ONE buffer that is NaN wherever no matrix entry lies: NaN gaps of 1 to 4 doubles between the
    problems, every third problem with ld = n + 3, the first dense problem of n >= 8 at an ODD offset from the 16-byte
    aligned base (element loads in the in-place entries) and the next dense one at an even offset (16-byte loads).
    nan_below: problems of fewer taxa get no entries at all (the order calls never read them)."""

    def __init__(self, mats, nan_below=0):
        ns = [m.shape[0] for m in mats]
        lds, offs, cur = [], [], 0
        self.odd = self.aligned = None
        for k, n in enumerate(ns):
            ld = n + 3 if k % 3 == 1 else n
            cur += k % 4 + 1
            if ld == n and n >= 8 and self.odd is None:
                self.odd = k
                cur += 1 - cur % 2
            elif ld == n and n >= 8 and self.aligned is None:
                self.aligned = k
                cur += cur % 2
            offs.append(cur)
            lds.append(ld)
            cur += max((n - 1) * ld + n, 0)
        raw = np.full(cur + 4, np.nan)
        shift = (-raw.ctypes.data // 8) % 2          # (numpy allocates on 16-byte boundaries; this makes no assumption of it)
        self.buf = raw[shift: shift + cur + 2]
        assert self.buf.ctypes.data % 16 == 0
        for m, n, ld, off in zip(mats, ns, lds, offs):
            if n >= max(nan_below, 1):
                rows = np.lib.stride_tricks.as_strided(self.buf[off:], shape=(n, n), strides=(ld * 8, 8))
                rows[:, :] = m
        self.offsets = np.array(offs, dtype=np.int64)
        self.ns = np.array(ns, dtype=np.int32)
        self.lds = np.array(lds, dtype=np.int64)

    def add_shared(self, j):
        """One more problem: the storage of problem j again."""
        self.offsets = np.append(self.offsets, self.offsets[j])
        self.ns = np.append(self.ns, self.ns[j])
        self.lds = np.append(self.lds, self.lds[j])


class Driver:
    """One library and one entry: the host entry, or the in-place entry (`place(buf)` -> (address, what keeps it alive): the
    buffer itself for the CPU driver, a copy on the GPU for the product)."""

    def __init__(self, api, on_device=False, place=None):
        self.api, self.on_device = api, on_device
        self.place = place or (lambda buf: (buf.ctypes.data, buf))

    def orders(self, L, **kw):
        ptr, keep = self.place(L.buf)
        out = _capi.run_ragged(self.api, ptr, L.offsets, L.ns, L.lds, on_device=self.on_device, **kw)
        del keep
        return out

    def weights(self, L, orders, **kw):
        ptr, keep = self.place(L.buf)
        out = _capi.run_splits_ragged(self.api, ptr, L.offsets, L.ns, orders, L.lds, on_device=self.on_device, **kw)
        del keep
        return out


def assert_problem(orders, ev, nev, b, ref, tag):
    bc.assert_matches_oracle(orders[b][None], [ev[b]], [nev[b]], [ref], (tag, b))
    assert not ev[b][int(nev[b]):].tobytes().strip(b"\0"), (tag, b, "records behind the last event are not zero")


def outputs(orders, ev, nev, b):
    return orders[b].tobytes(), ev[b].tobytes(), int(nev[b])


# ---- the cases of both suites; `drv` is a Driver ---------------------------------------------------------------------

def check_mixed(drv, lds_max_n):
    """Case 1: every size and route edge in one call, in a shuffled order, padded, apart, misaligned and aligned."""
    mats, refs = mixed(mixed_sizes(lds_max_n))
    L = Layout(mats, nan_below=4)
    assert L.odd is not None and L.aligned is not None and L.offsets[L.odd] % 2 == 1 and L.offsets[L.aligned] % 2 == 0
    assert (L.lds > L.ns).any()
    orders, ev, nev, st = drv.orders(L, events=True, validate=True)
    for b, ref in enumerate(refs):
        assert_problem(orders, ev, nev, b, ref, "mixed")
    big = int((L.ns >= 4).sum())
    assert st.n_problems == len(mats) and st.n_lds == big and st.n_fallback == 0 and st.n_global == 0
    assert st.n_events == sum(len(e) for _, e in refs)
    assert 2 <= st.chunks <= 8, st.chunks                      # launches: one per size class, never one per size
    assert st.block_threads == 1024 and 0 < st.lds_bytes <= 163840 and st.lds_max_n == lds_max_n
    return L, orders, ev, nev


def check_numbering(drv, lds_max_n):
    """Case 2: the outputs follow the problems through another permutation, and a matrix met twice (once through a shared
    offset) gives the same bytes twice."""
    sizes = (5, 3, 64, 9, 65, 16, 97, 8, 33, 7)
    first = {}
    for seed in (11, 12):
        order = [int(s) for s in np.random.default_rng(seed).permutation(np.array(sizes))]
        probs = [problem(n, sizes.index(n)) for n in order]     # the SAME problems, in the seed's order
        L = Layout([p[0] for p in probs], nan_below=4)
        orders, ev, nev, _ = drv.orders(L, events=True)
        for b, n in enumerate(order):
            assert_problem(orders, ev, nev, b, probs[b][1], ("permutation", seed))
            assert first.setdefault(n, outputs(orders, ev, nev, b)) == outputs(orders, ev, nev, b), (seed, n)
    j = order.index(64)
    L = Layout([p[0] for p in probs] + [probs[j][0]], nan_below=4)   # a copy of problem j at the end ...
    L.add_shared(j)                                                   # ... and its own storage once more
    orders, ev, nev, st = drv.orders(L, events=True)
    B = len(order)
    assert outputs(orders, ev, nev, j) == outputs(orders, ev, nev, B) == outputs(orders, ev, nev, B + 1) == first[64]
    assert st.n_lds == int((L.ns >= 4).sum())


def dense_layout(D):
    L = Layout([])
    B, n = D.shape[0], D.shape[1]
    L.buf = np.ascontiguousarray(D).reshape(-1)
    L.offsets = np.arange(B, dtype=np.int64) * n * n
    L.ns = np.full(B, n, dtype=np.int32)
    L.lds = None
    return L


def check_equal_sizes(drv, same_orders, same_weights):
    """Case 3: a same-size batch through the ragged calls gives the bytes of the same-size calls.  same_orders(D) -> (orders,
    events, nevents); same_weights(D, orders) -> weights, on the kernel route."""
    for n in (24, 65):
        D, refs = bc.dec4_batch(n, 6, seed0=300)
        o0, e0, n0 = same_orders(D)
        orders, ev, nev, st = drv.orders(dense_layout(D), events=True)
        assert np.stack(orders).tobytes() == o0.tobytes() and np.stack(ev).tobytes() == e0.tobytes() and (nev == n0).all()
        assert st.chunks == 1 and st.n_lds == 6
    for n in (12, 33):
        D, so = sc.synth_batch(n, 4)
        w, sw, st = drv.weights(dense_layout(D), list(so))
        assert np.stack(w).tobytes() == same_weights(D, so).tobytes()
        assert st.chunks == 1 and st.n_kernel + st.n_closed_form == 4


def check_chunking(drv, monkeypatch):
    """Case 4: three problems per chunk give the bytes of one chunk, in more launches."""
    mats, refs = mixed((5, 9, 16, 33, 65, 8, 7, 2, 64, 12))
    L = Layout(mats, nan_below=2)
    ord_of = [r[0] for r in refs]
    o1, e1, n1, s1 = drv.orders(L, events=True)
    w1, _, t1 = drv.weights(L, ord_of)
    monkeypatch.setenv("FNN_BATCH_CHUNK", "3")
    o2, e2, n2, s2 = drv.orders(L, events=True)
    w2, sw2, t2 = drv.weights(L, ord_of)
    monkeypatch.delenv("FNN_BATCH_CHUNK")
    assert s2.chunks > s1.chunks and t2.chunks > t1.chunks
    for b, ref in enumerate(refs):
        assert outputs(o1, e1, n1, b) == outputs(o2, e2, n2, b), b
        assert w1[b].tobytes() == w2[b].tobytes(), b
        assert_problem(o2, e2, n2, b, ref, "chunked")
    assert (sw2["certified"] == 1).all()


def check_validation(drv):
    """Case 5: the failing problem is named in the caller's numbering, and nothing is written."""
    sizes = (16, 5, 33, 9, 64, 6, 7, 65, 20, 8, 4, 97, 10)       # index 11 is larger than index 5: a sort by size meets it first
    mats = [problem(n, k)[0].copy() for k, n in enumerate(sizes)]
    for what in ("asymmetric", "nan", "diagonal"):
        bad = [m.copy() for m in mats]
        for b in (5, 11):
            if what == "asymmetric":
                bad[b][2, 3] += 0.5
            elif what == "nan":
                bad[b][2, 3] = bad[b][3, 2] = np.nan
            else:
                bad[b][1, 1] = 1e-3
        try:
            drv.orders(Layout(bad), validate=True, fill=SENTINEL)
        except _capi.FnnError as e:
            assert e.code == -1 and "problem 5:" in str(e), e
            assert (e.orders == SENTINEL).all()
        else:
            raise AssertionError(f"{what}: the call did not fail")
    L = Layout(mats)
    good, _, _, _ = drv.orders(L, validate=True)
    for b, n in enumerate(sizes):
        assert (good[b] == problem(n, b)[1][0]).all()
    for field, value in (("lds", lambda n: n - 1), ("ns", lambda n: -1)):
        L2 = Layout(mats)
        getattr(L2, field)[7] = value(sizes[7])
        try:
            drv.orders(L2, fill=SENTINEL)
        except _capi.FnnError as e:
            assert e.code == -1 and "problem 7" in str(e) and (e.orders == SENTINEL).all(), e
        else:
            raise AssertionError(f"{field}: the call did not fail")
    L0 = Layout([])
    orders, _, nev, st = drv.orders(L0)                             # batch == 0 is FNN_OK
    assert orders == [] and st.n_problems == 0
    tiny = Layout([np.full((n, n), np.nan) for n in (3, 1, 2, 0, 3)])
    orders, ev, nev, st = drv.orders(tiny, events=True)
    for b, n in enumerate((3, 1, 2, 0, 3)):
        assert (orders[b] == np.arange(n + 1)).all() and nev[b] == 0
    assert st.chunks == 0 and st.n_lds == 0 and st.t_kernel_s == 0 and st.n_problems == 5


def check_weights(drv, max_n, same_weights):
    """Case 6: the mixed batch of case 1 from 2 taxa on, with the oracle's orders.  same_weights(D, orders) -> weights of the
    same-size kernel route."""
    mats, refs = mixed(mixed_sizes(max_n, low=2))
    L = Layout(mats)
    ord_of = [r[0] for r in refs]
    w, sw, st = drv.weights(L, ord_of)
    assert st.n_problems == len(mats) and st.n_fallback == 0 and st.n_kernel + st.n_closed_form == len(mats), st.as_dict()
    assert 2 <= st.chunks <= 8 and st.block_threads == 1024 and 0 < st.lds_bytes <= 65536 and st.capacity == 6 * max_n
    for b, (D, o) in enumerate(zip(mats, ord_of)):
        n = D.shape[0]
        sc.assert_optimal(D[None], o[None], w[b][None], sw[b: b + 1], ("mixed", b, n))
        if n <= 33:
            import scipy.optimize as so
            xs = so.nnls(sc.W.live_design_matrix(n, o), sc.W.packed_distances(D), maxiter=10 ** 7)[0]
            assert np.abs(w[b] - xs).max() <= 1e-6 * max(1.0, np.abs(xs).max()), (n, b, np.abs(w[b] - xs).max())
        assert w[b].tobytes() == same_weights(D[None], o[None]).tobytes(), (b, n)
    return w


def emu_weight_giveups(a, mats, orders):
    """FNN_SW_GIVEUP_* per problem from the CPU driver's ragged weight call, whether it fails (a problem gave up) or not."""
    try:
        Driver(a).weights(Layout(mats), orders, fill=sc.SENTINEL)
    except _capi.FnnError as e:
        assert e.code == -6 and (e.weights == sc.SENTINEL).all(), e
        failed = str(e)
    else:
        failed = None
    g = np.zeros(len(mats), dtype=np.int32)
    assert a.split_weights_ragged_giveups(g.ctypes.data_as(C.POINTER(C.c_int32)), len(mats)) == len(mats)
    assert (failed is None) == (not g.any()) and (failed is None or f"problem {int(np.flatnonzero(g)[0])}:" in failed), (failed, g)
    return g


def check_safety_net(drv, emu, same_solve, single, monkeypatch):
    """The set-aside case of tests/splits_batch_common.py in one mixed call: FNN_SW_BATCH_DEP=0.02 reaches every workgroup of a
    ragged launch as it reaches the same-size kernel.  Per problem: the same give-up as the same-size route, its bytes and
    counters when it is solved, the certificate, scipy up to 33 taxa.  emu: the CPU driver's library (it says which problems
    give up); same_solve: splits_batch_common's solve of the same-size route; single: the one-problem solver on the GPU, None
    on the CPU, where the driver solves the problems that do not give up in a call of their own."""
    mats, refs = mixed((5, 9, 33, 65, 8, 97, 64, 12), seed=None)
    ord_of = [r[0] for r in refs]
    # none of these eight is set aside AND certified (they certify untouched or give up); two of splits_batch_common's list that
    # certify through set-aside, release and recheck join them, so that the counters of a ragged launch are seen to count
    for n, pair in ((64, ("outgroup", 4)), (65, ("outgroup", 5))):
        D, o = sc.class_batch(n, (pair,))
        mats.append(D[0])
        ord_of.append(o[0])
    monkeypatch.setenv("FNN_SW_BATCH_DEP", "0.02")
    g = emu_weight_giveups(emu, mats, ord_of)
    print("ragged set-aside: give-ups", g.tolist())
    assert set(g.tolist()) == {0, sc.GIVEUP_NUMERIC} and (g == 0).sum() >= 5, g     # both populations
    keep = [b for b in range(len(mats)) if single is not None or g[b] == 0]
    w, sw, st = drv.weights(Layout([mats[b] for b in keep]), [ord_of[b] for b in keep])
    assert st.n_fallback == (0 if single is None else int((g != 0).sum())), (st.as_dict(), g)
    total = dict.fromkeys(sc.COUNTERS, 0)
    for k, b in enumerate(keep):
        D, o, n = mats[b], ord_of[b], mats[b].shape[0]
        w1, sw1, g1, _ = same_solve(D[None], o[None])
        assert g1[0] == g[b], (b, n, g1, g)
        if g[b]:
            assert w[k].tobytes() == single(D, o).tobytes(), (b, n)
        else:
            assert w[k].tobytes() == w1[0].tobytes(), (b, n)
            for c in sc.COUNTERS:
                assert sw[c][k] == sw1[c][0], (b, n, c)
                total[c] += int(sw[c][k])
        xs = None
        if n <= 33:
            import scipy.optimize as so
            xs = so.nnls(sc.W.live_design_matrix(n, o), sc.W.packed_distances(D), maxiter=10 ** 7)[0]
        sc.assert_solved(D[None], o[None], w[k][None], sw[k: k + 1], 0, ("ragged set-aside", b, n), xs)
    monkeypatch.delenv("FNN_SW_BATCH_DEP")
    print("ragged set-aside: counters of the certified", total)
    assert total["aside_fresh"] > 0 and total["rechecks"] > 0 and total["releases"] > 0, total
    return total

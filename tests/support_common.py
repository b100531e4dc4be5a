"""Shared by tests/test_support_emu.py (CPU driver of the per-thread steps) and tests/test_support.py (the product on the GPU):
the reference of the split-support stage - plain Python: keys as Python integers built from the
definition, a dict in order of first appearance, sums as a for loop over ascending b; nothing from the product - and the
cases of both suites.  Every comparison is bytewise; no tolerance exists or is needed."""
import contextlib
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from fastneighbornet_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "fastneighbornet_amd", "csrc")
EMU_SRCS = [os.path.join(EMU_DIR, "fnn_support_emu.cpp")] + \
    [os.path.join(CSRC, f) for f in ("fnn_support.h", "fnn_small.h", "fnn_engine.h", "fnn_core.h", "fnn_small_splits.h")] + \
    [os.path.join(ROOT, "include", "fastnn.h"), os.path.join(EMU_DIR, "fnn_small_emu.h")]
FILL = 0xA5          # every byte of the output arrays before a call
SWITCHES = ("FNN_SUPPORT_ROUTE", "FNN_SUPPORT_HASH_BITS", "FNN_BATCH_CHUNK")


def newer(out, srcs):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(s) for s in srcs)


def emu_support_api():
    """tests/emu/fnn_support_emu.cpp as a shared library, behind the same ctypes view as the product."""
    out = os.path.join(EMU_DIR, "build", "libfnn_support_emu.so")
    if newer(out, EMU_SRCS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                               "-o", out, EMU_SRCS[0]])
    lib = C.CDLL(out)
    a = _capi.bind_support(_capi.Api(lib, "emu_", engine=False))
    lib.emu_support_set_reverse.argtypes = [C.c_int32]
    lib.emu_support_set_reverse.restype = None
    a.set_reverse = lib.emu_support_set_reverse
    return a


@contextlib.contextmanager
def switches(**kw):
    """The test switches of the call (route=, hash_bits=, chunk=) in the environment, the earlier state restored."""
    names = {"route": "FNN_SUPPORT_ROUTE", "hash_bits": "FNN_SUPPORT_HASH_BITS", "chunk": "FNN_BATCH_CHUNK"}
    old = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    for k, v in kw.items():
        if v is not None:
            os.environ[names[k]] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


# ---- the reference ----------------------------------------------------------------------------------------------

def pairs(n):
    return [(i, j) for i in range(n - 1) for j in range(i + 1, n)]


def k_of(n, i, j):
    return i * (2 * n - i - 1) // 2 + (j - i - 1)


def ref_key(order, n, i, j):
    """The split of positions i + 1 ... j of `order` as an integer: bit t - 1 for taxon t, on the side without taxon 1."""
    bits = 0
    for t in order[i + 1:j + 1]:
        bits |= 1 << (int(t) - 1)
    if bits & 1:
        bits ^= (1 << n) - 1
    return bits


def key_words(key, n):
    return [(key >> (64 * w)) & ((1 << 64) - 1) for w in range((n + 63) // 64)]


def ref_table(orders, W, threshold, lead):
    """dict key -> [first_b, first_k, count, weight_sum] in order of first appearance."""
    orders, W = np.asarray(orders), np.asarray(W, dtype=np.float64)
    B, n = orders.shape[0], orders.shape[1] - 1
    pr = pairs(n)
    rows = {}
    for b in range(B):
        order = [int(x) for x in orders[b]]
        for k in np.nonzero(W[b] > threshold)[0].tolist():   # (IEEE: a NaN is not above anything)
            i, j = pr[k]
            key = ref_key(order, n, i, j)
            if key not in rows:
                rows[key] = [b, k, 0, 0.0]
            if b >= lead:
                rows[key][2] += 1
                rows[key][3] = rows[key][3] + float(W[b, k])
    return rows


def ref_arrays(rows, n):
    words = (n + 63) // 64
    S = len(rows)
    keys = np.array([key_words(k, n) for k in rows], dtype=np.uint64).reshape(S, words)
    v = list(rows.values())
    return {"keys": keys, "first_b": np.array([r[0] for r in v], dtype=np.int64), "first_k": np.array([r[1] for r in v], dtype=np.int64),
            "count": np.array([r[2] for r in v], dtype=np.int64), "weight_sum": np.array([r[3] for r in v], dtype=np.float64)}


# ---- inputs -------------------------------------------------------------------------------------------------------

def order_row(perm):
    return np.concatenate([[0], perm]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def random_case(n, B, seed, per=3):
    """Orderings drawn from two base permutations and their rotations and reflections - the same split system at other (i, j)
    and on the complemented side -, each problem holding about per * n of its base's pool of 4 n arcs with positive weights;
    a few entries at or below zero and below the threshold 1e-6 in between."""
    r = np.random.default_rng(seed)
    K = n * (n - 1) // 2
    bases = [r.permutation(n) + 1 for _ in range(2)]
    pools = [[(int(r.integers(0, n)), int(r.integers(1, n))) for _ in range(4 * n)] for _ in range(2)]
    orders = np.zeros((B, n + 1), dtype=np.int32)
    W = np.zeros((B, K), dtype=np.float64)
    for b in range(B):
        g = int(r.integers(0, 2))
        c = bases[g]
        o = np.roll(c, int(r.integers(0, n)))
        if r.integers(0, 2):
            o = o[::-1]
        orders[b] = order_row(o)
        pos = np.zeros(n + 1, dtype=np.int64)
        pos[o] = np.arange(1, n + 1)
        junk = r.integers(0, K, max(n // 2, 1))
        W[b, junk] = r.choice([0.0, -1.0, 1e-7, 1e-6], len(junk))
        for s, ln in pools[g]:
            if r.random() >= per / 4.0:
                continue
            p = pos[c[(s + np.arange(ln)) % n]]
            lo, hi = int(p.min()), int(p.max())
            if hi == n or hi - lo + 1 != ln:      # the arc holds position n (or wraps): its complement is the interval
                inside = np.ones(n + 1, dtype=bool)
                inside[p] = False
                q = np.nonzero(inside[1:])[0] + 1
                lo, hi = int(q.min()), int(q.max())
                assert hi < n and hi - lo + 1 == n - ln
            W[b, k_of(n, lo - 1, hi)] = 0.01 + r.random()
    orders.setflags(write=False)
    W.setflags(write=False)
    return orders, W


@functools.lru_cache(maxsize=None)
def random_ref(n, B, seed, threshold=1e-6, lead=0):
    orders, W = random_case(n, B, seed)
    rows = ref_table(orders, W, threshold, lead)
    out = ref_arrays(rows, n)
    for v in out.values():
        v.setflags(write=False)
    return out


# ---- one call -----------------------------------------------------------------------------------------------------

def call(a, orders, W, threshold=1e-6, lead=0, capacity=None, in_place=False, extra=3):
    """One call through the raw entry with the output arrays filled with FILL bytes.  capacity None: a first call with
    capacity 0 for S, then S + extra rows.  Returns (table cut to the filled rows, S, stats, the whole arrays).  in_place:
    the device entry (True: the CPU driver's, which reads host memory in place; "torch": the weights as a tensor on the GPU)."""
    orders = np.ascontiguousarray(orders, dtype=np.int32)
    W = np.ascontiguousarray(W, dtype=np.float64)
    B, n = orders.shape[0], orders.shape[1] - 1
    keep = None
    if in_place == "torch":
        import torch
        keep = torch.from_numpy(W).to("cuda:0")
        torch.cuda.synchronize()
        wp = keep.data_ptr()
    else:
        wp = W.ctypes.data
    dev = bool(in_place)
    if capacity is None:
        _, S0, _ = _capi.run_support(a, n, B, orders.ctypes.data, wp, threshold, lead, 0, on_device=dev, fill=FILL)
        capacity = S0 + extra
    whole, S, st = _capi.run_support(a, n, B, orders.ctypes.data, wp, threshold, lead, capacity, on_device=dev, fill=FILL)
    del keep
    return {k: v[:min(S, capacity)] for k, v in whole.items()}, S, st, whole


def assert_untouched(whole, rows):
    """Everything behind the first `rows` rows still holds the FILL bytes."""
    for k, v in whole.items():
        assert (np.ascontiguousarray(v[rows:]).view(np.uint8) == FILL).all(), k


def assert_table(got, S, ref):
    assert S == len(ref["first_b"])
    for k in ("keys", "first_b", "first_k", "count", "weight_sum"):
        assert got[k].shape == ref[k].shape, k
        assert got[k].tobytes() == ref[k].tobytes(), k


def check_against(a, orders, W, ref, threshold=1e-6, lead=0, in_place=False, **sw):
    with switches(**sw):
        got, S, st, whole = call(a, orders, W, threshold, lead, in_place=in_place)
    assert_table(got, S, ref)
    assert_untouched(whole, S)
    assert st.n_splits == S and st.n_problems == orders.shape[0] and st.words == (orders.shape[1] + 62) // 64
    assert st.n_records == int((np.asarray(W) > threshold).sum())
    if sw.get("route") and not sw.get("hash_bits"):
        assert _capi.SUPPORT_ROUTES[st.route] == sw["route"]
    return st


# ---- the cases of both suites; `a` is the bound library -----------------------------------------------------------

WORD_EDGES = [(n, B) for n in (2, 3, 5, 63, 64, 65, 128, 129, 140, 141) for B in (1, 2, 17)] + [(1024, 3)]


def check_word_edge(a, n, B):
    orders, W = random_case(n, B, 1000 + n)
    ref = random_ref(n, B, 1000 + n)
    if n >= 63:
        assert 2 * n <= (W > 1e-6).sum(axis=1).min() and (W > 1e-6).sum(axis=1).max() <= 4 * n   # about 3 n counting records each
    st = check_against(a, orders, W, ref, route="kernel")
    if len(ref["first_b"]):
        assert st.table_slots >= 2 * st.n_records and st.hash_retries == 0 and st.chunks == 1
    check_against(a, orders, W, ref, route="host")


def check_fold(a):
    n = 6
    K = n * (n - 1) // 2
    # {2, 3} | {1, 4, 5, 6}: in problem 0 as positions 2 ... 3 (without taxon 1), in problem 1 as positions 1 ... 4 = {4, 5, 6, 1}
    orders = np.array([order_row([1, 2, 3, 4, 5, 6]), order_row([4, 5, 6, 1, 2, 3])])
    W = np.zeros((2, K))
    W[0, k_of(n, 1, 3)] = 0.5
    W[1, k_of(n, 0, 4)] = 0.25
    for route in ("kernel", "host"):
        with switches(route=route):
            got, S, _, _ = call(a, orders, W)
        assert S == 1 and got["keys"].tolist() == [[0b000110]] and got["count"].tolist() == [2]
        assert got["weight_sum"].tolist() == [0.75] and (got["first_b"][0], got["first_k"][0]) == (0, k_of(n, 1, 3))
    # {2, 3} and {2, 3, 4}: the sets differ in one bit, the splits are two
    W2 = np.zeros((1, K))
    W2[0, k_of(n, 1, 3)] = 0.5
    W2[0, k_of(n, 1, 4)] = 0.5
    for route in ("kernel", "host"):
        with switches(route=route):
            got, S, _, _ = call(a, orders[:1], W2)
        assert S == 2 and got["keys"].tolist() == [[0b000110], [0b001110]] and got["count"].tolist() == [1, 1]
    assert_table(*call(a, orders, W)[:2], ref_arrays(ref_table(orders, W, 1e-6, 0), n))


def check_sum_order(a):
    n, B = 5, 4
    orders = np.array([order_row([1, 2, 3, 4, 5])] * B)
    k = k_of(n, 1, 3)
    sums = []
    for ws in ((1e16, 1.0, 1.0, 1.0), (1.0, 1.0, 1.0, 1e16)):
        W = np.zeros((B, n * (n - 1) // 2))
        W[:, k] = ws
        ref = ref_arrays(ref_table(orders, W, 1e-6, 0), n)
        seq = 0.0
        for x in ws:
            seq = seq + x
        assert ref["weight_sum"].tolist() == [seq]
        sums.append(seq)
        for sw in (dict(route="kernel"), dict(route="host"), dict(route="kernel", chunk=3), dict(route="kernel", chunk=1)):
            st = check_against(a, orders, W, ref, **sw)
            if "chunk" in sw:
                assert st.chunks == (2 if sw["chunk"] == 3 else 4)
    assert sums[0] != sums[1]    # the two orders differ in fp64: a sum in any other order would show


LEADS = (0, 1, 2, 5)
LEAD_N = 16


def lead_case():
    return random_case(LEAD_N, 5, 77)


def check_lead(a, lead):
    orders, W = lead_case()
    n = LEAD_N
    ref = ref_arrays(ref_table(orders, W, 1e-6, lead), n)
    for route in ("kernel", "host"):
        check_against(a, orders, W, ref, lead=lead, route=route)
    # rows of problem 0 come first, in ascending k
    k0 = np.nonzero(W[0] > 1e-6)[0]
    assert (ref["first_b"][:len(k0)] == 0).all() and (ref["first_k"][:len(k0)] == k0).all() and (ref["first_b"][len(k0):] > 0).all()
    if lead:
        assert (ref["count"] == 0).any() and (ref["first_b"][ref["count"] == 0] < lead).all()   # splits that only lead problems hold
        zero = ref["weight_sum"][ref["count"] == 0]
        assert zero.tobytes() == np.zeros(len(zero)).tobytes()    # +0.0
    if lead == 5:
        assert (ref["count"] == 0).all()


def check_threshold(a):
    n, B = 5, 2
    K = n * (n - 1) // 2
    orders = np.array([order_row([1, 2, 3, 4, 5]), order_row([3, 4, 5, 1, 2])])
    thr = 0.25
    W = np.zeros((B, K))
    W[0, :6] = [thr, np.nextafter(thr, 1.0), 0.0, -1.0, np.nan, 0.75]
    W[1, :6] = [np.nan, thr, np.nextafter(thr, 0.0), 2.0, np.inf, -np.inf]
    ref = ref_arrays(ref_table(orders, W, thr, 0), n)
    assert len(ref["first_b"]) >= 3 and int(ref["count"].sum()) == 4
    W0 = np.zeros((B, K))
    W0[0, :4] = [0.0, -0.0, 5e-324, -5e-324]
    W0[1, :3] = [np.nan, 1.0, 0.0]
    ref0 = ref_arrays(ref_table(orders, W0, 0.0, 0), n)
    assert int(ref0["count"].sum()) == 2
    for route in ("kernel", "host"):
        check_against(a, orders, W, ref, threshold=thr, route=route)
        check_against(a, orders, W0, ref0, threshold=0.0, route=route)
        with switches(route=route):
            got, S, st, whole = call(a, orders, np.full((B, K), 1e-6))   # all at the threshold: nothing counts
        assert S == 0 and st.n_records == 0 and st.n_splits == 0
        assert_untouched(whole, 0)


def check_capacity(a, in_place=False):
    orders, W = random_case(65, 2, 1065)
    ref = random_ref(65, 2, 1065)
    S = len(ref["first_b"])
    for route in ("kernel", "host"):
        for cap in (0, S - 1, S, S + 1):
            with switches(route=route):
                got, S_got, _, whole = call(a, orders, W, capacity=cap, in_place=in_place)
            rows = min(S, cap)
            assert S_got == S
            assert_table(got, rows, {k: v[:rows] for k, v in ref.items()})
            assert_untouched(whole, rows)


def chunk_case():
    """B = 7 in chunks of 3, rotations and reflections of one circular order: split X in every problem, split Y first in
    problem 4 (chunk 2) and again in problem 6 (chunk 3), around eight random splits per problem."""
    n, B = 8, 7
    r = np.random.default_rng(88)
    c = r.permutation(n) + 1
    pr = pairs(n)
    orders = np.zeros((B, n + 1), dtype=np.int32)
    W = np.zeros((B, len(pr)))
    for b in range(B):
        o = np.roll(c, int(r.integers(0, n)))
        orders[b] = order_row(o[::-1] if b % 2 else o)
        W[b, r.integers(0, len(pr), 8)] = 0.01 + r.random(8)

    def where(b, key):   # the index k at which problem b holds the split `key`
        return next(k for k in range(len(pr)) if ref_key(orders[b].tolist(), n, *pr[k]) == key)

    xkey = ref_key(orders[0].tolist(), n, *pr[5])
    for b in range(B):
        W[b, where(b, xkey)] = 1.0 + b / 8.0
    held = ref_table(orders, W, 1e-6, 0)
    free = next(k for k in range(len(pr)) if ref_key(orders[4].tolist(), n, *pr[k]) not in held)   # a split that no problem holds yet
    ykey = ref_key(orders[4].tolist(), n, *pr[free])
    W[4, free] = 0.375
    W[6, where(6, ykey)] = 0.5
    return orders, W, xkey, ykey


def check_chunking(a, in_place=False):
    orders, W, xkey, ykey = chunk_case()
    rows = ref_table(orders, W, 1e-6, 0)
    assert rows[ykey][:3] == [4, rows[ykey][1], 2] and rows[xkey][0] == 0 and rows[xkey][2] == 7
    ref = ref_arrays(rows, 8)
    st = check_against(a, orders, W, ref, in_place=in_place, route="kernel", chunk=3)
    assert st.chunks == 3
    assert check_against(a, orders, W, ref, in_place=in_place, route="kernel").chunks == 1
    check_against(a, orders, W, ref, in_place=in_place, route="host", chunk=3)
    rows1 = ref_table(orders, W, 1e-6, 1)
    check_against(a, orders, W, ref_arrays(rows1, 8), lead=1, in_place=in_place, route="kernel", chunk=2)


def check_routes(a):
    orders, W = random_case(65, 17, 1065)
    ref = random_ref(65, 17, 1065)
    st_k = check_against(a, orders, W, ref, route="kernel")
    st_h = check_against(a, orders, W, ref, route="host")
    assert (st_k.route, st_h.route) == (0, 1) and st_h.hash_retries == 0 and st_h.table_slots == 0
    st = check_against(a, orders, W, ref, route="kernel", hash_bits=3)     # 8 hashes for hundreds of keys: every seed collides
    assert st.hash_retries == 3 and st.route == 1
    st = check_against(a, orders, W, ref, route="kernel", hash_bits=64)
    assert st.hash_retries == 0 and st.route == 0
    # the default route follows the crossover in batch * n * n
    with switches():
        small = call(a, *random_case(5, 2, 1005))[2]
        assert small.route == 1 and 2 * 5 * 5 < a.split_support_min_work()


def sparse_case():
    """n = 140, three problems: every split of one, two or three neighbouring taxa of the identity order, of a reflection and
    of an order that puts taxa 64, 96 and 128 side by side.  Keys of a few bits in different words are what a weak word-by-word
    hash lets cancel: {64, 96} against {128} is bit 63 of word 0 with bit 31 of word 1 against bit 63 of word 1."""
    n = 140
    rest = [t for t in range(2, n + 1) if t not in (64, 96, 128)]
    orders = np.array([order_row(np.arange(1, n + 1)), order_row(np.arange(n, 0, -1)), order_row([1, 64, 96, 128] + rest)])
    W = np.zeros((3, n * (n - 1) // 2))
    for b in range(3):
        for i in range(n - 1):
            for j in range(i + 1, min(i + 4, n)):
                W[b, k_of(n, i, j)] = 1.0 + (i + j + b) / 1024.0
    return orders, W


def check_sparse_keys(a):
    orders, W = sparse_case()
    rows = ref_table(orders, W, 1e-6, 0)
    assert (1 << 63 | 1 << 95) in rows and (1 << 127) in rows
    st = check_against(a, orders, W, ref_arrays(rows, 140), route="kernel")
    assert st.hash_retries == 0 and st.route == 0


def check_keys(a):
    for n in (2, 64, 65, 1024):
        r = np.random.default_rng(n)
        order = order_row(r.permutation(n) + 1)
        K = n * (n - 1) // 2
        ks = sorted({0, K - 1, K // 2} | set(r.integers(0, K, 20).tolist()))
        pr = pairs(n)
        got = _capi.run_split_keys(a, n, order, ks)
        want = np.array([key_words(ref_key(order.tolist(), n, *pr[k]), n) for k in ks], dtype=np.uint64)
        assert got.tobytes() == want.tobytes(), n
    order = order_row([2, 1, 3])
    bad = order_row([2, 2, 3])
    k = np.zeros(1, dtype=np.int64)
    out = np.zeros(1, dtype=np.uint64)
    assert a.split_keys(3, order.ctypes.data, k.ctypes.data, 0, None) == 0
    for args in ((1, order.ctypes.data, k.ctypes.data, 1, out.ctypes.data), (3, None, k.ctypes.data, 1, out.ctypes.data),
                 (3, order.ctypes.data, None, 1, out.ctypes.data), (3, order.ctypes.data, k.ctypes.data, 1, None),
                 (3, order.ctypes.data, k.ctypes.data, -1, out.ctypes.data), (3, bad.ctypes.data, k.ctypes.data, 1, out.ctypes.data)):
        assert a.split_keys(*args) == -1 and a.last_error()
    k[0] = 3
    assert a.split_keys(3, order.ctypes.data, k.ctypes.data, 1, out.ctypes.data) == -1


def check_arguments(a):
    """Argument checks come before any device use: they hold without a GPU, on either route."""
    n, B = 6, 4
    orders, W = (np.array(x) for x in random_case(n, B, 1234))
    S = C.c_int64(-5)
    cap = 64
    out = {k: np.full(cap * 8, FILL, dtype=np.uint8) for k in ("keys", "first_b", "first_k", "count", "weight_sum")}
    good = dict(n=n, batch=B, orders=orders.ctypes.data, W=W.ctypes.data, thr=1e-6, lead=0, cap=cap, S=C.addressof(S),
                **{k: v.ctypes.data for k, v in out.items()})

    def rc(in_place=False, **kw):
        k = dict(good, **kw)
        fn = a.split_support_device_f64 if in_place else a.split_support_f64
        return fn(k["n"], k["batch"], k["orders"], k["W"], k["thr"], k["lead"], 0, k["keys"], k["first_b"], k["first_k"], k["count"],
                  k["weight_sum"], k["cap"], k["S"], None)

    bad2 = orders.copy()
    bad2[1, 3] = bad2[1, 4]
    bad2[3, 1] = n + 1
    for route in ("kernel", "host", None):
        with switches(route=route):
            for in_place in (False, True):
                for bad in (dict(orders=None), dict(W=None), dict(S=None), dict(keys=None), dict(first_b=None), dict(first_k=None),
                            dict(count=None), dict(weight_sum=None), dict(n=1), dict(n=0), dict(n=-4), dict(batch=-1), dict(lead=-1),
                            dict(lead=B + 1), dict(thr=float("nan")), dict(cap=-1), dict(n=a.split_support_max_n() + 1)):
                    assert rc(in_place, **bad) == -1, (in_place, bad)
                    assert a.last_error()
                assert rc(in_place, orders=bad2.ctypes.data) == -1
                assert b"problem 1:" in a.last_error(), a.last_error()
                assert S.value == -5
                assert rc(in_place, batch=0) == 0 and S.value == 0
                S.value = -5
                assert rc(in_place, batch=0, orders=None, W=None, cap=0, keys=None, first_b=None, first_k=None, count=None, weight_sum=None) == 0
                assert S.value == 0
                S.value = -5
    assert all((v == FILL).all() for v in out.values())
    assert a.split_support_max_n() == 1024

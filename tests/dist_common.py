"""Shared by tests/test_dist_emu.py (CPU driver of the per-lane steps) and tests/test_dist.py (the product on the GPU): the
reference of the alignment-distance path - plain numpy and Python integers, nothing from the product
- and the cases of both suites.  Matrices are compared bitwise; no tolerance exists or is needed."""
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
EMU_SRCS = [os.path.join(EMU_DIR, "fnn_dist_emu.cpp")] + [os.path.join(CSRC, f) for f in ("fnn_dist.h", "fnn_small.h", "fnn_engine.h", "fnn_core.h")] + \
    [os.path.join(ROOT, "include", "fastnn.h"), os.path.join(EMU_DIR, "fnn_small_emu.h"), os.path.join(CSRC, "fnn_small_splits.h")]
MISSING = 255
SENTINEL = -77.0
MASK64 = (1 << 64) - 1


def newer(out, srcs):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(s) for s in srcs)


def emu_dist_api():
    """tests/emu/fnn_dist_emu.cpp as a shared library, behind the same ctypes view as the product."""
    out = os.path.join(EMU_DIR, "build", "libfnn_dist_emu.so")
    if newer(out, EMU_SRCS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                               "-o", out, EMU_SRCS[0]])
    return _capi.bind_dist(_capi.Api(C.CDLL(out), "emu_", engine=False))


# ---- the reference ----------------------------------------------------------------------------------------------

def ref_sums(seq, counts):
    """(mism, valid): int64 (B, n, n), from the definition."""
    seq = np.asarray(seq, dtype=np.int64)
    present = seq != MISSING
    both = present[:, None, :] & present[None, :, :]
    diff = both & (seq[:, None, :] != seq[None, :, :])
    c = np.asarray(counts, dtype=np.int64)
    return np.einsum("ijs,bs->bij", diff.astype(np.int64), c), np.einsum("ijs,bs->bij", both.astype(np.int64), c)


def first_empty(valid):
    """The lowest (b, i, j), i < j, with valid == 0, or None."""
    B, n, _ = valid.shape
    bad = (valid == 0) & np.triu(np.ones((n, n), dtype=bool), 1)[None]
    idx = np.argwhere(bad)
    return tuple(int(x) for x in idx[0]) if len(idx) else None


def ref_dist(seq, counts):
    mism, valid = ref_sums(seq, counts)
    assert first_empty(valid) is None, "the case has a pair without a common site"
    n = mism.shape[1]
    eye = np.eye(n, dtype=bool)[None]
    D = mism.astype(np.float64) / np.where(eye, 1, valid).astype(np.float64)
    D[np.broadcast_to(eye, D.shape)] = 0.0
    return D


def splitmix64_at(seed, k):
    z = (seed + (k + 1) * 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def ref_bootstrap_counts(L, B, seed):
    out = np.zeros((B, L), dtype=np.int64)
    for b in range(B):
        for k in range(L):
            out[b, (splitmix64_at(seed & MASK64, b * L + k) * L) >> 64] += 1
    return out


def same_bits(a, b):
    return a.shape == b.shape and (np.ascontiguousarray(a).view(np.int64) == np.ascontiguousarray(b).view(np.int64)).all()


# ---- inputs -------------------------------------------------------------------------------------------------------

def random_seq(n, L, seed, missing=0.0):
    """4-state sequences at about 10 % divergence from a common ancestor; `missing`: the share of bytes 255."""
    r = np.random.default_rng(seed)
    base = r.integers(0, 4, L)
    seq = np.where(r.random((n, L)) < 0.1, r.integers(0, 4, (n, L)), base[None, :])
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[seq].copy()
    if missing:
        seq[r.random((n, L)) < missing] = MISSING
    return seq


def random_counts(B, L, seed, cmax=127):
    """counts in 1 ... cmax (so that no replicate is empty), the largest one equal to cmax."""
    c = np.random.default_rng(seed).integers(1, cmax + 1, (B, L)).astype(np.uint16)
    c[B // 2, L // 2] = cmax
    return c


# ---- one call -----------------------------------------------------------------------------------------------------

def call(a, seq, counts, lds=None, ldc=None, ld=None, stride=None, in_place=False, pad_seed=99):
    """One call through the raw entry on arrays laid out with the given strides: the inputs' padding holds values that would
    change the result if read, the output's padding holds SENTINEL.  Returns (D[B, n, n] view of the padded output, the whole
    padded output, stats).  in_place: the device entry (the CPU driver's writes host memory in place)."""
    seq, counts = np.asarray(seq, dtype=np.uint8), np.asarray(counts, dtype=np.uint16)
    (n, L), B = seq.shape, counts.shape[0]
    lds, ldc, ld = lds or L, ldc or L, ld or n
    stride = stride or n * ld
    r = np.random.default_rng(pad_seed)
    s_buf = np.frombuffer(b"ACGT\xff", dtype=np.uint8)[r.integers(0, 5, (n, lds))].copy()
    s_buf[:, :L] = seq
    c_buf = np.full((B, ldc), 999, dtype=np.uint16)
    c_buf[:, :L] = counts
    out = np.full(max(B * stride, 1), SENTINEL, dtype=np.float64)
    if in_place == "torch":   # the product's device entry: the output is a tensor on the GPU
        import torch
        t = torch.from_numpy(out).to("cuda:0")
        torch.cuda.synchronize()
        st = _capi.run_dist(a, s_buf.ctypes.data, n, L, lds, c_buf.ctypes.data, B, ldc, t.data_ptr(), ld, stride, on_device=True)
        out = t.cpu().numpy()
    else:
        try:
            st = _capi.run_dist(a, s_buf.ctypes.data, n, L, lds, c_buf.ctypes.data, B, ldc, out.ctypes.data, ld, stride, on_device=bool(in_place))
        except _capi.FnnError as e:
            e.out = out
            raise
    view = np.lib.stride_tricks.as_strided(out, (B, n, n), (8 * stride, 8 * ld, 8)) if B else np.zeros((0, n, n))
    return view, out, st


def assert_padding_untouched(out, B, n, ld, stride):
    mask = np.ones(out.shape, dtype=bool)
    for b in range(B):
        for i in range(n):
            mask[b * stride + i * ld: b * stride + i * ld + n] = False
    assert (out[mask] == SENTINEL).all()


# ---- the cases of both suites; `a` is the bound library -----------------------------------------------------------

LANE_MAP_SITES = {"site j": (0, 1, 2, 3, 4, 5), "all lane groups": (3, 17, 30, 47, 52, 63)}


def first_primes(k):
    out, x = [], 2
    while len(out) < k:
        if all(x % p for p in out if p * p <= x):
            out.append(x)
        x += 1
    return out


def check_lane_maps(a, where):
    """n = 6, L = 64, B = 16: all sequences equal except that taxon j differs from all others at one site of its own;
    counts[b][s] distinct primes.  Every entry of every replicate is then one predicted sum: a swapped row / column, a wrong
    k-order inside a fragment or a wrong replicate column changes some entry."""
    n, L, B = 6, 64, 16
    sites = LANE_MAP_SITES[where]
    seq = np.full((n, L), ord("A"), dtype=np.uint8)
    for j in range(n):
        seq[j, sites[j]] = ord("C")
    counts = np.array(first_primes(B * L), dtype=np.uint16).reshape(L, B).T.copy()   # (asymmetric in b and s)
    assert len(set(counts.ravel().tolist())) == B * L
    D, _, st = call(a, seq, counts)
    tot = counts.astype(np.int64).sum(axis=1)
    for b in range(B):
        for i in range(n):
            for j in range(n):
                want = 0.0 if i == j else float(int(counts[b, sites[i]]) + int(counts[b, sites[j]])) / float(tot[b])
                assert D[b, i, j] == want, (b, i, j, D[b, i, j], want)
    assert same_bits(D, ref_dist(seq, counts))
    assert st.digit_passes == 2 and st.has_missing == 0 and st.n_pairs == 15 and st.n_sites == L and st.n_problems == B


# every n of {1, 2, 3, 5, 6, 7, 17, 33, 65}, every L of {1, 15, 16, 17, 63, 64, 65, 130}, every B of {1, 15, 16, 17, 33}
SHAPES = [(1, 1, 1), (2, 15, 15), (3, 16, 16), (5, 17, 17), (6, 63, 33), (7, 64, 1), (17, 65, 15), (33, 130, 16), (65, 1, 17),
          (1, 130, 33), (2, 64, 17), (3, 65, 1), (5, 63, 16), (6, 16, 15), (7, 17, 33), (17, 15, 1), (33, 1, 15), (65, 130, 33),
          (17, 130, 17), (65, 63, 16)]


def shape_case(k):
    n, L, B = SHAPES[k]
    seq = random_seq(n, L, 500 + k, missing=0.1 if (k % 2 and L >= 63) else 0.0)   # (every other long case: the counting kernel)
    return seq, random_counts(B, L, 600 + k)


def check_shape(a, k):
    seq, counts = shape_case(k)
    D, _, st = call(a, seq, counts)
    assert same_bits(D, ref_dist(seq, counts))
    assert st.has_missing == int((seq == MISSING).any()) and st.digit_passes == 1 and st.block_threads == 256


DIGIT_CASES = [(1, 1), (127, 1), (128, 2), (16383, 2), (16384, 3), (65535, 3)]


def check_digits(a, cmax, passes, missing):
    n, L, B = 7, 65, 17
    seq = random_seq(n, L, 700, missing=0.1 if missing else 0.0)
    counts = random_counts(B, L, 701 + cmax, cmax)
    D, _, st = call(a, seq, counts)
    assert st.digit_passes == passes and int(counts.max()) == cmax
    assert same_bits(D, ref_dist(seq, counts))


def missing_case():
    seq = random_seq(9, 130, 800, missing=0.1)
    assert 0.05 < (seq == MISSING).mean() < 0.15
    return seq, random_counts(5, 130, 801)


def check_missing(a, monkeypatch):
    seq, counts = missing_case()
    D, _, st = call(a, seq, counts)
    assert st.has_missing == 1
    assert same_bits(D, ref_dist(seq, counts))
    # the same alignment without any 255 through the two kernel variants
    full = random_seq(9, 130, 800)
    D0, _, st0 = call(a, full, counts)
    monkeypatch.setenv("FNN_DIST_FORCE_MISSING", "1")
    D1, _, st1 = call(a, full, counts)
    monkeypatch.delenv("FNN_DIST_FORCE_MISSING")
    assert (st0.has_missing, st1.has_missing) == (0, 1)
    assert same_bits(D0, D1) and same_bits(D0, ref_dist(full, counts))
    # a site column that is missing in every taxon contributes nothing
    col = seq.copy()
    col[:, 7] = MISSING
    without = counts.copy()
    without[:, 7] = 0
    Dc, _, _ = call(a, col, counts)
    assert same_bits(Dc, call(a, col, without)[0]) and same_bits(Dc, ref_dist(col, counts))


def empty_pair_case(also_an_empty_replicate=False):
    """Taxa 2 and 5 share the sites 30 ... 39 only; the counts of replicate 3 are zero there."""
    seq = random_seq(9, 130, 810, missing=0.1)
    seq[2] = random_seq(1, 130, 811)[0]
    seq[5] = random_seq(1, 130, 812)[0]
    seq[2, 40:] = MISSING
    seq[5, :30] = MISSING
    counts = random_counts(6, 130, 813)
    counts[3, 30:40] = 0
    if also_an_empty_replicate:
        counts[4, :] = 0
    return seq, counts


def check_empty_pair(a, also_an_empty_replicate=False):
    seq, counts = empty_pair_case(also_an_empty_replicate)
    assert first_empty(ref_sums(seq, counts)[1]) == (3, 2, 5)
    if not also_an_empty_replicate:
        assert (ref_sums(seq, counts)[1] == 0).sum() == 2   # (that pair, both triangles, and nothing else)
    with pytest.raises(_capi.FnnError) as ei:
        call(a, seq, counts)
    assert ei.value.code == -1 and "(3, 2, 5)" in str(ei.value), str(ei.value)
    assert (ei.value.out == SENTINEL).all()   # the host output array still holds its sentinel
    # without missing bytes `valid` is the replicate's total: an empty replicate fails at its pair (0, 1)
    c2 = random_counts(4, 64, 814)
    c2[2, :] = 0
    with pytest.raises(_capi.FnnError) as ei:
        call(a, random_seq(5, 64, 815), c2)
    assert ei.value.code == -1 and "(2, 0, 1)" in str(ei.value), str(ei.value)
    assert (ei.value.out == SENTINEL).all()


def layout_case():
    return random_seq(7, 65, 820, missing=0.1), random_counts(7, 65, 821, 300)


def check_layout(a, in_place=False):
    seq, counts = layout_case()
    n, B = 7, 7
    ref = ref_dist(seq, counts)
    for lds, ldc, ld, stride in ((65 + 5, 65 + 3, n + 2, n * (n + 2) + 11), (65, 65 + 1, n, n * n + 1), (65 + 16, 65, n + 1, n * (n + 1))):
        D, out, _ = call(a, seq, counts, lds=lds, ldc=ldc, ld=ld, stride=stride, in_place=in_place)
        assert same_bits(D, ref), (lds, ldc, ld, stride)
        assert_padding_untouched(out, B, n, ld, stride)


def check_chunking(a, monkeypatch, in_place=False):
    seq, counts = layout_case()
    ref = ref_dist(seq, counts)
    monkeypatch.setenv("FNN_BATCH_CHUNK", "3")
    D, out, st = call(a, seq, counts, ld=9, stride=70, in_place=in_place)
    monkeypatch.delenv("FNN_BATCH_CHUNK")
    assert st.chunks == 3 and same_bits(D, ref)
    assert_padding_untouched(out, 7, 7, 9, 70)
    assert call(a, seq, counts)[2].chunks == 1


def check_arguments(a):
    """Argument checks come before any device use: they hold without a GPU."""
    n, L, B = 4, 10, 2
    seq, counts = random_seq(n, L, 830), random_counts(B, L, 831)
    out = np.full(B * n * n, SENTINEL)
    good = dict(seq=seq.ctypes.data, n=n, L=L, lds=L, counts=counts.ctypes.data, batch=B, ldc=L, out=out.ctypes.data, ld=n, stride=n * n, model=0)

    def rc(in_place=False, **kw):
        k = dict(good, **kw)
        fn = a.alignment_distances_batch_device_f64 if in_place else a.alignment_distances_batch_f64
        return fn(k["seq"], k["n"], k["L"], k["lds"], k["counts"], k["batch"], k["ldc"], k["model"], 0, k["out"], k["ld"], k["stride"], None)

    for in_place in (False, True):
        for bad in (dict(L=0), dict(L=-1), dict(n=0), dict(n=-3), dict(lds=L - 1), dict(ldc=L - 1), dict(ld=n - 1), dict(stride=n * n - 1),
                    dict(seq=None), dict(counts=None), dict(out=None), dict(model=1), dict(model=-1), dict(batch=-1),
                    dict(L=(2 ** 31 + 126) // 127, lds=2 ** 40, ldc=2 ** 40)):
            assert rc(in_place, **bad) == -1, (in_place, bad)
            assert a.last_error()
        assert rc(in_place, batch=0) == 0
        assert rc(in_place, batch=0, seq=None, counts=None, out=None) == 0
    assert (out == SENTINEL).all()
    assert 127 * ((2 ** 31 + 126) // 127) >= 2 ** 31 > 127 * ((2 ** 31 + 126) // 127 - 1)   # the first L that is refused


BOOTSTRAP_CASES = [(1, 3, 0), (7, 5, 1), (1000, 4, 2 ** 63 + 5)]


def check_bootstrap_counts(a, L, B, seed):
    got = _capi.run_bootstrap_counts(a, L, B, seed)
    assert got.dtype == np.uint16 and got.shape == (B, L)
    assert (got.astype(np.int64) == ref_bootstrap_counts(L, B, seed)).all()
    assert (got.astype(np.int64).sum(axis=1) == L).all()


@functools.lru_cache(maxsize=None)
def pipeline_case():
    seq = random_seq(33, 200, 840)
    counts = ref_bootstrap_counts(200, 20, 7).astype(np.uint16)
    D = ref_dist(seq, counts)
    D.setflags(write=False)
    return seq, counts, D

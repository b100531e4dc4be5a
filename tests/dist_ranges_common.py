"""Shared by tests/test_dist_ranges_emu.py (CPU driver) and tests/test_dist_ranges.py (the product on the GPU): the cases of the
alignment distances over site ranges.

Problem b of a range call is the alignment restricted to the sites starts[b] <= s < ends[b]; the entry writes the bytes of its
counts entry on counts[b][s] = [starts[b] <= s < ends[b]].  The reference is what the repository already has, imported unchanged
and fed those 0/1 counts: `dist_common.ref_dist`, `dist_model_common.ref_model`, `dist_pairs_common.ref_model` / `ref_tables`,
`dist_gamma_common.ref_model`.  Every matrix comparison is bitwise.  `also_counts` compares, in addition, with the bound
library's own counts entry on the same 0/1 counts (the product on the GPU; the driver has those entries too)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import dist_common as dc
import dist_gamma_common as gc
import dist_model_common as mc
import dist_pairs_common as pc
from dist_common import MISSING, SENTINEL, same_bits
from dist_pairs_common import ISENTINEL
from fastneighbornet_amd import _capi

EMU_SRCS = [os.path.join(dc.EMU_DIR, "fnn_dist_ranges_emu.cpp"), os.path.join(dc.CSRC, "fnn_dist_ranges.h")] + gc.EMU_SRCS
INF = float("inf")


def emu_dist_ranges_api():
    """tests/emu/fnn_dist_ranges_emu.cpp as a shared library: the range entries and the counts entries behind one backend (prefix
    emur_)."""
    out = os.path.join(dc.EMU_DIR, "build", "libfnn_dist_ranges_emu.so")
    if dc.newer(out, EMU_SRCS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                               "-o", out, EMU_SRCS[0]])
    a = _capi.Api(C.CDLL(out), "emur_", engine=False)
    _capi.bind_dist_model(a)
    _capi.bind_pair_counts(a)
    _capi.bind_ranges(a)
    return a


# ---- ranges, their counts and the reference -----------------------------------------------------------------------------------

def as_bounds(ranges):
    r = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    return r[:, 0].copy(), r[:, 1].copy()


def counts_of(starts, ends, L):
    """The 0/1 counts of the ranges: what a caller of the counts entries has to build."""
    s = np.arange(L, dtype=np.int64)[None, :]
    return ((np.asarray(starts)[:, None] <= s) & (s < np.asarray(ends)[:, None])).astype(np.uint16)


def ref_model(seq, counts, model, shape=None, states=4):
    """(D, failures) of the existing references on `counts`; "p": failures are the empty pairs."""
    if model == "p":
        mism, valid = dc.ref_sums(seq, counts)
        n = mism.shape[1]
        off = ~np.eye(n, dtype=bool)[None]
        failures = [(int(b), int(i), int(j), "empty") for b, i, j in np.argwhere((valid == 0) & np.triu(np.ones((n, n), dtype=bool), 1)[None])]
        with np.errstate(invalid="ignore", divide="ignore"):
            D = np.where(off, mism.astype(np.float64) / valid.astype(np.float64), 0.0)
        return D, failures
    if shape is not None:
        return gc.ref_model(seq, counts, model, shape, states)
    if model in pc.MODELS:
        return pc.ref_model(seq, counts, model)
    return mc.ref_model(seq, counts, model, states)


def ref_clean(seq, counts, model, shape=None, states=4):
    if model == "p":
        return dc.ref_dist(seq, counts)
    D, failures = ref_model(seq, counts, model, shape, states)
    assert not failures, f"the case has an empty, degenerate or saturated pair: {failures[:3]}"
    return D


# ---- one call -----------------------------------------------------------------------------------------------------

def padded_seq(seq, lds, pad_seed):
    n, L = seq.shape
    s_buf = np.frombuffer(b"ACGT\xff", dtype=np.uint8)[np.random.default_rng(pad_seed).integers(0, 5, (n, lds))].copy()
    s_buf[:, :L] = seq
    return s_buf


def call(a, seq, starts, ends, model="p", shape=None, states=4, on_saturation="fail", cap=None, lds=None, ld=None, stride=None, in_place=False,
         pad_seed=99):
    """One call through the raw range entry: the alignment's padding holds values that would change the result if read, the
    output's padding holds SENTINEL.  Returns (D[B, n, n] view, the whole output, stats).  in_place: the device entry (the CPU
    driver's writes host memory in place); "torch": into a tensor on the GPU."""
    seq = np.asarray(seq, dtype=np.uint8)
    starts, ends = np.ascontiguousarray(starts, dtype=np.int64), np.ascontiguousarray(ends, dtype=np.int64)
    (n, L), B = seq.shape, starts.shape[0]
    lds, ld = lds or L, ld or n
    stride = stride or n * ld
    s_buf = padded_seq(seq, lds, pad_seed)
    out = np.full(max(B * stride, 1), SENTINEL, dtype=np.float64)
    m = _capi.dist_model(model, states, on_saturation, cap, shape)
    if in_place == "torch":
        import torch
        t = torch.from_numpy(out).to("cuda:0")
        torch.cuda.synchronize()
        st = _capi.run_ranges(a, s_buf.ctypes.data, n, L, lds, starts.ctypes.data, ends.ctypes.data, B, t.data_ptr(), ld, stride, m, on_device=True)
        out = t.cpu().numpy()
    else:
        try:
            st = _capi.run_ranges(a, s_buf.ctypes.data, n, L, lds, starts.ctypes.data, ends.ctypes.data, B, out.ctypes.data, ld, stride, m,
                                  on_device=bool(in_place))
        except _capi.FnnError as e:
            e.out = out
            raise
    view = np.lib.stride_tricks.as_strided(out, (B, n, n), (8 * stride, 8 * ld, 8)) if B else np.zeros((0, n, n))
    return view, out, st


def call_tables(a, seq, starts, ends, lds=None, ld=None, stride=None, in_place=False, pad_seed=99):
    """`call` through the table entries: (F[B, n, n, 4, 4] view, the whole int64 output, stats); the padding holds ISENTINEL."""
    seq = np.asarray(seq, dtype=np.uint8)
    starts, ends = np.ascontiguousarray(starts, dtype=np.int64), np.ascontiguousarray(ends, dtype=np.int64)
    (n, L), B = seq.shape, starts.shape[0]
    lds, ld = lds or L, ld or n
    stride = stride or 16 * n * ld
    s_buf = padded_seq(seq, lds, pad_seed)
    out = np.full(max(B * stride, 1), ISENTINEL, dtype=np.int64)
    if in_place == "torch":
        import torch
        t = torch.from_numpy(out).to("cuda:0")
        torch.cuda.synchronize()
        st = _capi.run_pair_counts_ranges(a, s_buf.ctypes.data, n, L, lds, starts.ctypes.data, ends.ctypes.data, B, t.data_ptr(), ld, stride, on_device=True)
        out = t.cpu().numpy()
    else:
        st = _capi.run_pair_counts_ranges(a, s_buf.ctypes.data, n, L, lds, starts.ctypes.data, ends.ctypes.data, B, out.ctypes.data, ld, stride,
                                          on_device=bool(in_place))
    view = np.lib.stride_tricks.as_strided(out, (B, n, n, 4, 4), (8 * stride, 128 * ld, 128, 32, 8)) if B else np.zeros((0, n, n, 4, 4), dtype=np.int64)
    return view, out, st


def counts_entry(a, seq, counts, model, shape=None, **kw):
    """The bound library's counts entry on the same problem: the whole output array."""
    if model == "tables":
        return pc.call_counts(a, seq, counts, **kw)[1]
    return gc.call(a, seq, counts, model, shape, **kw)[1]


def check_stats(st, B, n, L, missing):
    assert st.model.base.n_problems == B and st.model.base.n_pairs == n * (n - 1) // 2 and st.model.base.n_sites == L
    assert st.model.base.digit_passes == 1 and st.model.base.block_threads == 256 and st.model.base.has_missing == int(missing)
    assert st.n_site_blocks_dense == -(-B // 16) * (-(-L // 64))


def tile_blocks(starts, ends):
    """n_site_blocks from its definition: per tile of 16 consecutive ranges, (ceil64(max end) - floor64(min start)) / 64 over the
    tile's non-empty ranges."""
    total = 0
    for k in range(0, len(starts), 16):
        live = [(int(s), int(e)) for s, e in zip(starts[k:k + 16], ends[k:k + 16]) if e > s]
        if live:
            total += -(-max(e for _, e in live) // 64) - min(s for s, _ in live) // 64
    return total


# ---- case 1: the range operand, every k ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def operand_case():
    n, L = 6, 130
    seq = dc.random_seq(n, L, 2001)
    starts, ends = as_bounds([(s, s + 1) for s in range(L)] + [(15, 17), (63, 65), (127, 129), (0, 130), (129, 130)])
    return seq, starts, ends


def check_operand(a, also_counts=False):
    """The 130 one-site ranges: every entry is exactly 0.0 or 1.0, namely seq[i][s] != seq[j][s] - a byte of the operand that is
    set at a wrong k, or for a wrong column, changes one; then ranges across the 16- and 64-byte boundaries, into the last
    block's padding, and the whole alignment.  B = 135."""
    seq, starts, ends = operand_case()
    n, L = seq.shape
    D, _, st = call(a, seq, starts, ends)
    for s in range(L):
        want = (seq[:, None, s] != seq[None, :, s]).astype(np.float64)
        assert same_bits(D[s], want), s
    counts = counts_of(starts, ends, L)
    assert same_bits(D, dc.ref_dist(seq, counts))
    check_stats(st, 135, n, L, False)
    assert st.n_site_blocks == tile_blocks(starts, ends)
    if also_counts:
        assert call(a, seq, starts, ends)[1].tobytes() == counts_entry(a, seq, counts, "p").tobytes()


# ---- case 2: grids of windows under every model ----------------------------------------------------------------------------------

GRIDS = [(17, 200, 96, 8, 11), (33, 330, 128, 6, 12), (6, 1000, 150, 25, 13)]   # n, L, width, step, seed
GRID_NAMES = ["n%d-L%d-w%d-s%d" % g[:4] for g in GRIDS]
GRID_B = [18, 38, 39]
GRID_MODELS = [("p", None), ("jc69", None), ("k2p", None), ("f81", None), ("felsenstein84", None), ("tn93", None), ("logdet", None), ("k2p", 0.5),
               ("tn93", 0.5), ("tables", None)]
GRID_MODEL_NAMES = [m if s is None else "%s-gamma" % m for m, s in GRID_MODELS]


def grid_ranges(L, width, step):
    from fastneighbornet_amd import window_ranges
    s, e = window_ranges(L, width, step)
    extra = as_bounds([(0, L), (L - 70, L), (3, 93), (L - 100, L)])
    return np.concatenate([s, extra[0]]), np.concatenate([e, extra[1]])


@functools.lru_cache(maxsize=None)
def grid_case(k, missing):
    n, L, width, step, seed = GRIDS[k]
    seq = dc.random_seq(n, L, seed, missing=0.02 if missing else 0.0)
    assert bool((seq == MISSING).any()) == missing
    starts, ends = grid_ranges(L, width, step)
    assert len(starts) == GRID_B[k]
    return seq, starts, ends, counts_of(starts, ends, L)


@functools.lru_cache(maxsize=None)
def grid_ref(k, missing, model, shape):
    """The reference, computed once for both suites; asserts that the input is clean under the model."""
    seq, _, _, counts = grid_case(k, missing)
    ref = pc.want_tables(seq, counts) if model == "tables" else ref_clean(seq, counts, model, shape)
    ref.setflags(write=False)
    return ref


def check_grid(a, k, missing, model, shape, also_counts=False):
    seq, starts, ends, counts = grid_case(k, missing)
    n, L = seq.shape
    ref = grid_ref(k, missing, model, shape)
    if model == "tables":
        F, out, st = call_tables(a, seq, starts, ends)
        assert F.shape == ref.shape and (F == ref).all()
    else:
        D, out, st = call(a, seq, starts, ends, model, shape)
        assert same_bits(D, ref)
        assert st.model.n_saturated_problems == 0
    check_stats(st, GRID_B[k], n, L, missing)
    assert st.model.n_recoded == 0 and st.n_site_blocks == tile_blocks(starts, ends)
    if also_counts:
        assert out.tobytes() == counts_entry(a, seq, counts, model, shape).tobytes()


# ---- case 3: order and spans ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def order_case():
    L, n = 1000, 5
    seq = dc.random_seq(n, L, 2003)
    grid = [(s, s + 100) for s in range(0, L - 100 + 1, 50)]
    pick = np.random.default_rng(2004).permutation(len(grid))[:14]
    ranges = [(0, 3), (997, 1000), (500, 564), (0, 1000), (500, 564), (510, 520)] + [grid[int(p)] for p in pick]
    starts, ends = as_bounds(ranges)
    assert len(starts) == 20
    return seq, starts, ends


def check_order_and_spans(a, also_counts=False):
    """Far-apart, nested and repeated ranges within one window tile and across two.  The same ranges sorted give the same
    matrices, permuted; n_site_blocks follows its definition and is smaller for the sorted order."""
    seq, starts, ends = order_case()
    n, L = seq.shape
    D, out, st = call(a, seq, starts, ends)
    counts = counts_of(starts, ends, L)
    assert same_bits(D, dc.ref_dist(seq, counts))
    perm = np.lexsort((ends, starts))
    Ds, _, sts = call(a, seq, starts[perm], ends[perm])
    assert same_bits(Ds, D[perm])
    assert same_bits(D[2], D[4])   # (the repeated range)
    want, want_sorted = tile_blocks(starts, ends), tile_blocks(starts[perm], ends[perm])
    assert st.n_site_blocks == want and sts.n_site_blocks == want_sorted and want_sorted < want
    assert st.n_site_blocks_dense == sts.n_site_blocks_dense == 2 * 16
    if also_counts:
        assert out.tobytes() == counts_entry(a, seq, counts, "p").tobytes()


# ---- case 4: a long walk -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def long_case():
    from fastneighbornet_amd import window_ranges
    n, L = 6, 20000
    seq = dc.random_seq(n, L, 2005, missing=0.02)
    starts, ends = window_ranges(L, 500, 125)
    assert len(starts) == 157
    counts = counts_of(starts, ends, L)
    ref = ref_clean(seq, counts, "k2p")
    ref.setflags(write=False)
    return seq, starts, ends, counts, ref


def check_long_walk(a, also_counts=False):
    """Offsets beyond one chunk of 64 blocks, spans that start far from 0: 157 windows of 500 sites along 20 000."""
    seq, starts, ends, counts, ref = long_case()
    D, out, st = call(a, seq, starts, ends, "k2p")
    assert same_bits(D, ref)
    check_stats(st, 157, 6, 20000, True)
    assert st.n_site_blocks == tile_blocks(starts, ends) and 8 * st.n_site_blocks < st.n_site_blocks_dense
    if also_counts:
        assert out.tobytes() == counts_entry(a, seq, counts, "k2p").tobytes()


# ---- case 5: failures -----------------------------------------------------------------------------------------------------------

def check_failures(a, also_counts=False):
    n, L = 5, 200
    full = dc.random_seq(n, L, 2006)
    starts, ends = as_bounds([(0, 200), (10, 90), (50, 50), (100, 180), (20, 20)])
    # without missing bytes an empty range is its total: (2, 0, 1), before any device use (the CPU suite runs this on the product too)
    for model, policy in (("p", "fail"), ("k2p", "cap"), ("tn93", "cap")):
        with pytest.raises(_capi.FnnError) as ei:
            call(a, full, starts, ends, model, on_saturation=policy, cap=3.0 if policy == "cap" else None)
        assert ei.value.code == -1 and "(2, 0, 1)" in str(ei.value) and "valid == 0" in str(ei.value), str(ei.value)
        assert (ei.value.out == SENTINEL).all()
    if a.prefix == "fnn_" and not also_counts:
        return   # (the rest needs a device)
    # with missing bytes: taxa 1 and 3 share no site inside range 3 only, which lies below the empty range 4
    seq = dc.random_seq(n, L, 2007, missing=0.02)
    seq[1, 100:140] = MISSING
    seq[3, 140:180] = MISSING
    starts, ends = as_bounds([(0, 200), (10, 90), (90, 190), (100, 180), (20, 20), (0, 100)])
    counts = counts_of(starts, ends, L)
    for model in ("p", "jc69", "k2p", "tn93"):
        failures = ref_model(seq, counts, model)[1]
        assert failures[0] == (3, 1, 3, "empty") and {f[0] for f in failures} == {3, 4}
        with pytest.raises(_capi.FnnError) as ei:
            call(a, seq, starts, ends, model)
        assert ei.value.code == -1 and "(3, 1, 3)" in str(ei.value) and "valid == 0" in str(ei.value), str(ei.value)
        assert (ei.value.out == SENTINEL).all()
        if also_counts:
            with pytest.raises(_capi.FnnError) as ec:
                gc.call(a, seq, counts, model, None)
            assert str(ec.value).split(": ", 2)[2] == str(ei.value).split(": ", 2)[2]   # (only the entry's name differs)
    # a range in which the pair differs at every site, a transversion each: saturated under JC69 and K2P (with a third taxon some
    # pair of it would be saturated under K2P too: every site gives one of its two pairs a transversion)
    sat = np.full((2, 128), ord("A"), dtype=np.uint8)
    sat[1, 64:96] = ord("C")
    starts, ends = as_bounds([(0, 128), (64, 96), (0, 64), (32, 128)])
    counts = counts_of(starts, ends, 128)
    for model in ("jc69", "k2p"):
        ref, failures = ref_model(sat, counts, model)
        assert failures == [(1, 0, 1, "saturated")]
        with pytest.raises(_capi.FnnError) as ei:
            call(a, sat, starts, ends, model)
        assert ei.value.code == -1 and "(1, 0, 1)" in str(ei.value) and "saturated" in str(ei.value), str(ei.value)
        assert (ei.value.out == SENTINEL).all()
        D, out, st = call(a, sat, starts, ends, model, on_saturation="cap", cap=7.5)
        want = ref.copy()
        want[want == INF] = 7.5
        assert same_bits(D, want) and (D == 7.5).sum() == 2 and st.model.n_saturated_problems == 1
        if also_counts:
            assert out.tobytes() == counts_entry(a, sat, counts, model, on_saturation="cap", cap=7.5).tobytes()
    # the tables never fail: an empty range is 16 zeros per pair
    starts, ends = as_bounds([(0, 128), (5, 5), (64, 96)])
    F, _, st = call_tables(a, sat, starts, ends)
    assert (F == pc.want_tables(sat, counts_of(starts, ends, 128))).all() and (F[1] == 0).all()


# ---- case 6: layouts and chunks --------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def layout_case():
    seq = dc.random_seq(7, 165, 2008, missing=0.05)
    starts, ends = as_bounds([(0, 165), (1, 120), (40, 165), (64, 128), (63, 129), (20, 150), (0, 100)])
    return seq, starts, ends, counts_of(starts, ends, 165)


def check_layout(a, in_place=False, also_counts=False):
    """Padded lds, ld and stride with sentinels in every padding."""
    seq, starts, ends, counts = layout_case()
    n, B = 7, 7
    for model in ("p", "k2p", "tn93"):
        ref = ref_clean(seq, counts, model)
        for lds, ld, stride in ((165 + 5, n + 2, n * (n + 2) + 11), (165, n, n * n + 1), (165 + 16, n + 1, n * (n + 1))):
            D, out, _ = call(a, seq, starts, ends, model, lds=lds, ld=ld, stride=stride, in_place=in_place)
            assert same_bits(D, ref), (model, lds, ld, stride)
            dc.assert_padding_untouched(out, B, n, ld, stride)
            if also_counts:
                assert out.tobytes() == counts_entry(a, seq, counts, model, lds=lds, ld=ld, stride=stride, in_place=in_place).tobytes()
    want = pc.want_tables(seq, counts)
    for lds, ld, stride in ((165 + 5, n + 2, 16 * n * (n + 2) + 11), (165, n, 16 * n * n)):
        F, out, _ = call_tables(a, seq, starts, ends, lds=lds, ld=ld, stride=stride, in_place=in_place)
        assert (F == want).all()
        pc.assert_counts_padding_untouched(out, B, n, ld, stride)


def check_chunking(a, monkeypatch, model, in_place=False):
    """FNN_BATCH_CHUNK=3 at B = 7: three chunks, each with its own bounds and spans; padded layout, padding untouched."""
    seq, starts, ends, counts = layout_case()
    ref = ref_clean(seq, counts, model)
    monkeypatch.setenv("FNN_BATCH_CHUNK", "3")
    D, out, st = call(a, seq, starts, ends, model, lds=170, ld=9, stride=70, in_place=in_place)
    monkeypatch.delenv("FNN_BATCH_CHUNK")
    assert st.model.base.chunks == 3 and same_bits(D, ref)
    dc.assert_padding_untouched(out, 7, 7, 9, 70)
    assert st.n_site_blocks == sum(tile_blocks(starts[k:k + 3], ends[k:k + 3]) for k in (0, 3, 6))   # (a chunk starts a new tile)
    assert call(a, seq, starts, ends, model)[2].model.base.chunks == 1


# ---- case 7: arguments, without a device -------------------------------------------------------------------------------------------

def check_arguments(a):
    """The argument checks come before any device use: they hold without a GPU.  All four range entries."""
    n, L, B = 4, 10, 3
    seq = dc.random_seq(n, L, 2009)
    starts, ends = as_bounds([(0, 10), (2, 7), (5, 10)])
    out = np.full(16 * B * n * n, SENTINEL)
    good = dict(seq=seq.ctypes.data, n=n, L=L, lds=L, starts=starts.ctypes.data, ends=ends.ctypes.data, batch=B, out=out.ctypes.data, ld=n)

    def rc(entry, m=None, **kw):
        k = dict(good, **kw)
        if entry < 2:
            fn = a.alignment_distances_ranges_device_f64 if entry else a.alignment_distances_ranges_f64
            m = _capi.dist_model() if m is None else m
            return fn(k["seq"], k["n"], k["L"], k["lds"], k["starts"], k["ends"], k["batch"], _capi.dist_model_ref(m) if m != "null" else None, 0, k["out"],
                      k["ld"], k.get("stride", n * n), None)
        fn = a.alignment_pair_counts_ranges_device_i64 if entry == 3 else a.alignment_pair_counts_ranges_i64
        return fn(k["seq"], k["n"], k["L"], k["lds"], k["starts"], k["ends"], k["batch"], 0, k["out"], k["ld"], k.get("stride", 16 * n * n), None)

    def bounds(ranges):
        s, e = as_bounds(ranges)
        keep.extend([s, e])
        return dict(starts=s.ctypes.data, ends=e.ctypes.data)

    keep = []
    for entry in range(4):
        cell = 1 if entry < 2 else 16
        for bad in (dict(L=0), dict(n=0), dict(n=-3), dict(lds=L - 1), dict(ld=n - 1), dict(stride=cell * n * n - 1), dict(seq=None), dict(starts=None),
                    dict(ends=None), dict(out=None), dict(batch=-1), dict(L=(2 ** 31 + 126) // 127, lds=2 ** 40)):
            assert rc(entry, **bad) == -1 and a.last_error(), (entry, bad)
        # a range outside 0 <= start <= end <= L: the lowest such b is named
        for ranges, b in (([(0, 10), (-1, 4), (3, 11)], 1), ([(0, 10), (2, 7), (6, 5)], 2), ([(0, 11), (2, 7), (5, 10)], 0), ([(0, 10), (11, 11), (-2, -1)], 1)):
            assert rc(entry, **bounds(ranges)) == -1 and b"range %d:" % b in a.last_error(), (entry, ranges, a.last_error())
        assert rc(entry, batch=0) == 0
        assert rc(entry, batch=0, seq=None, starts=None, ends=None, out=None) == 0
    for entry in range(2):
        assert rc(entry, m="null") == -1 and b"NULL model" in a.last_error()
        assert rc(entry, m=_capi.dist_model(3)) == -1 and b"unknown model" in a.last_error()
        assert rc(entry, m=_capi.dist_model("k2p", on_saturation=2)) == -1 and rc(entry, m=_capi.dist_model("k2p", on_saturation="cap")) == -1
        assert rc(entry, m=_capi.dist_model("jc69", states=1)) == -1
        for model in ("p", "logdet"):
            assert rc(entry, m=_capi.dist_model(model, gamma_shape=0.5)) == -1 and b"gamma" in a.last_error()
        for shape in (0.0, -1.0, INF, float("nan")):
            assert rc(entry, m=_capi.dist_model("tn93", gamma_shape=shape)) == -1 and b"shape" in a.last_error()
        assert rc(entry, m=_capi.dist_model("tn93", gamma_shape=float("nan")), batch=0) == -1   # (the checks come first)
        assert rc(entry, m=_capi.dist_model("tn93", gamma_shape=0.5), batch=0) == 0
    assert (out == SENTINEL).all()


STRUCT_C = ('#include <stdio.h>\n#include <stddef.h>\n#include "fastnn.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(fnn_range_stats), '
            'offsetof(fnn_range_stats, n_site_blocks), offsetof(fnn_range_stats, n_site_blocks_dense), offsetof(fnn_range_stats, reserved), '
            'sizeof(fnn_dist_model_stats)); return 0; }\n')


def check_struct(tmp_path):
    """sizeof and offsets of fnn_range_stats against the C compiler's."""
    src = tmp_path / "ranges.c"
    src.write_text(STRUCT_C)
    exe = tmp_path / "ranges"
    subprocess.check_call(["gcc", "-I", os.path.join(dc.ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    R = _capi.FnnRangeStats
    assert got == [C.sizeof(R), R.n_site_blocks.offset, R.n_site_blocks_dense.offset, R.reserved.offset, C.sizeof(_capi.FnnDistModelStats)]
    assert got[0] == got[4] + 48


# ---- case 10: the pipeline's reference matrices --------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pipeline_case():
    """n = 33, L = 330, windows of 128 every 6 sites (grid 1 without its four extra ranges), TN93."""
    from fastneighbornet_amd import window_ranges
    seq = grid_case(1, False)[0]
    starts, ends = window_ranges(330, 128, 6)
    D = ref_clean(seq, counts_of(starts, ends, 330), "tn93")
    D.setflags(write=False)
    return seq, starts, ends, D

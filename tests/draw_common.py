"""Shared by tests/test_draw_emu.py (CPU driver) and tests/test_draw.py (the product on the GPU): the cases of the bootstrap
entries that draw their replicates on the device.

The reference is what the repository has: `dist_common.ref_bootstrap_counts` (Python integers) for the counts - with an all-ones
row in front for lead = 1 -, then `dist_common.ref_dist` or `dist_model_common.ref_model` on those counts.  Every matrix comparison
is bitwise.  Every case builder asserts that its reference has no empty or saturated pair it did not ask for."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import dist_common as dc
import dist_model_common as mc
from dist_common import MISSING, SENTINEL, same_bits
from fastneighbornet_amd import _capi

EMU_SRCS = [os.path.join(dc.EMU_DIR, "fnn_draw_emu.cpp"), os.path.join(dc.CSRC, "fnn_draw.h")] + mc.EMU_SRCS
M64 = 2 ** 64 - 1
MODELS = ["p", "jc69", "k2p"]


def emu_draw_api():
    """tests/emu/fnn_draw_emu.cpp as a shared library: the bootstrap entries, the model entries and emu_bootstrap_draw_planes."""
    out = os.path.join(dc.EMU_DIR, "build", "libfnn_draw_emu.so")
    if dc.newer(out, EMU_SRCS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                               "-o", out, EMU_SRCS[0]])
    a = _capi.bind_boot(_capi.bind_dist_model(_capi.Api(C.CDLL(out), "emu_", engine=False)))
    a._fn("bootstrap_draw_planes", C.c_int32, [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p])
    return a


# ---- the reference ----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ref_counts(L, batch, seed, lead=0):
    """The counts the call stands for: uint16 (batch, L); `lead` rows of ones, then the replicates of (L, batch - lead, seed)."""
    c = np.concatenate([np.ones((lead, L), dtype=np.int64), dc.ref_bootstrap_counts(L, batch - lead, seed)])
    assert (c.sum(axis=1) == L).all() and c.max() <= 127
    c = c.astype(np.uint16)
    c.setflags(write=False)
    return c


def ref_matrices(seq, counts, model, states=4):
    return dc.ref_dist(seq, counts) if model == "p" else mc.ref_clean(seq, counts, model, states)


def is_clean(seq, counts, model):
    if model == "p":
        return dc.first_empty(dc.ref_sums(seq, counts)[1]) is None
    return mc.is_clean(seq, counts, model)


# ---- one call -----------------------------------------------------------------------------------------------------

def call(a, seq, batch, seed, lead=0, model="p", states=4, on_saturation="fail", cap=None, lds=None, ld=None, stride=None, in_place=False,
         pad_seed=99):
    """One call through the raw entry: the alignment's padding holds bytes that would change the result if read, the output's
    padding holds SENTINEL.  Returns (D[batch, n, n] view, the whole output, stats)."""
    seq = np.asarray(seq, dtype=np.uint8)
    n, L = seq.shape
    lds, ld = lds or L, ld or n
    stride = stride or n * ld
    r = np.random.default_rng(pad_seed)
    s_buf = np.frombuffer(b"ACGT\xff", dtype=np.uint8)[r.integers(0, 5, (n, lds))].copy()
    s_buf[:, :L] = seq
    out = np.full(max(batch * stride, 1), SENTINEL, dtype=np.float64)
    m = _capi.dist_model(model, states, on_saturation, cap)
    if in_place == "torch":   # the product's device entry: the output is a tensor on the GPU
        import torch
        t = torch.from_numpy(out).to("cuda:0")
        torch.cuda.synchronize()
        st = _capi.run_boot(a, s_buf.ctypes.data, n, L, lds, batch, seed, lead, t.data_ptr(), ld, stride, m, on_device=True)
        out = t.cpu().numpy()
    else:
        try:
            st = _capi.run_boot(a, s_buf.ctypes.data, n, L, lds, batch, seed, lead, out.ctypes.data, ld, stride, m, on_device=bool(in_place))
        except _capi.FnnError as e:
            e.out = out
            raise
    view = np.lib.stride_tricks.as_strided(out, (batch, n, n), (8 * stride, 8 * ld, 8)) if batch else np.zeros((0, n, n))
    return view, out, st


def route(st):
    return _capi.DRAW_ROUTES[st.draw_route]


# ---- case 1: the counts themselves --------------------------------------------------------------------------------

PLANE_CASES = [(1, 1, 0, 0, 1), (15, 15, 7, 0, 1), (17, 16, M64, 1, 1), (64, 17, 0, 0, 2), (65, 63, 7, 1, 3), (130, 64, M64, 0, 1), (200, 70, 7, 1, 2),
               (63, 65, 0, 1, 1), (16, 1, 7, 1, 1)]


def check_planes(a, L, batch, seed, lead, digits, first=0):
    """The driver's export: one launch of the draw.  Every byte of every plane against the reference's digits - rows behind the
    batch and sites behind L zero -, every row's total and the largest count.  first > 0: a later chunk of a longer call."""
    lpad, rows = -(-L // 64) * 64, -(-batch // 64) * 64
    planes = np.full((digits, rows, lpad), 0x55, dtype=np.int8)
    total = np.full(rows, -1, dtype=np.int64)
    most = np.zeros(1, dtype=np.uint32)
    a.check(a.bootstrap_draw_planes(L, batch, first, lead, seed, digits, planes.ctypes.data, total.ctypes.data, most.ctypes.data))
    want = ref_counts(L, first + batch, seed, lead)[first:].astype(np.int64)
    for d in range(digits):
        ref = np.zeros((rows, lpad), dtype=np.int64)
        ref[:batch, :L] = (want >> (7 * d)) & 127
        assert (planes[d].astype(np.int64) == ref).all(), d
    assert (total[:batch] == L).all() and (total[batch:] == 0).all()
    assert int(most[0]) == int(want.max())


def check_single_counts(a, L=17, B=17, seed=7):
    """n = 3 rows in which site s differs only at s: row 0 is all A, row 1 differs from it at site s, row 2 at site s'.  The
    matrix of replicate b then holds count[b][s] / L, count[b][s'] / L and their sum / L: every count of every replicate
    read off a matrix entry, ceil(L / 2) calls."""
    counts = ref_counts(L, B, seed)
    for s in range(0, L, 2):
        s2 = s + 1 if s + 1 < L else 0
        seq = np.full((3, L), ord("A"), dtype=np.uint8)
        seq[1, s] = ord("C")
        seq[2, s2] = ord("G")
        D, _, st = call(a, seq, B, seed)
        for b in range(B):
            c1, c2 = int(counts[b, s]), int(counts[b, s2])
            assert D[b, 0, 1] == float(c1) / float(L) and D[b, 0, 2] == float(c2) / float(L) and D[b, 1, 2] == float(c1 + c2) / float(L), (s, b)
        assert st.max_count == int(counts.max()) and route(st) == "device"


# ---- case 2: shapes and models -------------------------------------------------------------------------------------
# every L of {1, 15, 16, 17, 63, 64, 65, 130, 200}, every B of {1, 15, 16, 17, 63, 64, 65, 70} (the replicate padding edges of
# 16 RT and 64), the seeds 0, 7, 2^64 - 1, every n of {1, 2, 5, 17, 33}: (n, L, B, seed)
SHAPES = [(1, 1, 1, 0), (2, 15, 15, 7), (5, 16, 16, M64), (17, 17, 17, 0), (33, 63, 63, 7), (2, 64, 64, M64), (5, 65, 65, 0), (17, 130, 70, 7),
          (33, 200, 1, M64), (2, 200, 70, 0), (5, 1, 17, 7)]
SHAPE_IDS = ["n%d-L%d-B%d-s%d" % (n, L, B, min(seed, 9)) for n, L, B, seed in SHAPES]


@functools.lru_cache(maxsize=None)
def shape_case(k, model, missing):
    """The first alignment seed from 1500 + 40 k on for which no replicate has an empty or a saturated pair (at L = 1 every
    mismatch saturates and every missing byte empties: the rows are equal and complete there)."""
    n, L, B, seed = SHAPES[k]
    counts = ref_counts(L, B, seed)
    for s in range(1500 + 40 * k, 1500 + 40 * k + 4000):
        seq = dc.random_seq(n, L, s, missing=0.05 if missing and L > 1 else 0.0)
        if L == 1:
            seq[:] = seq[0]
        if is_clean(seq, counts, model):
            ref = ref_matrices(seq, counts, model)
            ref.setflags(write=False)
            return seq, ref
    raise AssertionError("no clean alignment found")


def check_shape(a, k, model, missing):
    n, L, B, seed = SHAPES[k]
    seq, ref = shape_case(k, model, missing)
    D, _, st = call(a, seq, B, seed, model=model)
    assert same_bits(D, ref)
    base = st.model.base
    assert base.has_missing == int((seq == MISSING).any()) and base.digit_passes == 1 and base.n_problems == B and base.n_sites == L
    assert route(st) == "device" and st.max_count == int(ref_counts(L, B, seed).max()) and st.t_draw_s >= 0.0
    assert st.model.n_recoded == 0 and st.model.n_saturated_problems == 0


@functools.lru_cache(maxsize=None)
def k2p_rt2_case():
    """K2P with missing bytes at B = 65: with three digit planes the kernel runs two replicate tiles per wave, three replicate
    groups of 32."""
    n, L, B, seed = 7, 65, 65, 7
    counts = ref_counts(L, B, seed)
    for s in range(1700, 5700):
        seq = dc.random_seq(n, L, s, missing=0.05)
        if is_clean(seq, counts, "k2p") and (seq == MISSING).any():
            return seq, B, seed, mc.ref_clean(seq, counts, "k2p")
    raise AssertionError("no clean alignment found")


def check_k2p_three_planes(a, monkeypatch):
    seq, B, seed, ref = k2p_rt2_case()
    monkeypatch.setenv("FNN_DIST_FORCE_DIGITS", "3")
    D, _, st = call(a, seq, B, seed, model="k2p")
    monkeypatch.delenv("FNN_DIST_FORCE_DIGITS")
    assert st.model.base.digit_passes == 3 and st.model.base.has_missing == 1 and same_bits(D, ref)


# ---- case 3: lead -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def lead_case(model):
    n, L, B, seed = 5, 65, 17, 7
    for s in range(1900, 5900):
        seq = dc.random_seq(n, L, s, missing=0.05)
        if is_clean(seq, ref_counts(L, B + 1, seed, 1), model):
            return seq, B, seed
    raise AssertionError("no clean alignment found")


def check_lead(a, model):
    """lead = 1: problem 0 is the all-ones call through the counts entry, problems 1 ... are lead = 0's problems 0 ...; batch = 1
    with lead = 1 is that one problem."""
    seq, B, seed = lead_case(model)
    n, L = seq.shape
    D1, _, st1 = call(a, seq, B + 1, seed, lead=1, model=model)
    D0, _, _ = call(a, seq, B, seed, lead=0, model=model)
    ones, _, _ = mc.call(a, seq, np.ones((1, L), dtype=np.uint16), model)
    assert same_bits(D1[:1], ones) and same_bits(D1[1:], D0)
    assert same_bits(D1, ref_matrices(seq, ref_counts(L, B + 1, seed, 1), model)) and st1.model.base.n_problems == B + 1
    only, _, st = call(a, seq, 1, seed, lead=1, model=model)
    assert same_bits(only, ones) and st.max_count == 1 and st.model.base.n_problems == 1


# ---- case 4: forced digits -----------------------------------------------------------------------------------------------

def check_forced_digits(a, monkeypatch, model):
    seq, B, seed = lead_case(model)
    D1, out1, st1 = call(a, seq, B + 1, seed, lead=1, model=model)
    assert st1.model.base.digit_passes == 1
    for digits in (2, 3):
        monkeypatch.setenv("FNN_DIST_FORCE_DIGITS", str(digits))
        D, out, st = call(a, seq, B + 1, seed, lead=1, model=model)
        monkeypatch.delenv("FNN_DIST_FORCE_DIGITS")
        assert st.model.base.digit_passes == digits and out.tobytes() == out1.tobytes()


# ---- case 5: chunking and layout ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def layout_case():
    n, L, B, seed = 7, 65, 7, 2 ** 63 + 5
    for s in range(2100, 6100):
        seq = dc.random_seq(n, L, s, missing=0.1)
        if is_clean(seq, ref_counts(L, B, seed, 1), "k2p"):
            return seq, B, seed, mc.ref_clean(seq, ref_counts(L, B, seed, 1), "k2p")
    raise AssertionError("no clean alignment found")


def check_layout(a, in_place=False):
    seq, B, seed, ref = layout_case()
    n = 7
    for lds, ld, stride in ((65 + 5, n + 2, n * (n + 2) + 11), (65, n, n * n + 1), (65 + 16, n + 1, n * (n + 1))):
        D, out, _ = call(a, seq, B, seed, lead=1, model="k2p", lds=lds, ld=ld, stride=stride, in_place=in_place)
        assert same_bits(D, ref), (lds, ld, stride)
        dc.assert_padding_untouched(out, B, n, ld, stride)


def check_chunking(a, monkeypatch, in_place=False):
    """Three chunks of 3, 3 and 1 problems: the replicate a row draws is the call's b - lead, not the chunk's."""
    seq, B, seed, ref = layout_case()
    monkeypatch.setenv("FNN_BATCH_CHUNK", "3")
    D, out, st = call(a, seq, B, seed, lead=1, model="k2p", ld=9, stride=70, in_place=in_place)
    monkeypatch.delenv("FNN_BATCH_CHUNK")
    assert st.model.base.chunks == 3 and same_bits(D, ref) and st.max_count == int(ref_counts(65, B, seed, 1).max())
    dc.assert_padding_untouched(out, 7, 7, 9, 70)
    assert call(a, seq, B, seed, lead=1, model="k2p")[2].model.base.chunks == 1


# ---- case 6: the site limit ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def limit_case(L):
    seq = dc.random_seq(2, L, 2300)
    ref = dc.ref_dist(seq, ref_counts(L, 2, 7))
    ref.setflags(write=False)
    return seq, ref


def check_limit(a, monkeypatch, above):
    """L = the limit is drawn on the device, L + 1 on the host; both are the reference."""
    limit = a.bootstrap_draw_max_sites()
    assert limit >= 30000
    monkeypatch.delenv("FNN_DRAW_ROUTE", raising=False)
    L = limit + (1 if above else 0)
    seq, ref = limit_case(L)
    D, _, st = call(a, seq, 2, 7)
    assert route(st) == ("host" if above else "device") and same_bits(D, ref)
    assert st.max_count == int(ref_counts(L, 2, 7).max()) and st.model.base.n_sites == L


def check_forced_device_above_the_limit(a, monkeypatch):
    """FNN_DRAW_ROUTE=device above the limit: FNN_EINVAL before any device use (it holds without a GPU)."""
    L = a.bootstrap_draw_max_sites() + 1
    monkeypatch.setenv("FNN_DRAW_ROUTE", "device")
    with pytest.raises(_capi.FnnError) as ei:
        call(a, np.full((2, L), ord("A"), dtype=np.uint8), 2, 7)
    monkeypatch.delenv("FNN_DRAW_ROUTE")
    assert ei.value.code == -1 and "sites" in str(ei.value) and (ei.value.out == SENTINEL).all()


def check_forced_host(a, monkeypatch, model):
    seq, B, seed = lead_case(model)
    D0, out0, st0 = call(a, seq, B + 1, seed, lead=1, model=model)
    monkeypatch.setenv("FNN_DRAW_ROUTE", "host")
    D1, out1, st1 = call(a, seq, B + 1, seed, lead=1, model=model)
    monkeypatch.delenv("FNN_DRAW_ROUTE")
    assert (route(st0), route(st1)) == ("device", "host") and out0.tobytes() == out1.tobytes()
    assert st0.max_count == st1.max_count and st1.t_draw_s == 0.0


# ---- case 7: empty and saturated pairs -----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def empty_pair_case():
    """n = 3, L = 8, 12 replicates: taxon 1 is present at site 0 only, so its pairs are empty in a replicate that never draws site
    0.  The first seed for which exactly one replicate does that, and not the first one."""
    seq = dc.random_seq(3, 8, 2500)
    seq[:, 0] = ord("A")   # (equal where taxon 1 is present: its pairs are never saturated)
    seq[1, 1:] = MISSING
    for seed in range(0, 4000):
        counts = ref_counts(8, 12, seed)
        hit = np.flatnonzero(counts[:, 0] == 0)
        if len(hit) == 1 and hit[0] > 0:
            valid = dc.ref_sums(seq, counts)[1]
            off = ~np.eye(3, dtype=bool)[None]
            assert dc.first_empty(valid) == (int(hit[0]), 0, 1) and ((valid == 0) & off).sum() == 4   # (0, 1) and (1, 2), both triangles
            for model in ("jc69", "k2p"):   # no saturated pair in a lower replicate (or anywhere)
                assert mc.ref_model(seq, counts, model)[1] == [(int(hit[0]), 0, 1, "empty"), (int(hit[0]), 1, 2, "empty")]
            return seq, seed, int(hit[0])
    raise AssertionError("no seed found")


def check_empty_pair(a, in_place=False):
    seq, seed, b = empty_pair_case()
    for kw in (dict(model="p"), dict(model="jc69"), dict(model="k2p", on_saturation="cap", cap=5.0)):
        with pytest.raises(_capi.FnnError) as ei:
            call(a, seq, 12, seed, in_place=in_place, **kw)
        assert ei.value.code == -1 and f"({b}, 0, 1)" in str(ei.value) and "valid == 0" in str(ei.value), str(ei.value)
        if not in_place:
            assert (ei.value.out == SENTINEL).all()
    # with the original data in front the replicate is problem b + 1
    with pytest.raises(_capi.FnnError) as ei:
        call(a, seq, 13, seed, lead=1)
    assert f"({b + 1}, 0, 1)" in str(ei.value) and (ei.value.out == SENTINEL).all()


@functools.lru_cache(maxsize=None)
def saturated_case():
    """n = 3, L = 8, 12 replicates, JC69: taxon 2 differs from the two others at five sites of eight; a replicate that draws
    them six times or more is saturated (4 m >= 3 * 8).  The first seed with some such replicates, not the first one among
    them, and some without."""
    seq = np.full((3, 8), ord("A"), dtype=np.uint8)
    seq[2, :5] = ord("C")
    for seed in range(0, 4000):
        counts = ref_counts(8, 12, seed)
        sat = counts[:, :5].astype(np.int64).sum(axis=1) >= 6
        if 2 <= sat.sum() <= 9 and not sat[0]:
            ref, failures = mc.ref_model(seq, counts, "jc69")
            assert all(f[3] == "saturated" for f in failures) and failures[0][:3] == (int(np.flatnonzero(sat)[0]), 0, 2)
            return seq, seed, ref, failures, int(sat.sum())
    raise AssertionError("no seed found")


def check_saturated_pair(a):
    seq, seed, ref, failures, n_sat = saturated_case()
    b, i, j, _ = failures[0]
    with pytest.raises(_capi.FnnError) as ei:
        call(a, seq, 12, seed, model="jc69")
    assert ei.value.code == -1 and f"({b}, {i}, {j})" in str(ei.value) and "saturated" in str(ei.value), str(ei.value)
    assert (ei.value.out == SENTINEL).all()
    D, _, st = call(a, seq, 12, seed, model="jc69", on_saturation="cap", cap=7.5)
    want = ref.copy()
    want[want == mc.INF] = 7.5
    assert same_bits(D, want) and (D == 7.5).sum() == len(failures) * 2
    assert st.model.n_saturated_problems == n_sat


# ---- case 8: arguments and struct ----------------------------------------------------------------------------------------------

def check_arguments(a, monkeypatch):
    """The argument checks come before any device use: they hold without a GPU."""
    monkeypatch.delenv("FNN_DRAW_ROUTE", raising=False)
    n, L, B = 4, 10, 3
    seq = dc.random_seq(n, L, 830)
    out = np.full(B * n * n, SENTINEL)
    good = dict(seq=seq.ctypes.data, n=n, L=L, lds=L, batch=B, seed=7, lead=0, out=out.ctypes.data, ld=n, stride=n * n)

    def rc(in_place, m, **kw):
        k = dict(good, **kw)
        fn = a.bootstrap_distances_batch_device_f64 if in_place else a.bootstrap_distances_batch_f64
        return fn(k["seq"], k["n"], k["L"], k["lds"], k["batch"], k["seed"], k["lead"], C.byref(m) if m is not None else None, 0, k["out"],
                  k["ld"], k["stride"], None)

    M = _capi.dist_model
    for in_place in (False, True):
        for route_switch in (None, "host", "device"):
            if route_switch:
                monkeypatch.setenv("FNN_DRAW_ROUTE", route_switch)
            for m in (None, M(3), M(-1), M("jc69", on_saturation=2), M("jc69", states=1), M("jc69", states=256), M("jc69", states=3),
                      M("k2p", on_saturation="cap"), M("jc69", on_saturation="cap", cap=mc.NAN)):
                assert rc(in_place, m) == -1, (in_place, m and (m.model, m.states, m.on_saturation, m.cap))
                assert a.last_error()
            for model in MODELS:
                for bad in (dict(lead=2), dict(lead=-1), dict(lead=1, batch=0), dict(L=0), dict(n=0), dict(lds=L - 1), dict(ld=n - 1),
                            dict(stride=n * n - 1), dict(seq=None), dict(out=None), dict(batch=-1), dict(L=(2 ** 31 + 126) // 127, lds=2 ** 40)):
                    assert rc(in_place, M(model), **bad) == -1, (in_place, model, bad)
                assert rc(in_place, M(model), lead=2) == -1 and b"lead" in a.last_error()
                assert rc(in_place, M(model), batch=0) == 0
                assert rc(in_place, M(model), batch=0, seq=None, out=None) == 0
            if route_switch:
                monkeypatch.delenv("FNN_DRAW_ROUTE")
    assert (out == SENTINEL).all()


STRUCT_SIZES_C = ('#include <stdio.h>\n#include <stddef.h>\n#include "fastnn.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %d %d\\n", '
                  'sizeof(fnn_boot_stats), sizeof(fnn_dist_model_stats), offsetof(fnn_boot_stats, draw_route), offsetof(fnn_boot_stats, max_count), '
                  'offsetof(fnn_boot_stats, t_draw_s), offsetof(fnn_boot_stats, reserved), (int)FNN_DRAW_DEVICE, (int)FNN_DRAW_HOST); return 0; }\n')


def check_struct_sizes(tmp_path):
    src = tmp_path / "size.c"
    src.write_text(STRUCT_SIZES_C)
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(dc.ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    S = _capi.FnnBootStats
    assert got == [C.sizeof(S), C.sizeof(_capi.FnnDistModelStats), S.draw_route.offset, S.max_count.offset, S.t_draw_s.offset, S.reserved.offset,
                   _capi.DRAW_DEVICE, _capi.DRAW_HOST]
    assert got[:2] == [128 + 48, 128]   # the model stats' size is pinned; the new struct adds two words, a double and four reserved words

"""Shared by tests/test_bootscan_emu.py (CPU driver) and tests/test_bootscan.py (the product on the GPU): the cases of the bootscan
entries - R bootstrap replicates inside every site range, with `lead` problems of the range's original data
in front.

The definition is restated here in Python integers (`ref_counts`) and checked against `fnn_bootscan_counts`; every distance entry
is then compared, bitwise and with no case excluded, with the bound library's own counts entry on `fnn_bootscan_counts`, whose
bytes the entry promises - outputs whole, padding included, and failures by status and message -, with the bootstrap entry on each
window's slice, and the routes with each other."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import dist_common as dc
import dist_ranges_common as rc
from dist_common import MISSING, SENTINEL
from dist_pairs_common import ISENTINEL
from fastneighbornet_amd import _capi

EMU_SRCS = [os.path.join(dc.EMU_DIR, "fnn_bootscan_emu.cpp"), os.path.join(dc.CSRC, "fnn_scan.h")] + rc.EMU_SRCS
M64 = 2 ** 64 - 1
GROUP_ROWS = {False: 64, True: 32}   # rows of a column group: 16 RT, the models' RT = 4 and the tables' 2


def emu_bootscan_api():
    """tests/emu/fnn_bootscan_emu.cpp as a shared library: the bootscan entries, the counts and bootstrap entries behind one backend
    (prefix emus_) and emus_bootscan_draw_planes."""
    out = os.path.join(dc.EMU_DIR, "build", "libfnn_bootscan_emu.so")
    if dc.newer(out, EMU_SRCS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                               "-o", out, EMU_SRCS[0]])
    a = _capi.Api(C.CDLL(out), "emus_", engine=False)
    _capi.bind_dist_model(a)
    _capi.bind_pair_counts(a)
    _capi.bind_boot(a)
    _capi.bind_scan(a)
    a._fn("bootstrap_counts", C.c_int32, [C.c_int64, C.c_int64, C.c_uint64, C.c_void_p])
    a._fn("bootscan_draw_planes", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_uint64, C.c_int64, C.c_int64, C.c_int32,
                                              C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p])
    return a


# ---- the definition ---------------------------------------------------------------------------------------------------------------

def seed_of(seed, w):
    return dc.splitmix64_at(seed & M64, w)


def ref_counts(L, starts, ends, R, seed, lead):
    """The definition in Python integers: int64 (W (R + lead), L)."""
    P = R + lead
    out = np.zeros((len(starts) * P, L), dtype=np.int64)
    for w, (s, e) in enumerate(zip(starts, ends)):
        s, e = int(s), int(e)
        width, sw = e - s, seed_of(seed, w)
        for q in range(P):
            if q < lead:
                out[w * P + q, s:e] = 1
                continue
            for k in range(width):
                out[w * P + q, s + ((dc.splitmix64_at(sw, (q - lead) * width + k) * width) >> 64)] += 1
    return out


def counts_of(a, L, starts, ends, R, seed, lead, **kw):
    return _capi.run_bootscan_counts(a, L, starts, ends, R, seed, lead, **kw)


DEFINITION_CASES = [(40, [(0, 40), (3, 20), (3, 20), (39, 40), (7, 7)], 3, 7, 1), (70, [(0, 64), (1, 66), (63, 70)], 4, M64, 0),
                    (130, [(64, 128), (0, 130)], 2, 2 ** 63 + 5, 1), (9, [(2, 5)], 0, 0, 1)]


def check_definition(a, L, ranges, R, seed, lead):
    """fnn_bootscan_counts against the restatement, against rows of fnn_bootstrap_counts(width, R, seed_w), in slices; repeated
    ranges differ; lead rows are the 0/1 row."""
    starts, ends = rc.as_bounds(ranges)
    P, W = R + lead, len(starts)
    want = ref_counts(L, starts, ends, R, seed, lead)
    got = counts_of(a, L, starts, ends, R, seed, lead)
    assert got.dtype == np.uint16 and got.shape == want.shape and (got == want).all()
    for w in range(W):
        s, e = int(starts[w]), int(ends[w])
        block = got[w * P:(w + 1) * P]
        assert (block[:, :s] == 0).all() and (block[:, e:] == 0).all() and (block.sum(axis=1) == e - s).all()
        if lead:
            assert (block[0, s:e] == 1).all()
        if e > s and R:
            boot = np.zeros((R, e - s), dtype=np.uint16)
            a.check(a.bootstrap_counts(e - s, R, seed_of(seed, w), boot.ctypes.data))
            assert (block[lead:, s:e] == boot).all()
    for first, count in ((0, 0), (0, 1), (1, W * P - 1), (W * P - 1, 1), (P - 1, min(P + 2, W * P - P + 1)), (W * P, 0)):
        assert (counts_of(a, L, starts, ends, R, seed, lead, first=first, count=count) == got[first:first + count]).all()
    for w in range(W):
        for v in range(w):
            if (starts[w], ends[w]) == (starts[v], ends[v]) and ends[w] - starts[w] >= 8 and R:
                assert (got[w * P + lead:(w + 1) * P] != got[v * P + lead:(v + 1) * P]).any()


# ---- one call ---------------------------------------------------------------------------------------------------------------------

def call(a, seq, starts, ends, R, seed, lead=1, model="p", shape=None, states=4, on_saturation="fail", cap=None, lds=None, ld=None, stride=None,
         in_place=False, pad_seed=99):
    """One call through the raw entry (model="tables": the pair-count entry): the alignment's padding holds bytes that would change
    the result if read, the output's padding holds the sentinel.  Returns (view[W P, n, n(, 4, 4)], the whole output, stats)."""
    seq = np.asarray(seq, dtype=np.uint8)
    starts, ends = np.ascontiguousarray(starts, dtype=np.int64), np.ascontiguousarray(ends, dtype=np.int64)
    (n, L), W, tables = seq.shape, starts.shape[0], model == "tables"
    B, cell = W * (R + lead), 16 if tables else 1
    lds, ld = lds or L, ld or n
    stride = stride or cell * n * ld
    s_buf = rc.padded_seq(seq, lds, pad_seed)
    out = np.full(max(B * stride, 1), ISENTINEL, dtype=np.int64) if tables else np.full(max(B * stride, 1), SENTINEL, dtype=np.float64)
    m = None if tables else _capi.dist_model(model, states, on_saturation, cap, shape)
    args = (a, s_buf.ctypes.data, n, L, lds, starts.ctypes.data, ends.ctypes.data, W, R, seed, lead)
    if in_place == "torch":
        import torch
        t = torch.from_numpy(out).to("cuda:0")
        torch.cuda.synchronize()
        st = _capi.run_scan(*args, t.data_ptr(), ld, stride, m, on_device=True, tables=tables)
        out = t.cpu().numpy()
    else:
        try:
            st = _capi.run_scan(*args, out.ctypes.data, ld, stride, m, on_device=bool(in_place), tables=tables)
        except _capi.FnnError as e:
            e.out = out
            raise
    if tables:
        view = np.lib.stride_tricks.as_strided(out, (B, n, n, 4, 4), (8 * stride, 128 * ld, 128, 32, 8)) if B else np.zeros((0, n, n, 4, 4), dtype=np.int64)
    else:
        view = np.lib.stride_tricks.as_strided(out, (B, n, n), (8 * stride, 8 * ld, 8)) if B else np.zeros((0, n, n))
    return view, out, st


def message(e):
    return str(e.value).split(": ", 2)[2]   # (without the status and the entry's name)


def against_counts(a, seq, starts, ends, R, seed, lead=1, model="p", shape=None, **kw):
    """The entry and the counts entry on fnn_bootscan_counts: the same bytes, padding included, or the same failure.  Returns the
    entry's (view, out, stats), or the failure's message."""
    counts = counts_of(a, seq.shape[1], starts, ends, R, seed, lead)
    ckw = {k: v for k, v in kw.items() if k not in ("pad_seed",)}
    if model == "tables":
        ckw = {k: v for k, v in ckw.items() if k in ("lds", "ld", "stride", "in_place")}
    try:
        want = rc.counts_entry(a, seq, counts, model, shape, **ckw)
    except _capi.FnnError as e:
        with pytest.raises(_capi.FnnError) as ei:
            call(a, seq, starts, ends, R, seed, lead, model, shape, **kw)
        assert ei.value.code == e.code and message(ei) == str(e).split(": ", 2)[2], (str(ei.value), str(e))
        if kw.get("in_place") is not True:
            assert (ei.value.out == (ISENTINEL if model == "tables" else SENTINEL)).all()
        return message(ei)
    view, out, st = call(a, seq, starts, ends, R, seed, lead, model, shape, **kw)
    assert out.tobytes() == want.tobytes(), (model, shape, kw)
    return view, out, st


def check_stats(st, W, P, n, L, missing, route="device", host_chunks=0):
    base = st.boot.model.base
    assert base.n_problems == W * P and base.n_pairs == n * (n - 1) // 2 and base.n_sites == L and base.block_threads == 256
    assert base.has_missing == int(missing) and _capi.DRAW_ROUTES[st.boot.draw_route] == route
    assert st.n_windows == W and st.n_host_chunks == host_chunks and st.n_site_blocks_dense == -(-(W * P) // 16) * (-(-L // 64))
    if route == "device" and not host_chunks:
        assert base.digit_passes == 1 and st.boot.t_draw_s >= 0.0


def group_blocks(starts, ends, P, tables=False, chunk=None):
    """n_site_blocks from its definition: per chunk, per window, per column group, per 16 rows: the window's padded span / 64."""
    B, G, total = len(starts) * P, GROUP_ROWS[tables], 0
    chunk = chunk or B
    for b0 in range(0, B, chunk):
        for w in range(b0 // P, (min(b0 + chunk, B) - 1) // P + 1):
            rows = min((w + 1) * P, b0 + chunk, B) - max(w * P, b0)
            span = -(-int(ends[w]) // 64) - int(starts[w]) // 64
            for r in range(0, rows, G):
                total += -(-min(G, rows - r) // 16) * span
    return total


# ---- case 2: the compact planes and the rows' words (driver) and every boundary under the distance entries ----------------------------

PLANE_STARTS, PLANE_WIDTHS = (0, 1, 15, 16, 63, 64, 65), (1, 15, 16, 17, 63, 64, 65, 130)


@functools.lru_cache(maxsize=None)
def plane_case():
    """n = 6, L = 200: every start x width across the 16- and 64-byte boundaries, and a window that ends at L inside the last
    block's padding.  57 windows."""
    seq = dc.random_seq(6, 200, 2101)
    starts, ends = rc.as_bounds([(s, s + w) for s in PLANE_STARTS for w in PLANE_WIDTHS] + [(190, 200)])
    assert ends.max() == 200 and len(starts) == 57
    return seq, starts, ends


def check_planes(a, R=3, lead=1, seed=7):
    """The driver's export: one launch of k_draw_ranges over a whole call and over chunks that begin and end inside windows.  Every
    byte of every compact row against the digit of the counts over [lo, hi), total = width, the largest count."""
    _, starts, ends = plane_case()
    P, W, lpad = R + lead, len(starts), 256
    counts = np.zeros((W * P, lpad), dtype=np.int64)
    counts[:, :200] = counts_of(a, 200, starts, ends, R, seed, lead)
    assert counts.max() <= 127
    for first, count, G in ((0, W * P, 64), (0, W * P, 32), (2, 9, 64), (P * 20 + 3, 2, 32), (W * P - 1, 1, 64)):
        plane = np.full(W * P * lpad, 0x55, dtype=np.int8)
        total = np.full(count, -1, dtype=np.int64)
        most, nbytes = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.int64)
        a.check(a.bootscan_draw_planes(starts.ctypes.data, ends.ctypes.data, W, R, lead, seed, first, count, G, plane.ctypes.data, plane.size,
                                       nbytes.ctypes.data, total.ctypes.data, most.ctypes.data))
        at = 0
        for p in range(first, first + count):
            w = p // P
            lo, hi = int(starts[w]) // 64 * 64, -(-int(ends[w]) // 64) * 64
            assert (plane[at:at + hi - lo].astype(np.int64) == counts[p, lo:hi]).all(), p
            assert total[p - first] == ends[w] - starts[w]
            at += hi - lo
        assert at == int(nbytes[0]) and (plane[at:] == 0x55).all() and int(most[0]) == int(counts[first:first + count].max())


def check_plane_windows(a):
    """The same windows through the distance entries: "p" and the tables take a window of one site."""
    seq, starts, ends = plane_case()
    for model in ("p", "tables"):
        _, _, st = against_counts(a, seq, starts, ends, 3, 7, 1, model)
        check_stats(st, 57, 4, 6, 200, False)
        assert st.n_site_blocks == group_blocks(starts, ends, 4, model == "tables")


# ---- case 3: column groups ----------------------------------------------------------------------------------------------------------

GROUP_P = (1, 3, 16, 17, 64, 65, 66)


@functools.lru_cache(maxsize=None)
def group_case():
    return dc.random_seq(3, 200, 2102), *rc.as_bounds([(3, 93), (70, 200)])


def check_groups(a, P, lead):
    """P = R + lead across one tile of 16 and one group (64 rows; the tables': 32), two windows, in a padded layout pre-filled with
    the sentinel: a row behind a window's last problem leaves no byte anywhere."""
    seq, starts, ends = group_case()
    n = 3
    for model in ("p", "k2p", "tables"):
        cell = 16 if model == "tables" else 1
        _, _, st = against_counts(a, seq, starts, ends, P - lead, 11, lead, model, lds=205, ld=n + 2, stride=cell * n * (n + 2) + 5)
        check_stats(st, 2, P, n, 200, False)
        assert st.n_site_blocks == group_blocks(starts, ends, P, model == "tables")


# ---- case 4: the grid ---------------------------------------------------------------------------------------------------------------

WINDOW_SETS = [[(0, 64), (40, 104), (80, 144), (120, 184), (136, 200)], [(1, 131), (15, 80), (63, 128), (65, 195), (16, 200)],
               [(0, 200), (50, 150), (50, 150), (100, 164)]]
GRID_MODELS, GRID_MODEL_NAMES = rc.GRID_MODELS, rc.GRID_MODEL_NAMES
GRID_R, GRID_SEED = 5, 2 ** 63 + 5


@functools.lru_cache(maxsize=None)
def grid_case(k, missing):
    seq = dc.random_seq(6, 200, 2101, missing=0.02 if missing else 0.0)
    assert bool((seq == MISSING).any()) == missing
    return seq, *rc.as_bounds(WINDOW_SETS[k])


def boot_slice(a, seq, s, e, batch, seed, lead, model, shape):
    """The bootstrap entry on the slice seq[:, s:e]: the whole output."""
    n, L = seq.shape[0], e - s
    part = np.ascontiguousarray(seq[:, s:e])
    if model == "tables":
        counts = np.concatenate([np.ones((lead, L), dtype=np.uint16), _capi.run_bootstrap_counts(a, L, batch - lead, seed)])
        return rc.counts_entry(a, part, counts, "tables")
    out = np.full(batch * n * n, SENTINEL, dtype=np.float64)
    _capi.run_boot(a, part.ctypes.data, n, L, L, batch, seed, lead, out.ctypes.data, n, n * n, _capi.dist_model(model, gamma_shape=shape))
    return out


def check_grid(a, k, missing, model, shape):
    """Against the counts entry on fnn_bootscan_counts (the case has no failing pair: the counts entry itself would fail), and every
    window against the bootstrap entry on its slice with seed_w."""
    seq, starts, ends = grid_case(k, missing)
    P = GRID_R + 1
    got = against_counts(a, seq, starts, ends, GRID_R, GRID_SEED, 1, model, shape)
    assert not isinstance(got, str), got
    _, out, st = got
    check_stats(st, len(starts), P, 6, 200, missing)
    assert st.boot.model.n_recoded == 0 and st.boot.model.n_saturated_problems == 0
    assert st.n_site_blocks == group_blocks(starts, ends, P, model == "tables") and 0 < st.boot.max_count <= 127
    per = out.size // len(starts)
    for w in range(len(starts)):
        want = boot_slice(a, seq, int(starts[w]), int(ends[w]), P, seed_of(GRID_SEED, w), 1, model, shape)
        assert out[w * per:(w + 1) * per].tobytes() == want.tobytes(), w


def check_whole_alignment(a):
    """One window [0, L) with lead = 1 is bootstrap_distances(seq, R, seed_0, lead = 1)."""
    seq = grid_case(0, True)[0]
    for model in ("p", "k2p"):
        _, out, _ = call(a, seq, [0], [200], 9, 5, 1, model)
        assert out.tobytes() == boot_slice(a, seq, 0, 200, 10, seed_of(5, 0), 1, model, None).tobytes()


# ---- case 5: routes -----------------------------------------------------------------------------------------------------------------

def check_routes(a, monkeypatch, model):
    """FNN_DRAW_ROUTE=host and FNN_DIST_FORCE_DIGITS=2 against the device route: all bytes; under forced digits every chunk is the
    host's."""
    seq, starts, ends = grid_case(1, True)
    kw = dict(lds=203, ld=8, stride=(16 if model == "tables" else 1) * 6 * 8 + 3)
    for k in ("FNN_DRAW_ROUTE", "FNN_DIST_FORCE_DIGITS", "FNN_BATCH_CHUNK"):
        monkeypatch.delenv(k, raising=False)
    _, out0, st0 = call(a, seq, starts, ends, 4, 9, 1, model, **kw)
    check_stats(st0, 5, 5, 6, 200, True)
    monkeypatch.setenv("FNN_DRAW_ROUTE", "host")
    _, out1, st1 = call(a, seq, starts, ends, 4, 9, 1, model, **kw)
    monkeypatch.delenv("FNN_DRAW_ROUTE")
    check_stats(st1, 5, 5, 6, 200, True, route="host")
    assert out1.tobytes() == out0.tobytes() and st1.boot.max_count == st0.boot.max_count and st1.boot.t_draw_s == 0.0
    for chunk in (None, "4"):
        if chunk:
            monkeypatch.setenv("FNN_BATCH_CHUNK", chunk)
        monkeypatch.setenv("FNN_DIST_FORCE_DIGITS", "2")
        _, out2, st2 = call(a, seq, starts, ends, 4, 9, 1, model, **kw)
        monkeypatch.delenv("FNN_DIST_FORCE_DIGITS")
        if chunk:
            monkeypatch.delenv("FNN_BATCH_CHUNK")
        chunks = 7 if chunk else 1
        assert st2.boot.model.base.chunks == chunks
        check_stats(st2, 5, 5, 6, 200, True, host_chunks=chunks)
        assert out2.tobytes() == out0.tobytes() and st2.boot.model.base.digit_passes == 2 and st2.boot.max_count == st0.boot.max_count


@functools.lru_cache(maxsize=None)
def limit_case(L):
    return dc.random_seq(2, L, 2103)


def check_limit(a, monkeypatch, above):
    """A window whose padded span is the limit is drawn on the device, one a block wider on the host; both are the counts entry's
    bytes (the second window keeps the call from being one range)."""
    limit = a.bootstrap_draw_max_sites()
    assert limit >= 30000 and limit % 64 == 0
    monkeypatch.delenv("FNN_DRAW_ROUTE", raising=False)
    width = limit + (64 if above else 0)
    seq = limit_case(limit + 200)
    starts, ends = rc.as_bounds([(64, 64 + width - 3), (5, 100)])
    _, _, st = against_counts(a, seq, starts, ends, 1, 7, 1, "p")
    check_stats(st, 2, 2, 2, limit + 200, False, route="host" if above else "device")


def check_forced_device_above_the_limit(a, monkeypatch):
    """FNN_DRAW_ROUTE=device above the limit: FNN_EINVAL before any device use (it holds without a GPU)."""
    limit = a.bootstrap_draw_max_sites()
    monkeypatch.setenv("FNN_DRAW_ROUTE", "device")
    for model in ("p", "tables"):
        with pytest.raises(_capi.FnnError) as ei:
            call(a, np.full((2, limit + 100), ord("A"), dtype=np.uint8), [1, 0], [limit + 2, 10], 1, 7, 1, model)
        assert ei.value.code == -1 and "sites" in str(ei.value) and (ei.value.out == (ISENTINEL if model == "tables" else SENTINEL)).all()
    monkeypatch.delenv("FNN_DRAW_ROUTE")


# ---- case 6: chunks ---------------------------------------------------------------------------------------------------------------

def check_chunking(a, monkeypatch, model, in_place=False):
    """FNN_BATCH_CHUNK=3 at P = 5: chunks begin and end inside windows; padded layout, padding untouched."""
    seq, starts, ends = grid_case(2, True)
    cell = 16 if model == "tables" else 1
    kw = dict(lds=207, ld=9, stride=cell * 6 * 9 + 7, in_place=in_place)
    _, want, st1 = call(a, seq, starts, ends, 4, 3, 1, model, **kw)
    monkeypatch.setenv("FNN_BATCH_CHUNK", "3")
    got = against_counts(a, seq, starts, ends, 4, 3, 1, model, **kw)
    monkeypatch.delenv("FNN_BATCH_CHUNK")
    assert not isinstance(got, str), got
    _, out, st = got
    assert st1.boot.model.base.chunks == 1 and st.boot.model.base.chunks == 7 and out.tobytes() == want.tobytes()
    assert st.n_site_blocks == group_blocks(starts, ends, 5, model == "tables", chunk=3) and st.boot.max_count == st1.boot.max_count
    if model == "tables":
        from dist_pairs_common import assert_counts_padding_untouched
        assert_counts_padding_untouched(out, 20, 6, 9, kw["stride"])
    else:
        dc.assert_padding_untouched(out, 20, 6, 9, kw["stride"])


# ---- case 7: failures ---------------------------------------------------------------------------------------------------------------

def check_empty_window(a, device=True):
    """An empty window below a non-empty one: its first problem is the lowest (b, i, j)."""
    full = dc.random_seq(4, 200, 2104)
    starts, ends = rc.as_bounds([(0, 100), (50, 50), (100, 200), (64, 64)])
    for model, policy in (("p", "fail"), ("k2p", "cap"), ("tn93", "cap")):   # without missing bytes: before any device use
        with pytest.raises(_capi.FnnError) as ei:
            call(a, full, starts, ends, 2, 5, 1, model, on_saturation=policy, cap=3.0 if policy == "cap" else None)
        assert ei.value.code == -1 and "(3, 0, 1)" in str(ei.value) and "valid == 0" in str(ei.value), str(ei.value)
        assert (ei.value.out == SENTINEL).all()
    if not device:
        return
    seq = dc.random_seq(4, 200, 2105, missing=0.02)
    for model in ("p", "jc69", "k2p", "tn93"):
        msg = against_counts(a, seq, starts, ends, 2, 5, 1, model)
        assert isinstance(msg, str) and "(3, 0, 1)" in msg and "valid == 0" in msg, msg
        for env in ("host", None):   # (the host route names the call's problem too)
            if env:
                os.environ["FNN_DRAW_ROUTE"] = env
            try:
                with pytest.raises(_capi.FnnError) as ei:
                    call(a, seq, starts, ends, 2, 5, 1, model)
            finally:
                os.environ.pop("FNN_DRAW_ROUTE", None)
            assert message(ei) == msg
    F, _, _ = against_counts(a, seq, starts, ends, 2, 5, 1, "tables")   # the tables never fail: an empty window is zeros
    assert (F[3:6] == 0).all() and (F[9:12] == 0).all() and F[0].any()


@functools.lru_cache(maxsize=None)
def empty_pair_case():
    """Window 1 = [8, 16): taxon 1 is present at site 8 only, so its pairs are empty in a replicate that never draws site 8.  The
    first seed for which some replicate of window 1 does that, and not its first one, and no row of window 0 is empty."""
    seq = dc.random_seq(3, 24, 2106)
    seq[:, 8] = ord("A")
    seq[1, 9:16] = MISSING
    starts, ends = rc.as_bounds([(0, 8), (8, 16), (16, 24)])
    for seed in range(4000):
        c = ref_counts(24, starts, ends, 6, seed, 1)
        hit = np.flatnonzero(c[7:14, 8] == 0)
        if len(hit) and hit[0] >= 2:
            return seq, starts, ends, seed, 7 + int(hit[0])
    raise AssertionError("no seed found")


def check_empty_pair(a):
    seq, starts, ends, seed, b = empty_pair_case()
    for kw in (dict(model="p"), dict(model="jc69", on_saturation="cap", cap=5.0), dict(model="k2p", on_saturation="cap", cap=5.0)):
        msg = against_counts(a, seq, starts, ends, 6, seed, 1, **kw)
        assert isinstance(msg, str) and f"({b}, 0, 1)" in msg and "valid == 0" in msg, msg


@functools.lru_cache(maxsize=None)
def saturated_case():
    """Window 1 = [8, 16), JC69: taxon 2 differs from the others at five of its eight sites; a replicate that draws them six times or
    more is saturated.  The first seed with some such replicates in window 1, not its first, some without, and none elsewhere."""
    seq = np.full((3, 24), ord("A"), dtype=np.uint8)
    seq[2, 8:13] = ord("C")
    starts, ends = rc.as_bounds([(0, 8), (8, 16), (16, 24)])
    for seed in range(4000):
        c = ref_counts(24, starts, ends, 6, seed, 1)
        sat = c[:, 8:13].sum(axis=1) >= 6
        if 2 <= sat.sum() <= 4 and not sat[8]:
            return seq, starts, ends, seed, int(np.flatnonzero(sat)[0]), int(sat.sum())
    raise AssertionError("no seed found")


def check_saturated(a):
    seq, starts, ends, seed, b, n_sat = saturated_case()
    msg = against_counts(a, seq, starts, ends, 6, seed, 1, "jc69")
    assert isinstance(msg, str) and f"({b}, 0, 2)" in msg and "saturated" in msg, msg
    _, _, st = against_counts(a, seq, starts, ends, 6, seed, 1, "jc69", on_saturation="cap", cap=7.5)
    assert st.boot.model.n_saturated_problems == n_sat


def check_arguments(a, monkeypatch):
    """The argument checks come before any device use: they hold without a GPU.  All four distance entries and the counts."""
    monkeypatch.delenv("FNN_DRAW_ROUTE", raising=False)
    n, L, W, R = 4, 10, 3, 2
    seq = dc.random_seq(n, L, 2107)
    starts, ends = rc.as_bounds([(0, 10), (2, 7), (5, 10)])
    out = np.full(16 * W * (R + 1) * n * n, SENTINEL)
    good = dict(seq=seq.ctypes.data, n=n, L=L, lds=L, starts=starts.ctypes.data, ends=ends.ctypes.data, windows=W, replicates=R, seed=7, lead=1,
                out=out.ctypes.data, ld=n)
    entries = (a.bootscan_distances_f64, a.bootscan_distances_device_f64, a.bootscan_pair_counts_i64, a.bootscan_pair_counts_device_i64)
    keep = []

    def run(entry, m=None, **kw):
        k = dict(good, **kw)
        m = _capi.dist_model() if m is None else m
        return entries[entry](k["seq"], k["n"], k["L"], k["lds"], k["starts"], k["ends"], k["windows"], k["replicates"], k["seed"], k["lead"],
                              _capi.dist_model_ref(m) if m != "null" else None, 0, k["out"], k["ld"], k.get("stride", (1 if entry < 2 else 16) * n * n), None)

    def bounds(ranges):
        s, e = rc.as_bounds(ranges)
        keep.extend([s, e])
        return dict(starts=s.ctypes.data, ends=e.ctypes.data)

    for entry in range(4):
        cell = 1 if entry < 2 else 16
        for bad in (dict(L=0), dict(n=0), dict(n=-3), dict(lds=L - 1), dict(ld=n - 1), dict(stride=cell * n * n - 1), dict(seq=None), dict(starts=None),
                    dict(ends=None), dict(out=None), dict(windows=-1), dict(replicates=-1), dict(lead=2), dict(lead=-1),
                    dict(L=(2 ** 31 + 126) // 127, lds=2 ** 40)):
            assert run(entry, **bad) == -1 and a.last_error(), (entry, bad)
        assert run(entry, lead=2) == -1 and b"lead" in a.last_error()
        for ranges, w in (([(0, 10), (-1, 4), (3, 11)], 1), ([(0, 10), (2, 7), (6, 5)], 2), ([(0, 11), (2, 7), (5, 10)], 0)):
            assert run(entry, **bounds(ranges)) == -1 and b"window %d:" % w in a.last_error(), (entry, ranges, a.last_error())
        assert run(entry, windows=0) == 0 and run(entry, replicates=0, lead=0) == 0
        assert run(entry, windows=0, seq=None, starts=None, ends=None, out=None) == 0
    for entry in range(2):
        assert run(entry, m="null") == -1 and b"NULL model" in a.last_error()
        assert run(entry, m=_capi.dist_model(3)) == -1 and b"unknown model" in a.last_error()
        assert run(entry, m=_capi.dist_model("k2p", on_saturation="cap")) == -1 and run(entry, m=_capi.dist_model("jc69", states=1)) == -1
        assert run(entry, m=_capi.dist_model("p", gamma_shape=0.5)) == -1 and b"gamma" in a.last_error()
        assert run(entry, m=_capi.dist_model("tn93", gamma_shape=float("nan"))) == -1 and b"shape" in a.last_error()
    assert run(2, m="null", windows=0) == 0   # (the table entries ignore the model)
    assert (out == SENTINEL).all()
    # fnn_bootscan_counts
    c = np.full((W * (R + 1), L), 999, dtype=np.uint16)

    def counts(**kw):
        k = dict(good, first=0, count=W * (R + 1), counts=c.ctypes.data)
        k.update(kw)
        return a.bootscan_counts(k["L"], k["starts"], k["ends"], k["windows"], k["replicates"], k["lead"], k["seed"], k["first"], k["count"], k["counts"])

    for bad in (dict(L=0), dict(starts=None), dict(ends=None), dict(counts=None), dict(windows=-1), dict(replicates=-1), dict(lead=2), dict(lead=-1),
                dict(first=-1), dict(count=-1), dict(first=1), dict(count=W * (R + 1) + 1), dict(first=W * (R + 1) + 1, count=0)):
        assert counts(**bad) == -1 and a.last_error(), bad
    assert counts(**bounds([(0, 10), (2, 7), (6, 5)])) == -1 and b"window 2:" in a.last_error()
    assert (c == 999).all() and counts(count=0, counts=None) == 0 and counts(windows=0, count=0, starts=None, ends=None, counts=None) == 0
    assert counts() == 0 and (c == ref_counts(L, starts, ends, R, 7, 1)).all()


STRUCT_C = ('#include <stdio.h>\n#include <stddef.h>\n#include "fastnn.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %d\\n", '
            'sizeof(fnn_scan_stats), offsetof(fnn_scan_stats, boot), offsetof(fnn_scan_stats, n_windows), offsetof(fnn_scan_stats, n_site_blocks), '
            'offsetof(fnn_scan_stats, n_site_blocks_dense), offsetof(fnn_scan_stats, n_host_chunks), offsetof(fnn_scan_stats, reserved), '
            'sizeof(fnn_boot_stats), (int)FASTNN_ABI_VERSION); return 0; }\n')


def check_struct(tmp_path):
    """sizeof and offsets of fnn_scan_stats against the C compiler's; the ABI version stays 2 and fnn_boot_stats its size."""
    src = tmp_path / "scan.c"
    src.write_text(STRUCT_C)
    exe = tmp_path / "scan"
    subprocess.check_call(["gcc", "-I", os.path.join(dc.ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    S = _capi.FnnScanStats
    assert got[:8] == [C.sizeof(S), S.boot.offset, S.n_windows.offset, S.n_site_blocks.offset, S.n_site_blocks_dense.offset, S.n_host_chunks.offset,
                       S.reserved.offset, C.sizeof(_capi.FnnBootStats)]
    assert got[1] == 0 and got[7] == 176 and got[0] == 176 + 64 and got[8] == 2


# ---- case 9: the pipeline's inputs ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pipeline_case():
    """n = 12, L = 384: windows of 128 every 64, R = 5, TN93."""
    return dc.random_seq(12, 384, 2108), 128, 64, 5, 2 ** 40 + 3

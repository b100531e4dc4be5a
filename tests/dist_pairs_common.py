"""Shared by tests/test_dist_pairs_emu.py (CPU driver) and tests/test_dist_pairs.py (the product on the GPU): the reference of
the 4 x 4 tables of state pairs and of F81, F84, TN93 and LogDet on them, and the cases of both suites.

Definitions, restated from include/fastnn.h.  The alignment is recoded as for K2P (A a -> 0, C c -> 1, G g -> 2, T t U u -> 3, 255
stays, every other byte -> 255 and is counted in n_recoded).  For i < j, F[s][t] = sum over sites of counts[b][site] where taxon i
shows s and taxon j shows t; v = sum F, r_s and c_t the row and column sums, n_s = r_s + c_s, mism = v - trace F,
ts1 = F[A][G] + F[G][A], ts2 = F[C][T] + F[T][C], tv = mism - ts1 - ts2, g_s = n_s / (2 v).  Per pair, in this order: v == 0 is
empty (NaN, fails under both policies); mism == 0 is +0.0; degenerate by integer tests (F84, TN93: some n_s == 0; LogDet: some
r_s == 0 or c_s == 0; F81 never); saturated when some y of a ln(1 - y) is not below 1.0 or LogDet's determinant is not above 0.

The reference is exact integers - an int64 einsum of one-hot codes against the counts - and then Python floats that follow
fnn_dist_model.h line by line (`ref_log` restates dist_log as `dist_model_common.ref_log1p` restates dist_log1p).  A Python float
operation is one IEEE operation with one rounding, as every operation of the kernel is: matrices are compared bitwise.  Every
case builder asserts that its reference has no empty, degenerate or saturated pair it did not ask for."""
import ctypes as C
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

import dist_common as dc
import dist_model_common as mc
from dist_common import MISSING, SENTINEL, same_bits
from dist_model_common import INF, NAN, bits, from_bits, ref_log1p
from fastneighbornet_amd import _capi

MODELS = ["f81", "felsenstein84", "tn93", "logdet"]
EMU_SRCS = [os.path.join(dc.EMU_DIR, f) for f in ("fnn_dist_pairs_emu.cpp", "fnn_draw_emu.cpp", "fnn_dist_model_emu.cpp")] + \
    [os.path.join(dc.CSRC, f) for f in ("fnn_dist_pairs.h", "fnn_dist_model.h", "fnn_draw.h")] + dc.EMU_SRCS[1:]
ISENTINEL = -77


def emu_dist_pairs_api():
    """tests/emu/fnn_dist_pairs_emu.cpp as a shared library: the model, bootstrap and table entries (prefix emup_) and
    emup_dist_log."""
    out = os.path.join(dc.EMU_DIR, "build", "libfnn_dist_pairs_emu.so")
    if dc.newer(out, EMU_SRCS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                               "-o", out, EMU_SRCS[0]])
    a = _capi.Api(C.CDLL(out), "emup_", engine=False)
    _capi.bind_dist_model(a)
    _capi.bind_pair_counts(a)
    _capi.bind_boot(a)
    a._fn("dist_log", C.c_double, [C.c_double])
    return a


# ---- the reference: dist_log ---------------------------------------------------------------------------------------

LG = mc.LP   # (fdlibm's log and log1p share the polynomial)
TWO54 = 1.80143985094819840000e+16


def ref_log(x):
    """dist_log of fastneighbornet_amd/csrc/fnn_dist_model.h, line by line."""
    if not (x > 0.0):
        return NAN
    hx = bits(x) >> 32
    if hx >= 0x7ff00000:
        return NAN
    k = 0
    if hx < 0x00100000:
        k = -54
        x = x * TWO54
        hx = bits(x) >> 32
    k += (hx >> 20) - 1023
    hx &= 0x000fffff
    i = (hx + 0x95f64) & 0x100000
    x = from_bits(((hx | (i ^ 0x3ff00000)) << 32) | (bits(x) & 0xffffffff))
    k += i >> 20
    f = x - 1.0
    dk = float(k)
    if (0x000fffff & (2 + hx)) < 3:
        if f == 0.0:
            if k == 0:
                return 0.0
            return dk * mc.LN2_HI + dk * mc.LN2_LO
        R = f * f * (0.5 - 0.33333333333333333 * f)
        if k == 0:
            return f - R
        return dk * mc.LN2_HI - ((R - dk * mc.LN2_LO) - f)
    s = f / (2.0 + f)
    z = s * s
    w = z * z
    t1 = w * (LG[1] + w * (LG[3] + w * LG[5]))
    t2 = z * (LG[0] + w * (LG[2] + w * (LG[4] + w * LG[6])))
    R = t2 + t1
    if ((hx - 0x6147a) | (0x6b851 - hx)) > 0:
        hfsq = 0.5 * f * f
        if k == 0:
            return f - (hfsq - s * (hfsq + R))
        return dk * mc.LN2_HI - ((hfsq - (s * (hfsq + R) + dk * mc.LN2_LO)) - f)
    if k == 0:
        return f - s * (f - R)
    return dk * mc.LN2_HI - ((s * (f - R) - dk * mc.LN2_LO) - f)


# The largest distance of dist_log from math.log over `log_arguments()`, in ulp: deterministic, measured on the CPU driver and
# recorded in DESIGN.md section 18.  The tests allow one more for math.log's own error.
LOG_WORST_ULP_RECORDED = 1


def log_arguments():
    """The arguments section 16 used for log1p, mapped to (0, inf) - u = 1 + x in (0, 1] and 1 / u -, and the arguments at which
    dist_log takes another path with their neighbours: the mantissa (top 20 bits) at sqrt(2) (0x6a09c: x / 2^(k + 1) from there
    on), within 2^-20 of 1 on either side (0xffffe ... 0x00000), at the two ends of the short series' window (0x6147a, 0x6b851),
    for exponents from the subnormals to 2^1023; the smallest and largest doubles."""
    xs = []
    for x in mc.log1p_arguments():
        u = 1.0 + x
        if u > 0.0:
            xs += [u, 1.0 / u]
    for e in (0, 1, 2, 500, 1000, 1021, 1022, 1023, 1024, 1025, 1500, 2046):
        for hm in (0x6a09b, 0x6a09c, 0x6a09d, 0xffffd, 0xffffe, 0xfffff, 0x00000, 0x00001, 0x61479, 0x6147a, 0x6147b, 0x6b850, 0x6b851,
                   0x6b852, 0x80000):
            for lo in (0, 1, 0x80000000, 0xffffffff):
                xs.append(from_bits((((e << 20) | hm) << 32) | lo))
    xs += [from_bits(1), from_bits(0x000fffffffffffff), from_bits(0x0010000000000000), from_bits(0x7fefffffffffffff), 1.0, 2.0, 0.5]
    return [x for x in xs if x > 0.0 and x < INF]


# ---- the reference: tables and models -------------------------------------------------------------------------------

def ref_tables(seq, counts):
    """F int64 (B, n, n, 4, 4) for ALL i, j (the diagonal blocks are not zeroed here), from the definition."""
    codes, _ = mc.recode(seq)
    hot = (codes[:, None, :] == np.arange(4, dtype=np.uint8)[None, :, None]).astype(np.int64)
    return np.einsum("isk,jtk,bk->bijst", hot, hot, np.asarray(counts, dtype=np.int64))


class Table:
    def __init__(self, F):
        self.F = [[int(F[s][t]) for t in range(4)] for s in range(4)]
        self.r = [sum(self.F[s]) for s in range(4)]
        self.c = [sum(self.F[s][t] for s in range(4)) for t in range(4)]
        self.v = sum(self.r)
        self.mism = self.v - sum(self.F[s][s] for s in range(4))
        self.ts1 = self.F[0][2] + self.F[2][0]
        self.ts2 = self.F[1][3] + self.F[3][1]
        self.tv = self.mism - self.ts1 - self.ts2

    def freq(self, s):
        return float(self.r[s] + self.c[s]) / float(2 * self.v)

    def lacks_a_base(self):
        return any(self.r[s] + self.c[s] == 0 for s in range(4))


def ref_f81(t):
    """(kind, D, the arguments y)."""
    gA, gC, gG, gT = (t.freq(s) for s in range(4))
    sq = ((gA * gA + gC * gC) + gG * gG) + gT * gT
    E = 1.0 - sq
    p = float(t.mism) / float(t.v)
    y = p / E
    if not (y < 1.0):
        return "saturated", INF, (y,)
    return "ok", -(E * ref_log1p(-y)), (y,)


def ref_f84(t):
    if t.lacks_a_base():
        return "degenerate", -INF, ()
    gA, gC, gG, gT = (t.freq(s) for s in range(4))
    gR, gY = gA + gG, gC + gT
    ct, ag = gC * gT, gA * gG
    A = ct / gY + ag / gR
    B = ct + ag
    Cc = gR * gY
    A2 = 2.0 * A
    P = float(t.ts1 + t.ts2) / float(t.v)
    Q = float(t.tv) / float(t.v)
    y1 = P / A2 + ((A - B) * Q) / (A2 * Cc)
    y2 = Q / (2.0 * Cc)
    if not (y1 < 1.0) or not (y2 < 1.0):
        return "saturated", INF, (y1, y2)
    return "ok", -(A2 * ref_log1p(-y1)) + (2.0 * ((A - B) - Cc)) * ref_log1p(-y2), (y1, y2)


def ref_tn93(t):
    if t.lacks_a_base():
        return "degenerate", -INF, ()
    gA, gC, gG, gT = (t.freq(s) for s in range(4))
    gR, gY = gA + gG, gC + gT
    k1 = ((2.0 * gA) * gG) / gR
    k2 = ((2.0 * gT) * gC) / gY
    k3 = 2.0 * ((gR * gY - ((gA * gG) * gY) / gR) - ((gT * gC) * gR) / gY)
    P1 = float(t.ts1) / float(t.v)
    P2 = float(t.ts2) / float(t.v)
    Q = float(t.tv) / float(t.v)
    y1 = P1 / k1 + Q / (2.0 * gR)
    y2 = P2 / k2 + Q / (2.0 * gY)
    y3 = Q / (2.0 * (gR * gY))
    if not (y1 < 1.0) or not (y2 < 1.0) or not (y3 < 1.0):
        return "saturated", INF, (y1, y2, y3)
    return "ok", (-(k1 * ref_log1p(-y1)) - k2 * ref_log1p(-y2)) - k3 * ref_log1p(-y3), (y1, y2, y3)


def det3(a, b, c, d, e, f, g, h, i):
    return (a * (e * i - f * h) - b * (d * i - f * g)) + c * (d * h - e * g)


def ref_logdet(t):
    if any(t.r[s] == 0 or t.c[s] == 0 for s in range(4)):
        return "degenerate", -INF, ()
    v = float(t.v)
    m = [float(t.F[k // 4][k % 4]) / v for k in range(16)]
    C0 = det3(m[5], m[6], m[7], m[9], m[10], m[11], m[13], m[14], m[15])
    C1 = det3(m[4], m[6], m[7], m[8], m[10], m[11], m[12], m[14], m[15])
    C2 = det3(m[4], m[5], m[7], m[8], m[9], m[11], m[12], m[13], m[15])
    C3 = det3(m[4], m[5], m[6], m[8], m[9], m[10], m[12], m[13], m[14])
    det = ((m[0] * C0 - m[1] * C1) + m[2] * C2) - m[3] * C3
    if not (det > 0.0):
        return "saturated", INF, (det,)
    ls = 0.0
    for s in range(4):
        ls = ls + (ref_log(float(t.r[s]) / v) + ref_log(float(t.c[s]) / v))
    return "ok", -(0.25 * (ref_log(det) - 0.5 * ls)), (det,)


REF = {"f81": ref_f81, "felsenstein84": ref_f84, "tn93": ref_tn93, "logdet": ref_logdet}


def ref_pair(F, model):
    """(kind, D) of one table, in the order of the tests: empty, no mismatch, degenerate, saturated."""
    t = Table(F)
    if t.v == 0:
        return "empty", NAN
    if t.mism == 0:
        return "ok", 0.0
    kind, D, _ = REF[model](t)
    return kind, D


def ref_model(seq, counts, model):
    """(D, failures): D float64 (B, n, n) with NaN at an empty pair, -inf at a degenerate and +inf at a saturated one, computed on
    the table of i < j; failures = the sorted list of (b, i, j, kind)."""
    F = ref_tables(seq, counts)
    B, n = F.shape[:2]
    D = np.zeros((B, n, n), dtype=np.float64)
    failures = []
    for b in range(B):
        for i in range(n):
            for j in range(i + 1, n):
                kind, d = ref_pair(F[b, i, j], model)
                if kind != "ok":
                    failures.append((b, i, j, kind))
                D[b, i, j] = D[b, j, i] = d
    return D, failures


def ref_clean(seq, counts, model):
    D, failures = ref_model(seq, counts, model)
    assert not failures, f"the case has an empty, degenerate or saturated pair: {failures[:3]}"
    return D


def quick_clean(seq, counts, model):
    """The integer tests alone, vectorised (cheap: for a builder that looks for a seed); the floats decide afterwards."""
    F = ref_tables(seq, counts)
    n = F.shape[1]
    off = np.triu(np.ones((n, n), dtype=bool), 1)[None]
    r, c = F.sum(axis=4), F.sum(axis=3)
    v = r.sum(axis=3)
    mism = v - np.trace(F, axis1=3, axis2=4)
    if ((v == 0) & off).any():
        return False
    lacks = ((r == 0) | (c == 0)).any(axis=3) if model == "logdet" else ((r + c) == 0).any(axis=3)
    if model != "f81" and (lacks & (mism > 0) & off).any():
        return False
    return not ((4 * mism >= 3 * v) & off).any()   # (far from every model's saturation)


# ---- one call -----------------------------------------------------------------------------------------------------

call = mc.call   # the model entries: (D[B, n, n] view, the whole output, stats)


def call_counts(a, seq, counts, lds=None, ldc=None, ld=None, stride=None, in_place=False, pad_seed=99):
    """`dist_common.call` through the table entries: (F[B, n, n, 4, 4] view, the whole int64 output, stats); the output's padding
    holds ISENTINEL."""
    seq, counts = np.asarray(seq, dtype=np.uint8), np.asarray(counts, dtype=np.uint16)
    (n, L), B = seq.shape, counts.shape[0]
    lds, ldc, ld = lds or L, ldc or L, ld or n
    stride = stride or 16 * n * ld
    r = np.random.default_rng(pad_seed)
    s_buf = np.frombuffer(b"ACGT\xff", dtype=np.uint8)[r.integers(0, 5, (n, lds))].copy()
    s_buf[:, :L] = seq
    c_buf = np.full((B, ldc), 999, dtype=np.uint16)
    c_buf[:, :L] = counts
    out = np.full(max(B * stride, 1), ISENTINEL, dtype=np.int64)
    if in_place == "torch":
        import torch
        t = torch.from_numpy(out).to("cuda:0")
        torch.cuda.synchronize()
        st = _capi.run_pair_counts(a, s_buf.ctypes.data, n, L, lds, c_buf.ctypes.data, B, ldc, t.data_ptr(), ld, stride, on_device=True)
        out = t.cpu().numpy()
    else:
        try:
            st = _capi.run_pair_counts(a, s_buf.ctypes.data, n, L, lds, c_buf.ctypes.data, B, ldc, out.ctypes.data, ld, stride, on_device=bool(in_place))
        except _capi.FnnError as e:
            e.out = out
            raise
    view = np.lib.stride_tricks.as_strided(out, (B, n, n, 4, 4), (8 * stride, 128 * ld, 128, 32, 8)) if B else np.zeros((0, n, n, 4, 4), dtype=np.int64)
    return view, out, st


def want_tables(seq, counts):
    """What the table entries write: the definition with zeroed diagonal blocks."""
    F = ref_tables(seq, counts)
    n = F.shape[1]
    F[:, np.arange(n), np.arange(n)] = 0
    return F


def assert_counts_padding_untouched(out, B, n, ld, stride):
    mask = np.ones(out.shape, dtype=bool)
    for b in range(B):
        for i in range(n):
            mask[b * stride + 16 * i * ld: b * stride + 16 * (i * ld + n)] = False
    assert (out[mask] == ISENTINEL).all()


# ---- case 1: the sixteen operands and the lane maps ------------------------------------------------------------------------

def check_counts_lane_maps(a):
    """n = 6, L = 64, B = 16, section 14's prime counts.  Taxon 0 shows code k % 4 and taxon 1 code (k / 4) % 4 at site k: each of
    the 16 cells of the pair (0, 1) is hit once in each lane group of 16 sites, so each entry is one predicted sum of four
    primes; the other taxa shift the pattern.  A swapped cell, a wrong k-order inside a fragment or a wrong replicate column
    changes some entry."""
    n, L, B = 6, 64, 16
    k = np.arange(L)
    code = np.stack([(k + 0 * k) % 4, (k // 4) % 4] + [((k // 4) * j + k * (j + 1) + j) % 4 for j in range(2, n)])
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[code].copy()
    counts = np.array(dc.first_primes(B * L), dtype=np.uint16).reshape(L, B).T.copy()
    for s in range(4):
        for t in range(4):
            hit = np.flatnonzero((code[0] == s) & (code[1] == t))
            assert sorted(hit // 16) == [0, 1, 2, 3]
    F, _, st = call_counts(a, seq, counts)
    for b in range(B):
        for i in range(n):
            for j in range(n):
                for s in range(4):
                    for t in range(4):
                        want = 0 if i == j else sum(int(counts[b, x]) for x in range(L) if code[i, x] == s and code[j, x] == t)
                        assert F[b, i, j, s, t] == want, (b, i, j, s, t, F[b, i, j, s, t], want)
    assert (F == want_tables(seq, counts)).all() and (F == F.transpose(0, 2, 1, 4, 3)).all()
    assert st.base.digit_passes == 2 and st.base.has_missing == 0 and st.base.n_pairs == 15 and st.n_recoded == 0


# ---- case 2: shape edges ---------------------------------------------------------------------------------------------
# dist_model_common.SHAPE_IDS holds n in {2, 5, 17, 33}, L in {1, 63, 64, 65, 130}, B in {1, 15, 16, 17, 33}; k_dist_pairs runs 2
# replicate tiles per wave with one digit plane (B = 33 = 16 * 2 + 1 is among them) and 1 tile with more (B = 17 in the digit
# cases below)

@functools.lru_cache(maxsize=None)
def shape_case(k, model, missing):
    """The first seed from 900 + 40 k on whose alignment is clean under the model (at L = 1 every mismatch saturates or is
    degenerate, every missing byte empties)."""
    n, L, B = dc.SHAPES[k]
    counts = dc.random_counts(B, L, 600 + k)
    for seed in range(900 + 40 * k, 900 + 40 * k + 4000):
        seq = dc.random_seq(n, L, seed, missing=0.05 if missing and L > 1 else 0.0)
        if not quick_clean(seq, counts, model):
            continue
        D, failures = ref_model(seq, counts, model)
        if not failures:
            return seq, counts, D
    raise AssertionError("no clean alignment found")


def check_shape(a, k, model, missing):
    seq, counts, ref = shape_case(k, model, missing)
    D, _, st = call(a, seq, counts, model)
    assert same_bits(D, ref)
    assert st.base.has_missing == int((seq == MISSING).any()) and st.base.digit_passes == 1 and st.base.block_threads == 256
    assert st.n_recoded == 0 and st.n_saturated_problems == 0


def check_shape_counts(a, k, missing):
    seq, counts, _ = shape_case(k, "f81", missing)
    F, _, _ = call_counts(a, seq, counts)
    assert (F == want_tables(seq, counts)).all()


# ---- case 3: digit planes ----------------------------------------------------------------------------------------------
DIGIT_CASES = mc.DIGIT_CASES


@functools.lru_cache(maxsize=None)
def digit_case(cmax, passes, missing):
    """B = 33 with one plane (two replicate tiles per wave: two groups of 32), B = 17 with more (one tile: two groups of 16)."""
    n, L, B = 7, 65, (33 if passes == 1 else 17)
    counts = dc.random_counts(B, L, 701 + cmax, cmax)
    for seed in range(700, 740):
        seq = dc.random_seq(n, L, seed, missing=0.1 if missing else 0.0)
        if quick_clean(seq, counts, "tn93") and not ref_model(seq, counts, "tn93")[1]:
            return seq, counts
    raise AssertionError("no clean alignment found")


def check_digits(a, cmax, passes, missing):
    """TN93 (all models hold the same sixteen accumulator sets per plane; TN93 has the most logarithms) and the tables."""
    seq, counts = digit_case(cmax, passes, missing)
    D, _, st = call(a, seq, counts, "tn93")
    assert st.base.digit_passes == passes and int(counts.max()) == cmax and st.base.has_missing == int(missing)
    assert same_bits(D, ref_clean(seq, counts, "tn93"))
    F, _, st = call_counts(a, seq, counts)
    assert st.base.digit_passes == passes and (F == want_tables(seq, counts)).all()


# ---- prescribed tables ---------------------------------------------------------------------------------------------------

def table_alignment(n, sites_per_cell=None):
    """L = 64: taxon 0 shows s and all other taxa show t at the sites of cell (s, t).  Returns (seq, {cell: its sites})."""
    per = sites_per_cell or {(s, t): 4 for s in range(4) for t in range(4)}
    assert sum(per.values()) == 64
    seq = np.zeros((n, 64), dtype=np.uint8)
    sites, at = {}, 0
    for (s, t), k in sorted(per.items()):
        sites[(s, t)] = list(range(at, at + k))
        seq[0, at:at + k] = b"ACGT"[s]
        seq[1:, at:at + k] = b"ACGT"[t]
        at += k
    return seq, sites


def table_counts(tables, sites):
    """Replicate b spreads tables[b] (4 x 4 integers) over the sites of its cells."""
    counts = np.zeros((len(tables), 64), dtype=np.uint16)
    for b, T in enumerate(tables):
        for s in range(4):
            for t in range(4):
                x = int(T[s][t])
                if (s, t) in sites:
                    counts[b, sites[(s, t)]] = mc.spread(x, len(sites[(s, t)]))
                else:
                    assert x == 0
    return counts


# ---- case 4: unequal frequencies -----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def skewed_case(n):
    """Tables with skewed marginals and their transposes (replicate b + 8 holds the transpose of replicate b's)."""
    r = np.random.default_rng(4100)
    tables = []
    for k in range(8):
        diag = np.array([9000, 2500, 5500, 1200]) * (k + 4) + r.integers(0, 500, 4)
        T = r.integers(20, 900, (4, 4)) * np.array([[1, 1, 5, 1], [2, 1, 1, 7], [3, 1, 1, 1], [1, 4, 2, 1]])
        T[np.arange(4), np.arange(4)] = diag
        tables.append(T)
    tables += [T.T.copy() for T in tables[:8]]
    seq, sites = table_alignment(n)
    counts = table_counts(tables, sites)
    refs = {m: ref_clean(seq, counts, m) for m in MODELS}
    return seq, counts, tables, refs


def check_skewed(a, n):
    seq, counts, tables, refs = skewed_case(n)
    F, _, _ = call_counts(a, seq, counts)
    for b, T in enumerate(tables):
        assert (F[b, 0, 1] == T).all() and (F[b, 1, 0] == T.T).all()
    k2p = mc.ref_clean(seq, counts, "k2p")
    for b in range(len(tables)):
        # the models differ there: a swapped cell or a swapped P1 / P2 shows
        assert len({bits(float(refs[m][b, 0, 1])) for m in ("tn93", "felsenstein84", "f81")} | {bits(float(k2p[b, 0, 1]))}) == 4
    for m in MODELS:
        D, _, st = call(a, seq, counts, m)
        assert same_bits(D, refs[m]) and same_bits(D, D.transpose(0, 2, 1)) and st.base.digit_passes == 3
        if m != "logdet":   # n_s, ts1, ts2 and tv are sums of integers: a table and its transpose give the same bits
            assert same_bits(D[:8], D[8:])


# ---- case 5: dist_log through stored LogDet distances ------------------------------------------------------------------
LOGDET_SITES = {(0, 0): 40, (0, 1): 1, (1, 1): 8, (2, 2): 8, (3, 3): 7}
LOGDET_SITES_NEAR_ONE = {(0, 0): 50, (0, 1): 1, (1, 1): 5, (2, 2): 4, (3, 3): 4}
# r_A / v at which dist_log changes its path (each >= 1/2, so that the other cells hold the rest): the mantissa passes sqrt(2)
# (sqrt(2)/2); both ends of the short series' window (mantissa 1 + 0x6147a / 2^20 and 1 + 0x6b851 / 2^20, halved); 1/2; 3/4
LOGDET_THRESHOLDS = (mc.SQRT_HALF, (1.0 + 0x6147a / 2.0 ** 20) / 2, (1.0 + 0x6b851 / 2.0 ** 20) / 2, 0.5, 0.75)


def logdet_table(num, den):
    """Upper triangular with r_A = num of v = den: the determinant is the product of the diagonal."""
    rest = den - num
    a_, b_ = rest // 3, rest // 3
    T = np.zeros((4, 4), dtype=np.int64)
    T[0, 0], T[0, 1], T[1, 1], T[2, 2], T[3, 3] = num - 1, 1, a_, b_, rest - a_ - b_
    assert T.sum() == den and (np.diag(T) > 0).all()
    return T


@functools.lru_cache(maxsize=None)
def logdet_ratio_case(n):
    """Two calls: the thresholds, and r_A / v within 2^-20 of 1 from below (v - 3 ... v - 6 of more than 3 * 2^20, which takes
    fifty sites for the cell (A, A))."""
    tables = []
    for den in (1800000, 2400000):
        nums = set()
        for t in LOGDET_THRESHOLDS:
            c = int(t * den)
            nums |= {c - 1, c, c + 1, c + 2}
        tables += [logdet_table(num, den) for num in sorted(nums)]
    ratios = [float(T[0].sum()) / float(T.sum()) for T in tables]
    assert 0.5 in ratios
    for t in LOGDET_THRESHOLDS:
        assert any(0 <= x - t < 2e-6 for x in ratios) and any(0 < t - x < 2e-6 for x in ratios), t
    near = [logdet_table(den - k, den) for den in (3200000, 3276000) for k in (3, 4, 5, 6)]
    assert all(0 < 1.0 - float(T[0].sum()) / float(T.sum()) < 2.0 ** -19 for T in near)
    assert any(1.0 - float(T[0].sum()) / float(T.sum()) < 2.0 ** -20 for T in near)
    out = []
    for tabs, per in ((tables, LOGDET_SITES), (near, LOGDET_SITES_NEAR_ONE)):
        seq, sites = table_alignment(n, per)
        counts = table_counts(tabs, sites)
        out.append((seq, counts, ref_clean(seq, counts, "logdet")))
    return out


def check_logdet_ratios(a, n):
    for seq, counts, ref in logdet_ratio_case(n):
        D, _, st = call(a, seq, counts, "logdet")
        assert same_bits(D, ref) and st.base.digit_passes == 3


# ---- case 6: model identities -----------------------------------------------------------------------------------------

def equal_marginal_table(m, v):
    """m mismatches spread evenly over the 12 off-diagonal cells, the rest evenly over the diagonal: every g_s is 1/4."""
    assert m % 12 == 0 and (v - m) % 4 == 0
    T = np.full((4, 4), m // 12, dtype=np.int64)
    T[np.arange(4), np.arange(4)] = (v - m) // 4
    return T


def check_f81_saturates_like_jc69(a):
    """With equal marginals E = 3/4 and F81's y = p / E is JC69's 4 m / (3 v): the two saturate together."""
    mv = [(2988, 4000), (3000, 4000), (3012, 4000), (12, 4000), (2400, 4000), (36, 48), (24, 48), (48, 64)]
    seq, sites = table_alignment(3)
    counts = table_counts([equal_marginal_table(m, v) for m, v in mv], sites)
    ref, failures = ref_model(seq, counts, "f81")
    sat = [b for b, (m, v) in enumerate(mv) if mc.jc69_saturated(4, m, v)]
    assert sat == [1, 2, 5, 7] and sorted({f[0] for f in failures}) == sat and all(f[3] == "saturated" for f in failures)
    D, _, st = call(a, seq, counts, "f81", on_saturation="cap", cap=3.25)
    want = ref.copy()
    want[want == INF] = 3.25
    assert same_bits(D, want) and st.n_saturated_problems == len(sat)
    Dj, _, stj = call(a, seq, counts, "jc69", on_saturation="cap", cap=3.25)
    assert ((D == 3.25) == (Dj == 3.25)).all() and stj.n_saturated_problems == len(sat)


def boot_call(a, seq, batch, seed, lead, model, in_place=False):
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    n, L = seq.shape
    out = np.full(batch * n * n, SENTINEL, dtype=np.float64)
    st = _capi.run_boot(a, seq.ctypes.data, n, L, L, batch, seed, lead, out.ctypes.data, n, n * n, _capi.dist_model(model), on_device=in_place)
    return out.reshape(batch, n, n), st


def check_bootstrap_entry(a, monkeypatch, model):
    """The bootstrap entries take the four models with no entry of their own, drawn on the device and on the host: problem 0 of
    lead = 1 is `counts` of all ones, problem b the replicate b - 1 of the reference's counts."""
    seq = dc.random_seq(9, 130, 4200, missing=0.05)
    counts = np.concatenate([np.ones((1, 130), dtype=np.int64), dc.ref_bootstrap_counts(130, 4, 11)]).astype(np.uint16)
    ref = ref_clean(seq, counts, model)
    ones, _, _ = call(a, seq, counts[:1], model)
    for route in ("device", "host"):
        monkeypatch.setenv("FNN_DRAW_ROUTE", route)
        D, st = boot_call(a, seq, 5, 11, 1, model)
        monkeypatch.delenv("FNN_DRAW_ROUTE")
        assert same_bits(D, ref) and same_bits(D[:1], ones) and _capi.DRAW_ROUTES[st.draw_route] == route
        assert st.model.base.has_missing == 1 and st.model.base.n_problems == 5


# ---- case 7: kinds -------------------------------------------------------------------------------------------------------
ONES = [[1] * 4] * 4
FINE = [[400, 3, 9, 2], [4, 300, 1, 8], [7, 2, 350, 3], [1, 6, 2, 250]]
NO_G = [[400, 3, 0, 2], [4, 300, 0, 8], [0, 0, 0, 0], [1, 6, 0, 250]]                    # neither taxon shows G
ONLY_TV = [[1, 1, 0, 1], [1, 1, 1, 0], [0, 1, 1, 1], [1, 0, 1, 1]]                        # diagonal and transversions: Q = 2/3
AG = [[1, 0, 3, 0], [0, 4, 0, 0], [3, 0, 1, 0], [0, 0, 0, 4]]                             # A <-> G only: P1 = 3/8
CT = [[4, 0, 0, 0], [0, 1, 0, 3], [0, 0, 4, 0], [0, 3, 0, 1]]                             # C <-> T only: P2 = 3/8
TS = [[1, 0, 3, 0], [0, 1, 0, 3], [3, 0, 1, 0], [0, 3, 0, 1]]                             # both transitions: P = 3/4
# (model, table): the arguments y that are not below 1.0 there (LogDet: the determinant that is not above 0)
SATURATED_KINDS = {"f81 y": ("f81", ONES, (0,)), "f84 y1": ("felsenstein84", TS, (0,)), "f84 y2": ("felsenstein84", ONLY_TV, (1,)),
                   "tn93 y1": ("tn93", AG, (0,)), "tn93 y2": ("tn93", CT, (1,)), "tn93 y3": ("tn93", ONLY_TV, (2,)),
                   "logdet det": ("logdet", ONES, (0,))}
CELL_SITES = {(s, t): [4 * s + t] for s in range(4) for t in range(4)}


def kinds_alignment():
    """n = 4, L = 16, site 4 s + t: taxa 0, 1 and 3 show s, taxon 2 shows t.  The pairs (0, 2) and (1, 2) hold the replicate's table
    (its counts), the pair (2, 3) its transpose, the other pairs no mismatch."""
    seq = np.zeros((4, 16), dtype=np.uint8)
    for s in range(4):
        for t in range(4):
            seq[:, 4 * s + t] = b"ACGT"[s]
            seq[2, 4 * s + t] = b"ACGT"[t]
    return seq


def kinds_counts(tables):
    return np.array([[T[s][t] for s in range(4) for t in range(4)] for T in tables], dtype=np.uint16)


def check_saturated_kind(a, kind):
    """B = 5: replicate 3 holds the table that saturates through one logarithm, the others a fine one."""
    model, table, which = SATURATED_KINDS[kind]
    ys = REF[model](Table(table))[2]
    assert REF[model](Table(table))[0] == "saturated"
    if model == "logdet":
        assert not (ys[0] > 0.0)
    else:
        assert [k for k, y in enumerate(ys) if not (y < 1.0)] == list(which), ys
    seq, counts = kinds_alignment(), kinds_counts([FINE, FINE, FINE, table, FINE])
    ref, failures = ref_model(seq, counts, model)
    assert failures == [(3, 0, 2, "saturated"), (3, 1, 2, "saturated"), (3, 2, 3, "saturated")]
    with pytest.raises(_capi.FnnError) as ei:
        call(a, seq, counts, model)
    assert ei.value.code == -1 and "(3, 0, 2)" in str(ei.value) and "saturated" in str(ei.value), str(ei.value)
    assert (ei.value.out == SENTINEL).all()
    D, _, st = call(a, seq, counts, model, on_saturation="cap", cap=7.5)
    want = ref.copy()
    want[want == INF] = 7.5
    assert same_bits(D, want) and (D == 7.5).sum() == 6 and st.n_saturated_problems == 1 and st.base.n_problems == 5


def check_degenerate(a, model):
    """A pair lacking G in both taxa: degenerate under F84, TN93 and LogDet, fine under F81."""
    seq, counts = kinds_alignment(), kinds_counts([FINE, NO_G, FINE, NO_G, FINE])
    ref, failures = ref_model(seq, counts, model)
    if model == "f81":
        assert not failures
        assert same_bits(call(a, seq, counts, model)[0], ref)
        return
    assert failures == [(b, i, j, "degenerate") for b in (1, 3) for i, j in ((0, 2), (1, 2), (2, 3))]
    with pytest.raises(_capi.FnnError) as ei:
        call(a, seq, counts, model)
    assert ei.value.code == -1 and "(1, 0, 2)" in str(ei.value) and "degenerate" in str(ei.value) and "saturated" not in str(ei.value), str(ei.value)
    assert (ei.value.out == SENTINEL).all()
    D, _, st = call(a, seq, counts, model, on_saturation="cap", cap=2.5)
    want = ref.copy()
    want[want == -INF] = 2.5
    assert same_bits(D, want) and (D == 2.5).sum() == 12 and st.n_saturated_problems == 2


KIND_WORDS = {"empty": "valid == 0", "degenerate": "degenerate", "saturated": "saturated"}


def check_kind_order(a, model):
    """An empty, a degenerate and a saturated replicate in each order: the lowest failing (b, i, j) is named with its kind; under
    the cap an empty pair still fails the call, and it alone."""
    sat_table = next(t for m, t, _ in SATURATED_KINDS.values() if m == model)
    special = {"empty": [[0] * 4] * 4, "degenerate": NO_G, "saturated": sat_table}
    seq = kinds_alignment()
    for order in itertools.permutations(special):
        counts = kinds_counts([FINE] + [special[k] for k in order] + [FINE])
        f = ref_model(seq, counts, model)[1]
        first = f[0]
        if model != "f81":
            assert first[0] == 1 and first[3] == order[0]
        with pytest.raises(_capi.FnnError) as ei:
            call(a, seq, counts, model)
        msg = str(ei.value)
        assert ei.value.code == -1 and "(%d, %d, %d)" % first[:3] in msg and KIND_WORDS[first[3]] in msg, (order, msg)
        assert [w for w in KIND_WORDS.values() if w in msg] == [KIND_WORDS[first[3]]]
        assert (ei.value.out == SENTINEL).all()
        b_empty = 1 + order.index("empty")
        with pytest.raises(_capi.FnnError) as ei:
            call(a, seq, counts, model, on_saturation="cap", cap=9.0)
        assert ei.value.code == -1 and f"({b_empty}, 0, 1)" in str(ei.value) and "valid == 0" in str(ei.value), (order, str(ei.value))
        assert (ei.value.out == SENTINEL).all()
    # the tables themselves never fail: an empty pair is sixteen zeros
    counts = kinds_counts([FINE, special["empty"], NO_G, sat_table])
    F, _, _ = call_counts(a, seq, counts)
    assert (F == want_tables(seq, counts)).all() and (F[1] == 0).all() and (F[3, 0, 2] == np.array(sat_table)).all()


# ---- case 8: recoding ------------------------------------------------------------------------------------------------

def check_recoding(a):
    """Lower case, U and the ambiguity letters R, Y, N: the reference on the recoded alignment, n_recoded exact."""
    seq, counts = mc.recoding_case()
    codes, n_recoded = mc.recode(seq)
    assert n_recoded == sum(ch in b"NRY" for ch in seq.tobytes()) > 5
    plain = np.frombuffer(b"ACGT", dtype=np.uint8)[np.minimum(codes, 3)].copy()
    plain[codes == MISSING] = MISSING
    for model in MODELS:
        ref = ref_clean(plain, counts, model)
        D, _, st = call(a, seq, counts, model)
        assert same_bits(D, ref) and st.n_recoded == n_recoded and st.base.has_missing == 1
    F, _, st = call_counts(a, seq, counts)
    assert (F == want_tables(plain, counts)).all() and st.n_recoded == n_recoded and st.base.has_missing == 1
    F2, _, st2 = call_counts(a, plain, counts)
    assert (F2 == F).all() and st2.n_recoded == 0 and st2.base.has_missing == 1


# ---- case 9: arguments, struct and enum ------------------------------------------------------------------------------------

def check_arguments(a):
    """The argument checks come before any device use: they hold without a GPU."""
    n, L, B = 4, 10, 2
    seq, counts = dc.random_seq(n, L, 830), dc.random_counts(B, L, 831)
    out = np.full(16 * B * n * n, SENTINEL)
    good = dict(seq=seq.ctypes.data, n=n, L=L, lds=L, counts=counts.ctypes.data, batch=B, ldc=L, out=out.ctypes.data, ld=n)
    bads = (dict(L=0), dict(n=0), dict(lds=L - 1), dict(ldc=L - 1), dict(ld=n - 1), dict(seq=None), dict(counts=None), dict(out=None),
            dict(batch=-1), dict(L=(2 ** 31 + 126) // 127, lds=2 ** 40, ldc=2 ** 40))

    def rc(in_place, m, **kw):
        k = dict(dict(good, stride=n * n), **kw)
        fn = a.alignment_distances_model_batch_device_f64 if in_place else a.alignment_distances_model_batch_f64
        return fn(k["seq"], k["n"], k["L"], k["lds"], k["counts"], k["batch"], k["ldc"], C.byref(m), 0, k["out"], k["ld"], k["stride"], None)

    def rc_counts(in_place, **kw):
        k = dict(dict(good, stride=16 * n * n), **kw)
        fn = a.alignment_pair_counts_batch_device_i64 if in_place else a.alignment_pair_counts_batch_i64
        return fn(k["seq"], k["n"], k["L"], k["lds"], k["counts"], k["batch"], k["ldc"], 0, k["out"], k["ld"], k["stride"], None)

    M = _capi.dist_model
    for in_place in (False, True):
        for model in MODELS:
            for m in (M(model, on_saturation=2), M(model, on_saturation=-1), M(model, on_saturation="cap"), M(model, on_saturation="cap", cap=0.0),
                      M(model, on_saturation="cap", cap=INF), M(model, on_saturation="cap", cap=NAN)):
                assert rc(in_place, m) == -1 and a.last_error()
            for bad in bads + (dict(stride=n * n - 1),):
                assert rc(in_place, M(model), **bad) == -1, (in_place, model, bad)
            assert rc(in_place, M(model), batch=0) == 0
            assert rc(in_place, M(model), batch=0, seq=None, counts=None, out=None) == 0
        assert rc(in_place, M(3)) == -1 and rc(in_place, M(15)) == -1 and rc(in_place, M(20)) == -1 and rc(in_place, M(100)) == -1 and b"unknown model" in a.last_error()
        for bad in bads + (dict(stride=16 * n * n - 1), dict(stride=n * n)):
            assert rc_counts(in_place, **bad) == -1, (in_place, bad)
            assert a.last_error()
        assert rc_counts(in_place, batch=0) == 0
        assert rc_counts(in_place, batch=0, seq=None, counts=None, out=None) == 0
    assert (out == SENTINEL).all()


def check_p_entries_refuse_the_models(a):
    """The p-only entries keep refusing every other model."""
    n, L, B = 4, 10, 2
    seq, counts = dc.random_seq(n, L, 830), dc.random_counts(B, L, 831)
    out = np.full(B * n * n, SENTINEL)
    for fn in (a.alignment_distances_batch_f64, a.alignment_distances_batch_device_f64):
        for model in (_capi.DIST_F81, _capi.DIST_F84, _capi.DIST_TN93, _capi.DIST_LOGDET, 3, 7, 100):
            assert fn(seq.ctypes.data, n, L, L, counts.ctypes.data, B, L, model, 0, out.ctypes.data, n, n * n, None) == -1
            assert b"unknown model" in a.last_error()
    assert (out == SENTINEL).all()


ENUMS_C = ('#include <stdio.h>\n#include "fastnn.h"\nint main(void) { printf("%d %d %d %d %d %d %d %zu %zu\\n", (int)FNN_DIST_P, (int)FNN_DIST_JC69, '
           '(int)FNN_DIST_K2P, (int)FNN_DIST_F81, (int)FNN_DIST_F84, (int)FNN_DIST_TN93, (int)FNN_DIST_LOGDET, sizeof(fnn_dist_model), '
           'sizeof(fnn_dist_model_stats)); return 0; }\n')


def check_enums(tmp_path):
    src = tmp_path / "enums.c"
    src.write_text(ENUMS_C)
    exe = tmp_path / "enums"
    subprocess.check_call(["gcc", "-I", os.path.join(dc.ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [_capi.DIST_P, _capi.DIST_JC69, _capi.DIST_K2P, _capi.DIST_F81, _capi.DIST_F84, _capi.DIST_TN93, _capi.DIST_LOGDET,
                   C.sizeof(_capi.FnnDistModel), C.sizeof(_capi.FnnDistModelStats)]
    assert got[:7] == [0, 1, 2, 16, 17, 18, 19]
    assert [_capi.DIST_MODELS[m] for m in MODELS] == [16, 17, 18, 19]


# ---- case 10: layout and chunking ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def layout_case():
    seq, counts = dc.layout_case()
    return seq, counts, ref_clean(seq, counts, "tn93"), want_tables(seq, counts)


def check_layout(a, in_place=False):
    seq, counts, ref, tables = layout_case()
    n, B = 7, 7
    for lds, ldc, ld, stride in ((65 + 5, 65 + 3, n + 2, n * (n + 2) + 11), (65, 65 + 1, n, n * n + 1), (65 + 16, 65, n + 1, n * (n + 1))):
        D, out, _ = call(a, seq, counts, "tn93", lds=lds, ldc=ldc, ld=ld, stride=stride, in_place=in_place)
        assert same_bits(D, ref), (lds, ldc, ld, stride)
        dc.assert_padding_untouched(out, B, n, ld, stride)
        F, out, _ = call_counts(a, seq, counts, lds=lds, ldc=ldc, ld=ld, stride=16 * stride + 5, in_place=in_place)
        assert (F == tables).all(), (lds, ldc, ld, stride)
        assert_counts_padding_untouched(out, B, n, ld, 16 * stride + 5)


def check_chunking(a, monkeypatch, in_place=False):
    seq, counts, ref, tables = layout_case()
    monkeypatch.setenv("FNN_BATCH_CHUNK", "3")
    D, out, st = call(a, seq, counts, "tn93", ld=9, stride=70, in_place=in_place)
    F, fout, fst = call_counts(a, seq, counts, ld=9, stride=16 * 70, in_place=in_place)
    monkeypatch.delenv("FNN_BATCH_CHUNK")
    assert st.base.chunks == 3 and same_bits(D, ref) and fst.base.chunks == 3 and (F == tables).all()
    dc.assert_padding_untouched(out, 7, 7, 9, 70)
    assert_counts_padding_untouched(fout, 7, 7, 9, 16 * 70)
    assert call(a, seq, counts, "tn93")[2].base.chunks == 1 and call_counts(a, seq, counts)[2].base.chunks == 1


# ---- case 11: the pipeline's reference matrices ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pipeline_case(model):
    """n = 33, L = 200, B = 20, seed 7: every taxon holds all four bases, and the reference is clean."""
    seq, counts, _ = dc.pipeline_case()
    assert all(set(row.tolist()) == set(b"ACGT") for row in seq)
    D = ref_clean(seq, counts, model)
    D.setflags(write=False)
    return seq, counts, D

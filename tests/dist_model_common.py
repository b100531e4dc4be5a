"""Shared by tests/test_dist_model_emu.py (CPU driver) and tests/test_dist_model.py (the product on the GPU): the reference of
the corrected alignment distances and the cases of both suites.

The reference is exact integers - `dist_common.ref_sums` for mism and valid, an einsum of (code_i ^ code_j) == 2 for the
transitions - and then Python floats: `ref_log1p` restates fnn_dist_model.h's dist_log1p line by line, `ref_jc69` and `ref_k2p`
the two formulas.  A Python float operation is one IEEE operation with one rounding, as every operation of the kernel is, so
matrices are compared bitwise (+0.0 is not -0.0); no tolerance exists or is needed.  Every case builder asserts that its
reference has no empty or saturated pair it did not ask for."""
import ctypes as C
import functools
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import dist_common as dc
from dist_common import MISSING, SENTINEL, same_bits
from fastneighbornet_amd import _capi

EMU_SRCS = [os.path.join(dc.EMU_DIR, "fnn_dist_model_emu.cpp"), os.path.join(dc.CSRC, "fnn_dist_model.h")] + dc.EMU_SRCS[1:]
NAN, INF = float("nan"), float("inf")


def emu_dist_model_api():
    """tests/emu/fnn_dist_model_emu.cpp as a shared library: the model entries and emu_dist_log1p."""
    out = os.path.join(dc.EMU_DIR, "build", "libfnn_dist_model_emu.so")
    if dc.newer(out, EMU_SRCS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                               "-o", out, EMU_SRCS[0]])
    a = _capi.bind_dist_model(_capi.Api(C.CDLL(out), "emu_", engine=False))
    a._fn("dist_log1p", C.c_double, [C.c_double])
    return a


# ---- the reference ----------------------------------------------------------------------------------------------

def bits(x):
    """The 64 bits of a float as a signed integer."""
    return struct.unpack("<q", struct.pack("<d", x))[0]


def from_bits(u):
    return struct.unpack("<d", struct.pack("<Q", u & dc.MASK64))[0]


LN2_HI, LN2_LO = 6.93147180369123816490e-01, 1.90821492927058770002e-10
LP = (6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01, 2.222219843214978396e-01,
      1.818357216161805012e-01, 1.531383769920937332e-01, 1.479819860511658591e-01)
# the arguments at which dist_log1p takes another path, as high words (sign, exponent, 20 mantissa bits) of x or of 1 + x
LOG1P_HIGH_WORDS = {"sqrt2 - 1": 0x3fda827a, "2^-29": 0x3e200000, "2^-54": 0x3c900000, "sqrt2/2 - 1": 0xbfd2bec3, "2^53": 0x43400000,
                    "mantissa sqrt2": 0x6a09e}


def ref_log1p(x):
    """dist_log1p of fastneighbornet_amd/csrc/fnn_dist_model.h, line by line."""
    hx = bits(x) >> 32
    ax = hx & 0x7fffffff
    if not (x > -1.0) or ax >= 0x7ff00000:
        return NAN
    k, hu, f, c = 1, 1, 0.0, 0.0
    if hx < 0x3fda827a:
        if ax < 0x3e200000:
            if ax < 0x3c900000:
                return x
            return x - x * x * 0.5
        if hx > 0 or hx <= 0xbfd2bec3 - (1 << 32):
            k, f, hu = 0, x, 1
    if k != 0:
        if hx < 0x43400000:
            u = 1.0 + x
            hu = bits(u) >> 32
            k = (hu >> 20) - 1023
            c = (1.0 - (u - x)) if k > 0 else (x - (u - 1.0))
            c = c / u
        else:
            u = x
            hu = bits(u) >> 32
            k = (hu >> 20) - 1023
            c = 0.0
        hu &= 0x000fffff
        lo = bits(u) & 0xffffffff
        if hu < 0x6a09e:
            u = from_bits(((hu | 0x3ff00000) << 32) | lo)
        else:
            k += 1
            u = from_bits(((hu | 0x3fe00000) << 32) | lo)
            hu = (0x00100000 - hu) >> 2
        f = u - 1.0
    dk = float(k)
    hfsq = 0.5 * f * f
    if hu == 0:
        if f == 0.0:
            if k == 0:
                return 0.0
            c = c + dk * LN2_LO
            return dk * LN2_HI + c
        R = hfsq * (1.0 - 0.66666666666666666 * f)
        if k == 0:
            return f - R
        return dk * LN2_HI - ((R - (dk * LN2_LO + c)) - f)
    s = f / (2.0 + f)
    z = s * s
    R = z * (LP[0] + z * (LP[1] + z * (LP[2] + z * (LP[3] + z * (LP[4] + z * (LP[5] + z * LP[6]))))))
    if k == 0:
        return f - (hfsq - s * (hfsq + R))
    return dk * LN2_HI - ((hfsq - (s * (hfsq + R) + (dk * LN2_LO + c))) - f)


def ulps_apart(a, b):
    """How many floats lie between a and b, ends included minus one (0: the same value)."""
    def key(x):
        q = bits(x)
        return q if q >= 0 else -(q & 0x7fffffffffffffff)
    return abs(key(a) - key(b))


def jc69_saturated(k, m, v):
    return k * m >= (k - 1) * v


def ref_jc69(k, m, v):
    y = float(k * m) / float((k - 1) * v)
    e = float(k - 1) / float(k)
    return -(e * ref_log1p(-y))


def k2p_saturated(ts, tv, v):
    return 2 * ts + tv >= v or 2 * tv >= v


def ref_k2p(ts, tv, v):
    y1 = float(2 * ts + tv) / float(v)
    y2 = float(2 * tv) / float(v)
    return 0.5 * (-ref_log1p(-y1)) + 0.25 * (-ref_log1p(-y2))


K2P_LUT = np.full(256, MISSING, dtype=np.uint8)
for _ch, _code in zip("AaCcGgTtUu", (0, 0, 1, 1, 2, 2, 3, 3, 3, 3)):
    K2P_LUT[ord(_ch)] = _code


def recode(seq):
    """(the alignment in K2P's codes, the number of bytes that became 255 and were not)."""
    seq = np.asarray(seq, dtype=np.uint8)
    out = K2P_LUT[seq]
    return out, int(((out == MISSING) & (seq != MISSING)).sum())


def ref_ts(codes, counts):
    c = np.asarray(codes, dtype=np.int64)
    present = c != MISSING
    trans = present[:, None, :] & present[None, :, :] & ((c[:, None, :] ^ c[None, :, :]) == 2)
    return np.einsum("ijs,bs->bij", trans.astype(np.int64), np.asarray(counts, dtype=np.int64))


def ref_model(seq, counts, model, states=4):
    """(D, failures): D float64 (B, n, n) with NaN at an empty pair and +inf at a saturated one; failures = the sorted list of
    (b, i, j, "empty" | "saturated"), i < j."""
    seq = np.asarray(seq, dtype=np.uint8)
    if model == "k2p":
        seq, _ = recode(seq)
        ts = ref_ts(seq, counts)
    mism, valid = dc.ref_sums(seq, counts)
    B, n, _ = mism.shape
    D = np.zeros((B, n, n), dtype=np.float64)
    failures = []
    for b in range(B):
        for i in range(n):
            for j in range(i + 1, n):
                m, v = int(mism[b, i, j]), int(valid[b, i, j])
                if v == 0:
                    d = NAN
                    failures.append((b, i, j, "empty"))
                elif m == 0:
                    d = 0.0
                elif model == "jc69":
                    d = INF if jc69_saturated(states, m, v) else ref_jc69(states, m, v)
                else:
                    s = int(ts[b, i, j])
                    d = INF if k2p_saturated(s, m - s, v) else ref_k2p(s, m - s, v)
                if d == INF:
                    failures.append((b, i, j, "saturated"))
                D[b, i, j] = D[b, j, i] = d
    return D, failures


def ref_clean(seq, counts, model, states=4):
    D, failures = ref_model(seq, counts, model, states)
    assert not failures, f"the case has an empty or saturated pair: {failures[:3]}"
    return D


def is_clean(seq, counts, model, states=4):
    """The integer tests alone (cheap: for a builder that looks for a seed)."""
    s = np.asarray(seq, dtype=np.uint8)
    if model == "k2p":
        s, _ = recode(s)
    m, v = dc.ref_sums(s, counts)
    off = ~np.eye(m.shape[1], dtype=bool)[None]
    if ((v == 0) & off).any():
        return False
    if model == "jc69":
        return not (states * m >= (states - 1) * v)[np.broadcast_to(off, m.shape)].any()
    t = ref_ts(s, counts)
    return not (((2 * t + (m - t) >= v) | (2 * (m - t) >= v)) & off).any()


# ---- one call -----------------------------------------------------------------------------------------------------

def call(a, seq, counts, model, states=4, on_saturation="fail", cap=None, lds=None, ldc=None, ld=None, stride=None, in_place=False, pad_seed=99):
    """`dist_common.call` through the model entries: padded inputs whose padding would change the result if read, an output
    whose padding holds SENTINEL.  Returns (D[B, n, n] view, the whole output, stats)."""
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
    m = _capi.dist_model(model, states, on_saturation, cap)
    if in_place == "torch":   # the product's device entry: the output is a tensor on the GPU
        import torch
        t = torch.from_numpy(out).to("cuda:0")
        torch.cuda.synchronize()
        st = _capi.run_dist_model(a, s_buf.ctypes.data, n, L, lds, c_buf.ctypes.data, B, ldc, t.data_ptr(), ld, stride, m, on_device=True)
        out = t.cpu().numpy()
    else:
        try:
            st = _capi.run_dist_model(a, s_buf.ctypes.data, n, L, lds, c_buf.ctypes.data, B, ldc, out.ctypes.data, ld, stride, m, on_device=bool(in_place))
        except _capi.FnnError as e:
            e.out = out
            raise
    view = np.lib.stride_tricks.as_strided(out, (B, n, n), (8 * stride, 8 * ld, 8)) if B else np.zeros((0, n, n))
    return view, out, st


# ---- case 1: dist_log1p alone -----------------------------------------------------------------------------------------

def log1p_arguments():
    xs = [-m / v for v in range(2, 130) for m in range(1, v)]
    for v in (1000, 4096, 10007, 65535, 2 ** 20 + 7, 2 ** 31 - 1, 2 ** 40 - 3):
        xs += [-m / v for m in (1, 2, 3, v // 7, v // 3, int(v * 0.2928), int(v * 0.2930), v // 2, v // 2 + 1, int(v * 0.7071), v - 2, v - 1)]
    for e in range(1, 53):
        xs += [-(2.0 ** -e), -(1.0 - 2.0 ** -e)]
    xs.append(-0.0)
    # the branch thresholds themselves and their neighbours: as arguments (high word of x) ...
    for hw in (0xbe200000, 0xbc900000, 0xbfd2bec3):
        for lo in (0, 1, 0xffffffff):
            xs += [from_bits((hw << 32) | lo), from_bits(((hw - 1) << 32) | lo), from_bits(((hw + 1) << 32) | lo)]
    # ... and as sums u = 1 + x: the mantissa at sqrt(2) (high 20 bits 0x6a09e) and at 1 (|f| < 2^-20), for a few exponents
    for e in (1022, 1021, 1020, 1015, 1000):
        for hm in (0x6a09d, 0x6a09e, 0x6a09f, 0x00000, 0x00001, 0xfffff):
            for lo in (0, 1, 0x80000000, 0xffffffff):
                u = from_bits((((e << 20) | hm) << 32) | lo)
                xs.append(u - 1.0)
    return [x for x in xs if -1.0 < x <= 0.0]


# ---- case 2: transition byte and lane map ------------------------------------------------------------------------------

def check_lane_maps(a, where, model):
    """n = 6, L = 64, B = 16: taxon j differs from all others at one site of its own, by a transition (A -> G) for odd j, by a
    transversion (A -> C) for even j; counts[b][s] distinct primes.  Every ts, tv and distance is one predicted value."""
    n, L, B = 6, 64, 16
    sites = dc.LANE_MAP_SITES[where]
    seq = np.full((n, L), ord("A"), dtype=np.uint8)
    for j in range(n):
        seq[j, sites[j]] = ord("G") if j % 2 else ord("C")
    counts = np.array(dc.first_primes(B * L), dtype=np.uint16).reshape(L, B).T.copy()
    D, _, st = call(a, seq, counts, model)
    tot = counts.astype(np.int64).sum(axis=1)
    for b in range(B):
        for i in range(n):
            for j in range(n):
                if i == j:
                    want = 0.0
                else:
                    ci, cj = int(counts[b, sites[i]]), int(counts[b, sites[j]])
                    ts = (ci if i % 2 else 0) + (cj if j % 2 else 0)
                    want = ref_k2p(ts, ci + cj - ts, int(tot[b])) if model == "k2p" else ref_jc69(4, ci + cj, int(tot[b]))
                assert bits(float(D[b, i, j])) == bits(want), (b, i, j, D[b, i, j], want)
    assert same_bits(D, ref_clean(seq, counts, model))
    assert st.base.digit_passes == 2 and st.base.has_missing == 0 and st.n_recoded == 0 and st.n_saturated_problems == 0


# ---- case 3: prescribed ratios ---------------------------------------------------------------------------------------

def spread(total, k):
    """`total` as k counts of at most 65535 each."""
    out = []
    for _ in range(k):
        out.append(min(total, 65535))
        total -= out[-1]
    assert total == 0
    return out


SQRT_HALF = 0.7071067811865476
# y at which dist_log1p(-y) changes its path and that a ratio of counts over at most 64 sites can reach (v below 2^22): the
# reduction starts (1 - sqrt(2)/2, where the mantissa of 1 - y also passes sqrt(2)); the mantissa of 1 - y passes sqrt(2) again
# (1 - sqrt(2)/4, 1 - sqrt(2)/8); 1 - y is a power of two or within 2^-20 of one from above (1/2, 3/4, 7/8: the short series)
RATIO_THRESHOLDS = (1.0 - SQRT_HALF, 1.0 - SQRT_HALF / 2, 1.0 - SQRT_HALF / 4, 0.5, 0.75, 0.875)


def ratio_targets(den):
    """Numerators num with num / den just below, at and just above every threshold, 1 / den and (den - 1) / den."""
    nums = {1, 2, den - 1, den - 2}
    for t in RATIO_THRESHOLDS:
        c = int(t * den)
        nums |= {c - 1, c, c + 1, c + 2}
    return sorted(x for x in nums if 0 < x < den)


RATIO_SITES = (24, 8, 32)   # sites that differ by a transition, by a transversion, not at all


def feasible(ts, tv, v):
    return all(0 <= x <= 65535 * k for x, k in zip((ts, tv, v - ts - tv), RATIO_SITES)) and ts + tv > 0


@functools.lru_cache(maxsize=None)
def ratio_case(model, n):
    """Taxon 0 against n - 1 equal taxa over L = 64 sites (RATIO_SITES); replicate b spreads its own (ts, tv, valid) over them.
    The small denominators reach every ratio from 1 / v to (v - 1) / v; the large ones (what 64 counts can hold) the
    thresholds only, among them 1/2 - 1/v with 1/v < 2^-21, where 1 - y is within 2^-20 of a power of two."""
    seq = np.full((n, 64), ord("A"), dtype=np.uint8)
    seq[1:, :24] = ord("G")
    seq[1:, 24:32] = ord("C")
    triples = []
    if model == "jc69":   # y = 4 m / (3 v) = m / (3 w) with v = 4 w
        for w in (333334, 700001):
            triples += [(m - min(m // 4, 500000), min(m // 4, 500000), 4 * w) for m in ratio_targets(3 * w)]
    else:
        for v in (1500000, 2500000):     # y1 = x / v with y2 = 2 / v or 4 / v
            triples += [((x - 1) // 2, 1 + (x - 1) % 2, v) for x in ratio_targets(v) if x >= 2]
        for v in (1048000,):             # y2 = x / v with y1 = x / (2 v)
            triples += [(0, x // 2, v) for x in ratio_targets(v) if x % 2 == 0]
        triples += [(0, 1, 1999999), (1, 0, 1999999), (0, 524279, 1048559)]   # 1 / v twice, y2 = (v - 1) / v
    triples = [t for t in triples if feasible(*t)]
    ys = [(2 * ts + tv) / v if model == "k2p" else 4 * (ts + tv) / (3 * v) for ts, tv, v in triples]
    assert min(ys) < 2e-6 and max(ys) > 1 - 2e-6 and any(0 < 0.5 - y < 2.0 ** -21 for y in ys) and 0.5 in ys
    for t in RATIO_THRESHOLDS:
        assert any(0 < y - t < 2e-6 for y in ys) and any(0 < t - y < 2e-6 for y in ys), t
    counts = np.array([sum((spread(x, k) for x, k in zip((ts, tv, v - ts - tv), RATIO_SITES)), []) for ts, tv, v in triples], dtype=np.uint16)
    return seq, counts, ref_clean(seq, counts, model)


def check_ratios(a, model, n):
    seq, counts, ref = ratio_case(model, n)
    D, _, st = call(a, seq, counts, model)
    assert same_bits(D, ref)
    assert st.base.digit_passes == 3 and len(counts) > 30


# ---- case 4: shape edges ---------------------------------------------------------------------------------------------
# a subset of dist_common.SHAPES with every n of {1, 2, 3, 17, 33, 65}, every L of {1, 15, 16, 17, 63, 64, 65, 130}, every B of
# {1, 15, 16, 17, 33}
SHAPE_IDS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 17)


@functools.lru_cache(maxsize=None)
def shape_case(k, model, missing):
    """The first seed from 900 + 40 k on whose alignment has neither an empty nor a saturated pair (at L = 1 every mismatch
    saturates, every missing byte empties)."""
    n, L, B = dc.SHAPES[k]
    counts = dc.random_counts(B, L, 600 + k)
    for seed in range(900 + 40 * k, 900 + 40 * k + 4000):
        seq = dc.random_seq(n, L, seed, missing=0.05 if missing and L > 1 else 0.0)   # (one site: nothing can be missing)
        if is_clean(seq, counts, model):
            return seq, counts, ref_clean(seq, counts, model)
    raise AssertionError("no clean alignment found")


def check_shape(a, k, model, missing):
    seq, counts, ref = shape_case(k, model, missing)
    D, _, st = call(a, seq, counts, model)
    assert same_bits(D, ref)
    assert st.base.has_missing == int((seq == MISSING).any()) and st.base.digit_passes == 1 and st.base.block_threads == 256
    assert st.n_recoded == 0 and st.n_saturated_problems == 0


# ---- case 5: digit planes with three accumulator sets -------------------------------------------------------------------
DIGIT_CASES = [(127, 1), (128, 2), (16384, 3)]


def check_digits(a, cmax, passes, missing):
    """K2P; the variant with three planes and `valid` counted runs two replicate tiles per wave: B = 65 makes three replicate
    groups of 32 there."""
    n, L, B = 7, 65, (65 if passes == 3 and missing else 17)
    seq = dc.random_seq(n, L, 700, missing=0.1 if missing else 0.0)
    counts = dc.random_counts(B, L, 701 + cmax, cmax)
    D, _, st = call(a, seq, counts, "k2p")
    assert st.base.digit_passes == passes and int(counts.max()) == cmax and st.base.has_missing == int(missing)
    assert same_bits(D, ref_clean(seq, counts, "k2p"))


# ---- case 6: recoding ------------------------------------------------------------------------------------------------

def recoding_case():
    rows = ["ACGTACGTacgtuUNRYAcgtACGTTGCAacgu",
            "ACGTACGAacgtUuARYRcgtaACGTTGCAacgt",
            "ACGTACGTACGTTTYNNAcgaACGTTGCTACGT",
            "GCGTACGTacgcuuNNNAcgtACGTAGCAacgt"]
    rows = [r[:32] for r in rows]
    seq = np.frombuffer("".join(rows).encode(), dtype=np.uint8).reshape(4, 32).copy()
    seq[1, 3] = MISSING
    return seq, dc.random_counts(5, 32, 850)


def check_recoding(a):
    """Lower case, U and the ambiguity letters R, Y, N under K2P: the reference on the recoded alignment."""
    seq, counts = recoding_case()
    codes, n_recoded = recode(seq)
    assert n_recoded == sum(ch in b"NRY" for ch in seq.tobytes()) > 5
    # the recoded alignment in letters: upper case, T for U, 255 where an ambiguity letter stood
    plain = np.frombuffer(b"ACGT", dtype=np.uint8)[np.minimum(codes, 3)].copy()
    plain[codes == MISSING] = MISSING
    assert (plain != seq).sum() > 20
    ref = ref_clean(plain, counts, "k2p")
    D, _, st = call(a, seq, counts, "k2p")
    assert same_bits(D, ref)
    assert st.n_recoded == n_recoded and st.base.has_missing == 1
    D2, _, st2 = call(a, plain, counts, "k2p")
    assert same_bits(D2, ref) and st2.n_recoded == 0 and st2.base.has_missing == 1
    # an alignment whose only bytes outside the letters are ambiguity codes takes the counting kernel too
    amb = np.frombuffer(b"ACGT", dtype=np.uint8)[np.minimum(codes, 3)].copy()
    amb[0, 5] = ord("N")
    D3, _, st3 = call(a, amb, counts, "k2p")
    assert st3.n_recoded == 1 and st3.base.has_missing == 1 and same_bits(D3, ref_clean(amb, counts, "k2p"))
    # taxa 1 and 2 share ambiguous sites only: an empty pair, named
    e = seq.copy()
    e[3, 4:8] = np.frombuffer(b"acgu", dtype=np.uint8)   # (so that taxa 1 and 2 share sites with the others)
    e[1, :] = MISSING
    e[2, :] = MISSING
    e[1, 4:8] = np.frombuffer(b"RYNT", dtype=np.uint8)
    e[2, 4:8] = np.frombuffer(b"ACGN", dtype=np.uint8)
    assert ref_model(e, counts, "k2p")[1][0] == (0, 1, 2, "empty")
    with pytest.raises(_capi.FnnError) as ei:
        call(a, e, counts, "k2p")
    assert ei.value.code == -1 and "(0, 1, 2)" in str(ei.value) and "valid == 0" in str(ei.value) and "saturated" not in str(ei.value)
    assert (ei.value.out == SENTINEL).all()


def check_too_many_states(a):
    """JC69 with states = 4 on five letters: FNN_EINVAL before any device use (it holds without a GPU)."""
    seq = dc.random_seq(4, 20, 860)
    seq[2, 7] = ord("N")
    counts = dc.random_counts(2, 20, 861)
    with pytest.raises(_capi.FnnError) as ei:
        call(a, seq, counts, "jc69", states=4)
    assert ei.value.code == -1 and "distinct" in str(ei.value)
    assert (ei.value.out == SENTINEL).all()


# ---- case 7: saturation ----------------------------------------------------------------------------------------------
SATURATION_KINDS = {"jc69": ("jc69", ord("C"), (3, 4), (2999, 4000)),           # 4 * 3 == 3 * 4; 4 * 2999 < 3 * 4000
                    "k2p y1": ("k2p", ord("G"), (2, 4), (1999, 4000)),          # transitions: 2 ts == v; 3998 < 4000
                    "k2p y2": ("k2p", ord("C"), (2, 4), (1999, 4000))}          # transversions: 2 tv == v with y1 = 1/2


def saturation_case(kind, empty_in=None):
    """n = 4, B = 5, L = 3.  Taxon 2 differs from the others at site 0; replicate 3 has the saturated ratio (m, v), the others the
    finite one.  empty_in = b: taxon 3 is present at site 2 only, and replicate b counts that site zero times: its pairs
    (0, 3), (1, 3), (2, 3) are empty there (elsewhere site 2 counts once, inside v)."""
    model, letter, sat, fin = SATURATION_KINDS[kind]
    seq = np.full((4, 3), ord("A"), dtype=np.uint8)
    seq[2, 0] = letter
    if empty_in is not None:
        seq[3, :2] = MISSING
    counts = np.zeros((5, 3), dtype=np.uint16)
    for b in range(5):
        m, v = sat if b == 3 else fin
        c2 = 0 if empty_in is None or empty_in == b else 1
        counts[b] = (m, v - m - c2, c2)
    return model, seq, counts


def check_saturation(a, kind):
    model, seq, counts = saturation_case(kind)
    ref, failures = ref_model(seq, counts, model)
    assert failures == [(3, 0, 2, "saturated"), (3, 1, 2, "saturated"), (3, 2, 3, "saturated")]
    with pytest.raises(_capi.FnnError) as ei:
        call(a, seq, counts, model)
    assert ei.value.code == -1 and "(3, 0, 2)" in str(ei.value) and "saturated" in str(ei.value), str(ei.value)
    assert (ei.value.out == SENTINEL).all()
    D, _, st = call(a, seq, counts, model, on_saturation="cap", cap=7.5)
    want = ref.copy()
    want[want == INF] = 7.5
    assert same_bits(D, want) and (D == 7.5).sum() == 6
    assert st.n_saturated_problems == 1 and st.base.n_problems == 5


def check_saturation_order(a, kind):
    """The lowest (b, i, j) is named, empty or saturated; an empty pair fails the call under both policies."""
    for empty_in, named, what in ((1, "(1, 0, 3)", "valid == 0"), (4, "(3, 0, 2)", "saturated"), (3, "(3, 0, 2)", "saturated")):
        model, seq, counts = saturation_case(kind, empty_in)
        f = ref_model(seq, counts, model)[1]
        assert f[0][:3] == tuple(int(x) for x in named.strip("()").split(", ")) and (f[0][3] == "saturated") == (what == "saturated")
        with pytest.raises(_capi.FnnError) as ei:
            call(a, seq, counts, model)
        assert ei.value.code == -1 and named in str(ei.value) and what in str(ei.value), (empty_in, str(ei.value))
        assert ("saturated" in str(ei.value)) == (what == "saturated")
        assert (ei.value.out == SENTINEL).all()
        with pytest.raises(_capi.FnnError) as ei:
            call(a, seq, counts, model, on_saturation="cap", cap=9.0)
        assert ei.value.code == -1 and f"({empty_in}, 0, 3)" in str(ei.value) and "valid == 0" in str(ei.value), (empty_in, str(ei.value))
        assert (ei.value.out == SENTINEL).all()
    # without a missing byte `valid` is the replicate's total: an empty replicate above the saturated one is named second
    model, seq, counts = saturation_case(kind)
    counts[4, :] = 0
    with pytest.raises(_capi.FnnError) as ei:
        call(a, seq, counts, model)
    assert "(3, 0, 2)" in str(ei.value) and "saturated" in str(ei.value)
    with pytest.raises(_capi.FnnError) as ei:
        call(a, seq, counts, model, on_saturation="cap", cap=9.0)
    assert "(4, 0, 1)" in str(ei.value) and "valid == 0" in str(ei.value)
    counts[1, :] = 0
    with pytest.raises(_capi.FnnError) as ei:
        call(a, seq, counts, model)
    assert "(1, 0, 1)" in str(ei.value) and "valid == 0" in str(ei.value)


# ---- case 8: old and new entry ---------------------------------------------------------------------------------------

def check_p_equals_old_entry(new, old, in_place=False):
    """FNN_DIST_P through the model entries: the bytes of the old entries, padding included, on the layout case."""
    seq, counts = dc.layout_case()
    for lds, ldc, ld, stride in ((70, 68, 9, 74), (65, 66, 7, 50)):
        D0, out0, st0 = dc.call(old, seq, counts, lds=lds, ldc=ldc, ld=ld, stride=stride, in_place=in_place)
        D1, out1, st1 = call(new, seq, counts, "p", lds=lds, ldc=ldc, ld=ld, stride=stride, in_place=in_place)
        assert out0.tobytes() == out1.tobytes() and same_bits(D1, dc.ref_dist(seq, counts))
        assert (st0.digit_passes, st0.has_missing, st0.chunks, st0.n_pairs) == (st1.base.digit_passes, st1.base.has_missing, st1.base.chunks, st1.base.n_pairs)
        assert st1.n_recoded == 0 and st1.n_saturated_problems == 0


def check_arguments(a):
    """The argument checks come before any device use: they hold without a GPU."""
    n, L, B = 4, 10, 2
    seq, counts = dc.random_seq(n, L, 830), dc.random_counts(B, L, 831)
    out = np.full(B * n * n, SENTINEL)
    good = dict(seq=seq.ctypes.data, n=n, L=L, lds=L, counts=counts.ctypes.data, batch=B, ldc=L, out=out.ctypes.data, ld=n, stride=n * n)

    def rc(in_place, m, **kw):
        k = dict(good, **kw)
        fn = a.alignment_distances_model_batch_device_f64 if in_place else a.alignment_distances_model_batch_f64
        return fn(k["seq"], k["n"], k["L"], k["lds"], k["counts"], k["batch"], k["ldc"], C.byref(m) if m is not None else None, 0, k["out"],
                  k["ld"], k["stride"], None)

    M = _capi.dist_model
    five = seq.copy()
    five[1, 1] = ord("N")
    for in_place in (False, True):
        for m in (None, M(3), M(-1), M("jc69", on_saturation=2), M("k2p", on_saturation=-1), M("p", on_saturation=5),
                  M("jc69", states=1), M("jc69", states=0), M("jc69", states=256), M("jc69", states=-4),
                  M("jc69", on_saturation="cap", cap=0.0), M("k2p", on_saturation="cap", cap=-1.0), M("k2p", on_saturation="cap", cap=INF),
                  M("jc69", on_saturation="cap", cap=NAN), M("k2p", on_saturation="cap")):
            assert rc(in_place, m) == -1, (in_place, m and (m.model, m.states, m.on_saturation, m.cap))
            assert a.last_error()
        assert rc(in_place, M("jc69", states=4), seq=five.ctypes.data) == -1 and b"distinct" in a.last_error()
        assert rc(in_place, M("jc69", states=3)) == -1 and b"distinct" in a.last_error()
        for model in ("p", "jc69", "k2p"):
            for bad in (dict(L=0), dict(n=0), dict(lds=L - 1), dict(ldc=L - 1), dict(ld=n - 1), dict(stride=n * n - 1), dict(seq=None),
                        dict(counts=None), dict(out=None), dict(batch=-1), dict(L=(2 ** 31 + 126) // 127, lds=2 ** 40, ldc=2 ** 40)):
                assert rc(in_place, M(model), **bad) == -1, (in_place, model, bad)
            assert rc(in_place, M(model), batch=0) == 0
            assert rc(in_place, M(model), batch=0, seq=None, counts=None, out=None) == 0
    assert (out == SENTINEL).all()


STRUCT_SIZES_C = ('#include <stdio.h>\n#include <stddef.h>\n#include "fastnn.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %d %d %d %d\\n", '
                  'sizeof(fnn_dist_model), sizeof(fnn_dist_model_stats), offsetof(fnn_dist_model, cap), offsetof(fnn_dist_model_stats, n_recoded), '
                  'sizeof(fnn_dist_stats), (int)FNN_DIST_JC69, (int)FNN_DIST_K2P, (int)FNN_DIST_SAT_FAIL, (int)FNN_DIST_SAT_CAP); return 0; }\n')


def check_struct_sizes(tmp_path):
    src = tmp_path / "size.c"
    src.write_text(STRUCT_SIZES_C)
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(dc.ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    base = C.sizeof(_capi.FnnDistStats)
    assert got == [C.sizeof(_capi.FnnDistModel), C.sizeof(_capi.FnnDistModelStats), _capi.FnnDistModel.cap.offset,
                   _capi.FnnDistModelStats.n_recoded.offset, base, _capi.DIST_JC69, _capi.DIST_K2P, _capi.DIST_SAT_FAIL, _capi.DIST_SAT_CAP]
    assert got[:5] == [24, base + 32, 16, base, 96]


# ---- case 9: layout and chunking for K2P -------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def layout_case():
    seq, counts = dc.layout_case()
    return seq, counts, ref_clean(seq, counts, "k2p")


def check_layout(a, in_place=False):
    seq, counts, ref = layout_case()
    n, B = 7, 7
    for lds, ldc, ld, stride in ((65 + 5, 65 + 3, n + 2, n * (n + 2) + 11), (65, 65 + 1, n, n * n + 1), (65 + 16, 65, n + 1, n * (n + 1))):
        D, out, _ = call(a, seq, counts, "k2p", lds=lds, ldc=ldc, ld=ld, stride=stride, in_place=in_place)
        assert same_bits(D, ref), (lds, ldc, ld, stride)
        dc.assert_padding_untouched(out, B, n, ld, stride)


def check_chunking(a, monkeypatch, in_place=False):
    seq, counts, ref = layout_case()
    monkeypatch.setenv("FNN_BATCH_CHUNK", "3")
    D, out, st = call(a, seq, counts, "k2p", ld=9, stride=70, in_place=in_place)
    monkeypatch.delenv("FNN_BATCH_CHUNK")
    assert st.base.chunks == 3 and same_bits(D, ref)
    dc.assert_padding_untouched(out, 7, 7, 9, 70)
    assert call(a, seq, counts, "k2p")[2].base.chunks == 1


# ---- case 11: the pipeline's reference matrices ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pipeline_case(model):
    seq, counts, _ = dc.pipeline_case()
    D = ref_clean(seq, counts, model)
    D.setflags(write=False)
    return seq, counts, D

"""Shared by tests/test_dist_gamma_emu.py (CPU driver) and tests/test_dist_gamma.py (the product on the GPU): the reference of the
corrected alignment distances with gamma-distributed rates and the cases of both suites.

Definitions, restated from include/fastnn.h.  For a shape alpha > 0, with log1p' and expm1' the library's own,
    g(y):  l = log1p'(-y);  t = (-l) / alpha;  e = expm1'(t);  g = alpha * e
and in the sequences of JC69, K2P, F81, F84 and TN93 every log1p'(-y) becomes -g(y); nothing else changes.  The order of the
per-pair tests is the equal-rates one (empty, mism == 0 gives +0.0, degenerate, saturated), and a pair is also saturated when some
e is not finite (`not (e < inf)`).

The reference is exact integers - `dist_common.ref_sums`, `dist_model_common.ref_ts` and the int64 einsum
`dist_pairs_common.ref_tables` - and then Python floats: `ref_expm1` restates fnn_dist_model.h's dist_expm1 line by line beside
`dist_model_common.ref_log1p`, and the five sequences are restated below.  A Python float operation is one IEEE operation with one
rounding, as every operation of the kernel is: matrices are compared bitwise.  Every case builder asserts that its reference has no
empty, degenerate or saturated pair it did not ask for."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import dist_common as dc
import dist_model_common as mc
import dist_pairs_common as pc
from dist_common import MISSING, SENTINEL, same_bits
from dist_model_common import INF, NAN, bits, from_bits, ref_log1p
from fastneighbornet_amd import _capi

MODELS = ["jc69", "k2p", "f81", "felsenstein84", "tn93"]   # the models with a gamma form
SHAPES = [0.05, 0.5, 1.0, 4.0]                             # alpha
EMU_SRCS = [os.path.join(dc.EMU_DIR, "fnn_dist_gamma_emu.cpp")] + pc.EMU_SRCS


def emu_dist_gamma_api():
    """tests/emu/fnn_dist_gamma_emu.cpp as a shared library: the model and bootstrap entries (prefix emug_) and emug_dist_expm1."""
    out = os.path.join(dc.EMU_DIR, "build", "libfnn_dist_gamma_emu.so")
    if dc.newer(out, EMU_SRCS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                               "-o", out, EMU_SRCS[0]])
    a = _capi.Api(C.CDLL(out), "emug_", engine=False)
    _capi.bind_dist_model(a)
    _capi.bind_boot(a)
    a._fn("dist_expm1", C.c_double, [C.c_double])
    return a


# ---- the reference: dist_expm1 --------------------------------------------------------------------------------------

LN2_HI, LN2_LO, INVLN2 = mc.LN2_HI, mc.LN2_LO, 1.44269504088896338700e+00
O_THRESHOLD = 7.09782712893383973096e+02
Q1, Q2, Q3, Q4, Q5 = (-3.33333333333331316428e-02, 1.58730158725481460165e-03, -7.93650757867487942473e-05, 4.00821782732936239552e-06,
                      -2.01099218183624371326e-07)
TWO1023 = from_bits(0x7fe0000000000000)


def add_to_exponent(y, k):
    """k added to the exponent bits of y (the 64 bits as an unsigned integer, wrapping)."""
    return from_bits((bits(y) + (k << 52)) & dc.MASK64)


def ref_expm1(x, path=None):
    """dist_expm1 of fastneighbornet_amd/csrc/fnn_dist_model.h, line by line.  path: a list that receives the name of the branch
    that produced the value."""
    def took(name):
        if path is not None:
            path.append(name)
    bx = bits(x) & dc.MASK64
    neg = (bx >> 63) != 0
    hx = (bx >> 32) & 0x7fffffff
    if hx >= 0x4043687a:
        if hx >= 0x40862e42:
            if hx >= 0x7ff00000:
                took("non-finite")
                if ((hx & 0x000fffff) | (bx & 0xffffffff)) != 0:
                    return x + x
                return -1.0 if neg else x
            if x > O_THRESHOLD:
                took("overflow")
                return INF
        if neg:
            took("minus one")
            return -1.0
    k, c = 0, 0.0
    if hx > 0x3fd62e42:
        if hx < 0x3ff0a2b2:
            if not neg:
                hi, lo, k = x - LN2_HI, LN2_LO, 1
            else:
                hi, lo, k = x + LN2_HI, -LN2_LO, -1
        else:
            k = int(INVLN2 * x + (-0.5 if neg else 0.5))   # (int() truncates, as the conversion does)
            t = float(k)
            hi = x - t * LN2_HI
            lo = t * LN2_LO
        x = hi - lo
        c = (hi - x) - lo
    elif hx < 0x3c900000:
        took("tiny")
        return x
    hfx = 0.5 * x
    hxs = x * hfx
    r1 = 1.0 + hxs * (Q1 + hxs * (Q2 + hxs * (Q3 + hxs * (Q4 + hxs * Q5))))
    t = 3.0 - r1 * hfx
    e = hxs * ((r1 - t) / (6.0 - x * t))
    if k == 0:
        took("k = 0")
        return x - (x * e - hxs)
    e = x * (e - c) - c
    e = e - hxs
    if k == -1:
        took("k = -1")
        return 0.5 * (x - e) - 0.5
    if k == 1:
        if x < -0.25:
            took("k = 1, r < -1/4")
            return -2.0 * (e - (x + 0.5))
        took("k = 1")
        return 1.0 + 2.0 * (x - e)
    if k <= -2 or k > 56:
        y = 1.0 - (e - x)
        if k == 1024:
            took("k = 1024")
            y = (y * 2.0) * TWO1023
        else:
            took("k <= -2" if k < 0 else "k > 56")
            y = add_to_exponent(y, k)
        return y - 1.0
    if k < 20:
        took("k < 20")
        t = from_bits((0x3ff00000 - (0x00200000 >> k)) << 32)
        y = t - (e - x)
        return add_to_exponent(y, k)
    took("20 <= k <= 56")
    t = from_bits((0x3ff - k) << 52)
    y = x - (e + t)
    y = y + 1.0
    return add_to_exponent(y, k)


LN2 = math.log(2.0)
# |x| at which dist_expm1 takes another path.  The tests on the high word (exponent and 20 mantissa bits) change at the first double
# with the next high word: |x| < 2^-54 returns x; k = +-1 directly from just above 0.5 ln 2 (high word 0x3fd62e42) to just below
# 1.5 ln 2 (0x3ff0a2b2; the general reduction still finds k = 1 up to 1.5 ln 2 itself), and for k = 1 the reduced argument passes -1/4
# near ln 2 - 1/4; k = (int)(x / ln 2 +- 0.5) reaches 2 near 1.5 ln 2, 20 near 19.5 ln 2, 57 near 56.5 ln 2 and 1024 near 1023.5 ln 2;
# x at or below -56 ln 2 (0x4043687a) is -1; x above 709.78... is +inf
EXPM1_THRESHOLDS = {"2^-54": 2.0 ** -54, "0.5 ln 2": from_bits(0x3fd62e43 << 32), "ln 2 - 1/4": LN2 - 0.25, "1.5 ln 2 (high word)": from_bits(0x3ff0a2b2 << 32),
                    "1.5 ln 2": 1.5 * LN2, "19.5 ln 2": 19.5 * LN2, "56 ln 2": from_bits(0x4043687a << 32), "56.5 ln 2": 56.5 * LN2,
                    "1023.5 ln 2": 1023.5 * LN2, "overflow": O_THRESHOLD}
# where a positive argument's value comes from the same reconstruction on both sides (the reduction changes, or only negative ones part)
EXPM1_SAME_PATH = ("1.5 ln 2 (high word)", "56 ln 2")
# the largest distance of dist_expm1 from math.expm1 over `expm1_arguments()`, in ulp: deterministic, measured on the CPU driver and
# recorded in DESIGN.md section 19.  The bound of the tests is 2: fdlibm's stated < 1 ulp and one for math.expm1 itself.
EXPM1_WORST_ULP_RECORDED = 1
EXPM1_BOUND_ULP = 2


def math_expm1(x):
    try:
        return math.expm1(x)
    except OverflowError:
        return INF


@functools.lru_cache(maxsize=None)
def expm1_arguments():
    """40 neighbours on either side of every threshold, of 0.5 ln 2 and 56 ln 2 themselves and of 1/4, 20 ln 2 and 57 ln 2,
    in both signs, and 20000 random arguments of both signs from 2^-60 to 2^9.5."""
    xs = []
    for c in list(EXPM1_THRESHOLDS.values()) + [0.5 * LN2, 56.0 * LN2, 0.25, 20.0 * LN2, 57.0 * LN2]:
        for s in (-1.0, 1.0):
            for toward in (0.0, s * INF):
                x = s * c
                for _ in range(41):
                    xs.append(x)
                    x = math.nextafter(x, toward)
    r = np.random.default_rng(1900)
    e = r.uniform(-60.0, 9.5, 20000)
    m = r.uniform(1.0, 2.0, 20000)
    s = r.choice((-1.0, 1.0), 20000)
    xs += [float(v) for v in s * 2.0 ** e * m]
    xs += [0.0, -0.0, 1.0, -1.0, 2.0 ** -1074, -2.0 ** -1074, 709.0, 710.0, -745.0, 1e308, -1e308]
    return tuple(xs)


def check_expm1(a):
    """The driver's export against the restatement, bit for bit, and against math.expm1 within EXPM1_BOUND_ULP; every path of the
    function is taken.  Returns the largest distance seen."""
    xs = expm1_arguments()
    assert len(xs) > 21500
    worst, paths = 0, set()
    for x in xs:
        p = []
        got, want = a.dist_expm1(x), ref_expm1(x, p)
        assert bits(got) == bits(want), (x, got, want)
        paths.add(p[0])
        d = mc.ulps_apart(got, math_expm1(x))
        assert d <= EXPM1_BOUND_ULP, (x, got, math_expm1(x), d)
        worst = max(worst, d)
    assert paths == {"overflow", "minus one", "tiny", "k = 0", "k = -1", "k = 1, r < -1/4", "k = 1", "k = 1024", "k <= -2", "k > 56", "k < 20",
                     "20 <= k <= 56"}, paths
    for x, want in ((NAN, NAN), (INF, INF), (-INF, -1.0), (0.0, 0.0), (-0.0, -0.0), (from_bits(0x7ff0000000000001), NAN)):
        got = a.dist_expm1(x)
        assert bits(got) == bits(ref_expm1(x)) and (math.isnan(got) if want != want else bits(got) == bits(want)), (x, got)
    return worst


# ---- the reference: the five sequences ----------------------------------------------------------------------------------

class Over(Exception):
    """Some e of the pair is not finite."""


def rate_log(y, shape):
    """What stands where the equal-rates sequences have log1p'(-y) (dist_rate_log): that logarithm with shape None, else -g(y)."""
    l = ref_log1p(-y)
    if shape is None:
        return l
    t = (-l) / shape
    e = ref_expm1(t)
    if not (e < INF):
        raise Over
    g = shape * e
    return -g


def gamma_t(y, shape):
    """The argument of expm1' for y."""
    return (-ref_log1p(-y)) / shape


def ref_jc69(k, m, v, shape):
    y = float(k * m) / float((k - 1) * v)
    e = float(k - 1) / float(k)
    return -(e * rate_log(y, shape))


def ref_k2p(ts, tv, v, shape):
    y1 = float(2 * ts + tv) / float(v)
    y2 = float(2 * tv) / float(v)
    a = 0.5 * (-rate_log(y1, shape))
    b = 0.25 * (-rate_log(y2, shape))
    return a + b


def ref_f81(t, shape):
    gA, gC, gG, gT = (t.freq(s) for s in range(4))
    sq = ((gA * gA + gC * gC) + gG * gG) + gT * gT
    E = 1.0 - sq
    p = float(t.mism) / float(t.v)
    y = p / E
    if not (y < 1.0):
        return "saturated", INF
    return "ok", -(E * rate_log(y, shape))


def ref_f84(t, shape):
    if t.lacks_a_base():
        return "degenerate", -INF
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
        return "saturated", INF
    return "ok", -(A2 * rate_log(y1, shape)) + (2.0 * ((A - B) - Cc)) * rate_log(y2, shape)


def ref_tn93(t, shape):
    if t.lacks_a_base():
        return "degenerate", -INF
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
        return "saturated", INF
    return "ok", (-(k1 * rate_log(y1, shape)) - k2 * rate_log(y2, shape)) - k3 * rate_log(y3, shape)


REF_TABLE = {"f81": ref_f81, "felsenstein84": ref_f84, "tn93": ref_tn93}


def ref_model(seq, counts, model, shape, states=4):
    """(D, failures): D float64 (B, n, n) with NaN at an empty pair, -inf at a degenerate and +inf at a saturated one (the pair
    models on the table of i < j); failures = the sorted list of (b, i, j, kind).  shape=None: equal rates."""
    seq = np.asarray(seq, dtype=np.uint8)
    on_table = model in REF_TABLE
    if on_table:
        F = pc.ref_tables(seq, counts)
        B, n = F.shape[:2]
    else:
        if model == "k2p":
            seq, _ = mc.recode(seq)
            ts = mc.ref_ts(seq, counts)
        mism, valid = dc.ref_sums(seq, counts)
        B, n, _ = mism.shape
    D = np.zeros((B, n, n), dtype=np.float64)
    failures = []
    for b in range(B):
        for i in range(n):
            for j in range(i + 1, n):
                kind = "ok"
                try:
                    if on_table:
                        t = pc.Table(F[b, i, j])
                        if t.v == 0:
                            kind, d = "empty", NAN
                        elif t.mism == 0:
                            d = 0.0
                        else:
                            kind, d = REF_TABLE[model](t, shape)
                    else:
                        m, v = int(mism[b, i, j]), int(valid[b, i, j])
                        if v == 0:
                            kind, d = "empty", NAN
                        elif m == 0:
                            d = 0.0
                        elif model == "jc69":
                            kind, d = ("saturated", INF) if mc.jc69_saturated(states, m, v) else ("ok", ref_jc69(states, m, v, shape))
                        else:
                            s = int(ts[b, i, j])
                            kind, d = ("saturated", INF) if mc.k2p_saturated(s, m - s, v) else ("ok", ref_k2p(s, m - s, v, shape))
                except Over:
                    kind, d = "saturated", INF
                if kind != "ok":
                    failures.append((b, i, j, kind))
                D[b, i, j] = D[b, j, i] = d
    return D, failures


def ref_clean(seq, counts, model, shape, states=4):
    D, failures = ref_model(seq, counts, model, shape, states)
    assert not failures, f"the case has an empty, degenerate or saturated pair: {failures[:3]}"
    return D


def check_reference_of_equal_rates():
    """shape=None restates the references of dist_model_common and dist_pairs_common."""
    seq, counts = dc.random_seq(5, 64, 1901, missing=0.05), dc.random_counts(4, 64, 1902)
    for model in MODELS:
        old = (pc.ref_model if model in REF_TABLE else mc.ref_model)(seq, counts, model)
        new = ref_model(seq, counts, model, None)
        assert same_bits(old[0], new[0]) and old[1] == new[1] == []


# ---- one call -----------------------------------------------------------------------------------------------------

def call(a, seq, counts, model, shape, states=4, on_saturation="fail", cap=None, lds=None, ldc=None, ld=None, stride=None, in_place=False,
         pad_seed=99, m=None):
    """`dist_model_common.call` with a shape: padded inputs whose padding would change the result if read, an output whose padding
    holds SENTINEL.  m: the model struct itself, in place of the names.  Returns (D[B, n, n] view, the whole output, stats)."""
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
    if m is None:
        m = _capi.dist_model(model, states, on_saturation, cap, shape)
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


# ---- case 2: dist_expm1 through stored JC69 distances --------------------------------------------------------------------
# Taxon 0 against taxon 1 over L = 64 sites, 24 of which differ; replicate b spreads its own (m, v) over them.  For the pair of
# replicate 0, l = log1p'(-y) is fixed, and alpha = (-l) / target with its neighbours puts t = (-l) / alpha on either side of
# `target`; the other replicates see the same alpha at other t.
THRESHOLD_MV = ((1000, 4000), (1, 4000), (2999, 4000), (1500, 4000))
THRESHOLD_CAP = 6.25


@functools.lru_cache(maxsize=None)
def threshold_alignment():
    seq = np.full((2, 64), ord("A"), dtype=np.uint8)
    seq[1, :24] = ord("C")
    counts = np.array([mc.spread(m, 24) + mc.spread(v - m, 40) for m, v in THRESHOLD_MV], dtype=np.uint16)
    return seq, counts


@functools.lru_cache(maxsize=None)
def threshold_case(name):
    """([(alpha, reference with the cap in place of +inf, saturated replicates)] for 9 neighbouring alpha around (-l) / target, the
    paths of dist_expm1 that replicate 0 takes there)."""
    target = EXPM1_THRESHOLDS[name]
    seq, counts = threshold_alignment()
    m, v = THRESHOLD_MV[0]
    y = float(4 * m) / float(3 * v)
    mid = (-ref_log1p(-y)) / target
    alphas = [mid]
    for toward in (0.0, INF):
        x = mid
        for _ in range(4):
            x = math.nextafter(x, toward)
            alphas.append(x)
    ts = [gamma_t(y, al) for al in alphas]
    assert any(t < target for t in ts) and any(t > target for t in ts) and all(abs(t - target) <= 16 * math.ulp(target) for t in ts), (name, ts)
    paths = set()
    for t in ts:
        p = []
        ref_expm1(t, p)
        paths.add(p[0])
    assert len(paths) == (1 if name in EXPM1_SAME_PATH else 2), (name, paths)   # the two sides take different paths
    out = []
    for al in alphas:
        D, failures = ref_model(seq, counts, "jc69", al)
        assert all(f[3] == "saturated" for f in failures)
        if name != "overflow":
            assert 0 not in {f[0] for f in failures}
        D[D == INF] = THRESHOLD_CAP
        out.append((al, D, sorted({f[0] for f in failures})))
    if name == "overflow":
        assert {0 in s for _, _, s in out} == {True, False}
    return out, paths


def check_threshold(a, name):
    seq, counts = threshold_alignment()
    cases, _ = threshold_case(name)
    for al, ref, saturated in cases:
        D, _, st = call(a, seq, counts, "jc69", al, on_saturation="cap", cap=THRESHOLD_CAP)
        assert same_bits(D, ref), (name, al)
        assert st.n_saturated_problems == len(saturated) and st.base.digit_passes == 2


def check_thresholds_reach_every_positive_path():
    """The stored-distance cases take every path of dist_expm1 that a positive argument can."""
    paths = set()
    for name in EXPM1_THRESHOLDS:
        paths |= threshold_case(name)[1]
    assert paths == {"overflow", "tiny", "k = 0", "k = 1, r < -1/4", "k = 1", "k = 1024", "k > 56", "k < 20", "20 <= k <= 56"}, paths


# ---- case 3: every model at the shapes of the kernels ------------------------------------------------------------------------
# n = 2 (one tile, mostly padding), 5 and 6; L = 64 (one step of the site loop); B = 16 (one replicate tile), 17 and 33 (one more
# than one and than two tiles: k_dist_pairs runs 2 tiles per wave with one digit plane)
GRID_SHAPES = [(2, 64, 16), (5, 64, 17), (6, 64, 33)]
GRID_NAMES = ["n%d-L%d-B%d" % s for s in GRID_SHAPES]


@functools.lru_cache(maxsize=None)
def grid_case(k, model, missing):
    """The first seed from 1910 + 40 k on whose alignment is clean under the model with equal rates and with every shape of SHAPES:
    (seq, counts, {alpha: reference})."""
    n, L, B = GRID_SHAPES[k]
    counts = dc.random_counts(B, L, 1905 + k)
    for seed in range(1910 + 40 * k, 1910 + 40 * k + 400):
        seq = dc.random_seq(n, L, seed, missing=0.05 if missing else 0.0)
        if missing and not (seq == MISSING).any():
            continue
        if ref_model(seq, counts, model, None)[1]:
            continue
        refs = {al: ref_model(seq, counts, model, al) for al in SHAPES}
        if not any(f for _, f in refs.values()):
            return seq, counts, {al: D for al, (D, _) in refs.items()}
    raise AssertionError("no clean alignment found")


def check_grid(a, k, model, missing, shape):
    seq, counts, refs = grid_case(k, model, missing)
    D, _, st = call(a, seq, counts, model, shape)
    assert same_bits(D, refs[shape])
    assert not same_bits(D, ref_model(seq, counts, model, None)[0])   # (the shape is read)
    assert st.base.has_missing == int(missing) and st.base.digit_passes == 1 and st.base.block_threads == 256
    assert st.n_recoded == 0 and st.n_saturated_problems == 0


DIGIT_CASES = mc.DIGIT_CASES   # (largest count, digit planes): (127, 1), (128, 2), (16384, 3)


@functools.lru_cache(maxsize=None)
def digit_case(cmax, passes, missing):
    """n = 7, L = 65; B = 65 for K2P's variant with three planes and `valid` counted (two replicate tiles per wave: three groups of
    32), else B = 33 with one plane and 17 with more (k_dist_pairs: two tiles, then one)."""
    n, L = 7, 65
    for seed in range(1950, 1990):
        seq = dc.random_seq(n, L, seed, missing=0.1 if missing else 0.0)
        big = dc.random_counts(65, L, 1951 + cmax, cmax)
        if all(not ref_model(seq, big, m, al)[1] for m in ("k2p", "tn93") for al in (None, 0.5)):
            return seq, big
    raise AssertionError("no clean alignment found")


def check_digits(a, model, cmax, passes, missing):
    seq, big = digit_case(cmax, passes, missing)
    B = 65 if (model == "k2p" and passes == 3 and missing) else (33 if passes == 1 else 17)
    counts = big[:B].copy()
    counts[0, 0] = cmax
    D, _, st = call(a, seq, counts, model, 0.5)
    assert st.base.digit_passes == passes and int(counts.max()) == cmax and st.base.has_missing == int(missing)
    assert same_bits(D, ref_clean(seq, counts, model, 0.5))


# ---- case 4: overflow ---------------------------------------------------------------------------------------------------------
HOT = [[100, 30, 60, 30], [30, 100, 30, 60], [60, 30, 100, 30], [30, 60, 30, 100]]
OVERFLOW_SHAPE = 0.001


def check_overflow(a, model):
    """n = 4, B = 5 (dist_pairs_common.kinds_alignment): replicate 3 holds a divergent table, the others a fine one.  Every pair is
    finite with equal rates and at alpha = 0.5; at alpha = 0.001 the divergent pairs' t passes 709.78... and they alone are
    saturated: named under FAIL, capped and counted under CAP."""
    seq, counts = pc.kinds_alignment(), pc.kinds_counts([pc.FINE, pc.FINE, pc.FINE, HOT, pc.FINE])
    assert not ref_model(seq, counts, model, None)[1] and not ref_model(seq, counts, model, 0.5)[1]
    ref, failures = ref_model(seq, counts, model, OVERFLOW_SHAPE)
    assert failures == [(3, 0, 2, "saturated"), (3, 1, 2, "saturated"), (3, 2, 3, "saturated")]
    with pytest.raises(_capi.FnnError) as ei:
        call(a, seq, counts, model, OVERFLOW_SHAPE)
    assert ei.value.code == -1 and "(3, 0, 2)" in str(ei.value) and "saturated" in str(ei.value), str(ei.value)
    assert (ei.value.out == SENTINEL).all()
    D, _, st = call(a, seq, counts, model, OVERFLOW_SHAPE, on_saturation="cap", cap=7.5)
    want = ref.copy()
    want[want == INF] = 7.5
    assert same_bits(D, want) and (D == 7.5).sum() == 6 and st.n_saturated_problems == 1 and st.base.n_problems == 5
    assert same_bits(call(a, seq, counts, model, 0.5)[0], ref_clean(seq, counts, model, 0.5))


# ---- case 5: equal rates through the new struct ----------------------------------------------------------------------------

def check_equal_rates_through_the_struct(a, in_place=False):
    """FNN_DIST_RATES_EQUAL in a fnn_dist_model_rates: the bytes of a plain fnn_dist_model, padding included; nothing behind
    `base` is read (the shape and the reserved words hold what would be refused)."""
    seq, counts = dc.layout_case()
    for model in ("p", "jc69", "k2p", "tn93", "logdet"):
        mr = _capi.FnnDistModelRates()
        mr.base = _capi.dist_model(model)
        mr.shape = NAN
        mr.reserved[1] = 3.0
        assert mr.base.reserved == _capi.DIST_RATES_EQUAL
        D0, out0, st0 = mc.call(a, seq, counts, model, lds=70, ldc=68, ld=9, stride=74, in_place=in_place)
        D1, out1, st1 = call(a, seq, counts, model, None, lds=70, ldc=68, ld=9, stride=74, in_place=in_place, m=mr)
        assert out0.tobytes() == out1.tobytes() and st0.base.digit_passes == st1.base.digit_passes
        want = dc.ref_dist(seq, counts) if model == "p" else (pc.ref_clean(seq, counts, model) if model in pc.MODELS else mc.ref_clean(seq, counts, model))
        assert same_bits(D1, want)


# ---- case 6: both draw routes ------------------------------------------------------------------------------------------------

def boot_call(a, seq, batch, seed, lead, m, in_place=False):
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    n, L = seq.shape
    out = np.full(batch * n * n, SENTINEL, dtype=np.float64)
    st = _capi.run_boot(a, seq.ctypes.data, n, L, L, batch, seed, lead, out.ctypes.data, n, n * n, m, on_device=in_place)
    return out.reshape(batch, n, n), st


def check_bootstrap_entry(a, monkeypatch, model):
    """The bootstrap entries with a shape, drawn on the device and on the host: problem 0 of lead = 1 is `counts` of all ones,
    problem b the replicate b - 1 of the reference's counts; the counts entry writes the same bytes."""
    seq = dc.random_seq(9, 130, 4200, missing=0.05)
    counts = np.concatenate([np.ones((1, 130), dtype=np.int64), dc.ref_bootstrap_counts(130, 4, 11)]).astype(np.uint16)
    ref = ref_clean(seq, counts, model, 0.5)
    by_counts, _, _ = call(a, seq, counts, model, 0.5)
    assert same_bits(by_counts, ref)
    for route in ("device", "host"):
        monkeypatch.setenv("FNN_DRAW_ROUTE", route)
        D, st = boot_call(a, seq, 5, 11, 1, _capi.dist_model(model, gamma_shape=0.5))
        monkeypatch.delenv("FNN_DRAW_ROUTE")
        assert same_bits(D, ref) and _capi.DRAW_ROUTES[st.draw_route] == route
        assert st.model.base.has_missing == 1 and st.model.base.n_problems == 5


# ---- case 7: arguments and the struct ----------------------------------------------------------------------------------------

def rates(model, shape, rates=_capi.DIST_RATES_GAMMA, reserved=(0.0, 0.0, 0.0), **kw):
    mr = _capi.FnnDistModelRates()
    mr.base = _capi.dist_model(model, **kw)
    mr.base.reserved = rates
    mr.shape = shape
    for k in range(3):
        mr.reserved[k] = reserved[k]
    return mr


def check_arguments(a):
    """The argument checks come before any device use: they hold without a GPU.  All four entries that take a fnn_dist_model."""
    n, L, B = 4, 10, 2
    seq, counts = dc.random_seq(n, L, 830), dc.random_counts(B, L, 831)
    out = np.full(B * n * n, SENTINEL)

    def rc(entry, m, batch=B):
        ref = _capi.dist_model_ref(m)
        if entry < 2:
            fn = a.alignment_distances_model_batch_device_f64 if entry else a.alignment_distances_model_batch_f64
            return fn(seq.ctypes.data, n, L, L, counts.ctypes.data, batch, L, ref, 0, out.ctypes.data, n, n * n, None)
        fn = a.bootstrap_distances_batch_device_f64 if entry == 3 else a.bootstrap_distances_batch_f64
        return fn(seq.ctypes.data, n, L, L, batch, 5, 0, ref, 0, out.ctypes.data, n, n * n, None)

    for entry in range(4):
        for model in MODELS:
            for shape in (0.0, -0.0, -1.0, INF, -INF, NAN):
                assert rc(entry, rates(model, shape)) == -1 and b"shape" in a.last_error(), (entry, model, shape, a.last_error())
            for k in range(3):
                res = [0.0, 0.0, 0.0]
                res[k] = 1.0
                assert rc(entry, rates(model, 0.5, reserved=res)) == -1 and b"reserved" in a.last_error(), (entry, model, k)
            assert rc(entry, rates(model, 0.5, reserved=(0.0, NAN, 0.0))) == -1 and b"reserved" in a.last_error()
            for bad in (2, -1, 7):
                assert rc(entry, rates(model, 0.5, rates=bad)) == -1 and b"rates" in a.last_error(), (entry, model, bad)
            # the other checks of the model still hold beside a good shape
            assert rc(entry, rates(model, 0.5, on_saturation=2)) == -1 and rc(entry, rates(model, 0.5, on_saturation="cap")) == -1
            # nothing to do: FNN_OK after the checks, and the checks still come first
            assert rc(entry, rates(model, 0.5), batch=0) == 0
            assert rc(entry, rates(model, NAN), batch=0) == -1 and b"shape" in a.last_error()
        for model in ("p", "logdet"):
            assert rc(entry, rates(model, 0.5)) == -1 and b"gamma" in a.last_error(), (entry, model, a.last_error())
            assert rc(entry, rates(model, 0.5, rates=2)) == -1 and b"rates" in a.last_error()
        assert rc(entry, rates("jc69", 0.5, states=1)) == -1 and rc(entry, rates(3, 0.5)) == -1 and b"unknown model" in a.last_error()
    assert (out == SENTINEL).all()


STRUCT_C = ('#include <stdio.h>\n#include <stddef.h>\n#include "fastnn.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %d %d %d\\n", '
            'sizeof(fnn_dist_model_rates), offsetof(fnn_dist_model_rates, base), offsetof(fnn_dist_model_rates, shape), '
            'offsetof(fnn_dist_model_rates, reserved), sizeof(fnn_dist_model), offsetof(fnn_dist_model, reserved), '
            '(int)FNN_DIST_RATES_EQUAL, (int)FNN_DIST_RATES_GAMMA, (int)sizeof(double)); return 0; }\n')


def check_struct(tmp_path):
    """sizeof and offsets of fnn_dist_model_rates against the C compiler's; fnn_dist_model keeps its 24 bytes."""
    src = tmp_path / "rates.c"
    src.write_text(STRUCT_C)
    exe = tmp_path / "rates"
    subprocess.check_call(["gcc", "-I", os.path.join(dc.ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    R = _capi.FnnDistModelRates
    assert got[:8] == [C.sizeof(R), R.base.offset, R.shape.offset, R.reserved.offset, C.sizeof(_capi.FnnDistModel), _capi.FnnDistModel.reserved.offset,
                       _capi.DIST_RATES_EQUAL, _capi.DIST_RATES_GAMMA]
    assert got[:8] == [56, 0, 24, 32, 24, 12, 0, 1]


# ---- case 8: layout and chunking ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def layout_case(model):
    seq, counts = dc.layout_case()   # n = 7, L = 65, B = 7
    return seq, counts, ref_clean(seq, counts, model, 0.5)


def check_chunking(a, monkeypatch, model, in_place=False):
    """FNN_BATCH_CHUNK=3 at B = 7: three chunks, each with the shape; padded layout, padding untouched."""
    seq, counts, ref = layout_case(model)
    monkeypatch.setenv("FNN_BATCH_CHUNK", "3")
    D, out, st = call(a, seq, counts, model, 0.5, lds=70, ldc=68, ld=9, stride=70, in_place=in_place)
    monkeypatch.delenv("FNN_BATCH_CHUNK")
    assert st.base.chunks == 3 and same_bits(D, ref)
    dc.assert_padding_untouched(out, 7, 7, 9, 70)
    assert call(a, seq, counts, model, 0.5)[2].base.chunks == 1


# ---- case 9: the pipeline's reference matrices ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pipeline_case(model, shape):
    """n = 33, L = 200, B = 20, seed 7 (dist_common.pipeline_case)."""
    seq, counts, _ = dc.pipeline_case()
    D = ref_clean(seq, counts, model, shape)
    D.setflags(write=False)
    return seq, counts, D

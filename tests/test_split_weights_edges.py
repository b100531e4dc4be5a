"""Circular split weights at the edges: fnn_split_weights_f64 (csrc/fnn_splits.hip) at scale, on degenerate input classes, on
forced solver paths and at the corners of its ABI.

CPU part (-m "not gpu"): the certificate every GPU assertion rests on (common.kkt_violation) is pinned against a dense
long-double evaluation and shown to have teeth; the expectations about tree metrics, duplicated taxa, constant matrices and
the distance of the CPU oracle to the optimum are confirmed with the CPU references before a GPU test relies on them.
GPU part: power-of-two scalings (bit for bit), the exact tie classes of tests/inputs.py, every knob that block_active_set()
reads (with the counters that prove the path ran), tiny n, foreign orderings, a padded row stride, constant and non-finite
input."""
import ctypes as C

import numpy as np
import pytest

import inputs
from common import kkt_violation, live_to_fast
from oracle import csw_oracle as W

COUNTERS = ("outer_iterations", "entered", "departed", "screened_out", "refactorizations")

# The CPU oracle (the reference's conjugate-gradient method, CG_EPSILON = 1e-8) stops short of the optimum.  On the outgroup
# class (three pendant weights near 1e6) its distance to scipy's dense NNLS optimum at 48 taxa, seed 13, relative to max(w):
# measured 1.322e-07 (0.132 absolute); test_cpu_outgroup_oracle_distance_to_the_optimum pins it.  The GPU comparison at 300
# taxa gets ten times that (the factor absorbs the growth of the CG stopping error with n).
ORACLE_OUTGROUP_REL = 1.33e-7


# ---------------------------------------------------------------------------------------------------------------- helpers
_nnls_cache = {}


def nnls(D, order, key=None):
    """Dense NNLS optimum of the live design matrix (scipy's Lawson-Hanson); computed once per `key`, never modified."""
    import scipy.optimize as so
    if key is not None and key in _nnls_cache:
        return _nnls_cache[key]
    xs, _ = so.nnls(W.live_design_matrix(D.shape[0], order), W.packed_distances(D), maxiter=10 ** 7)
    xs.setflags(write=False)
    if key is not None:
        _nnls_cache[key] = xs
    return xs


def random_order(n, seed):
    """A valid ordering that is not the Neighbor-Net one: ordering[0] = 0, then a random permutation of 1..n."""
    rng = np.random.default_rng(seed)
    while True:
        p = rng.permutation(n)
        if (p != np.arange(n)).any():                  # (tiny n: the draw may be the identity)
            return np.concatenate([[0], 1 + p]).astype(np.int32)


def identity_order(n):
    return np.arange(n + 1, dtype=np.int32)


def residual(D, order, live):
    """max |A w - d| with the oracle's prefix-sum operator, and max |d|."""
    n = D.shape[0]
    d = W.setup_d(D, order)
    return float(np.abs(W.calculate_ab(n, live_to_fast(n, live)) - d).max()), float(np.abs(d).max())


def duplicate_groups(D):
    """Group id per taxon: taxa at distance zero from each other are copies of one taxon (inputs.make: dup)."""
    n = D.shape[0]
    g = -np.ones(n, dtype=np.int64)
    c = 0
    for a in range(n):
        if g[a] < 0:
            g[(D[a] == 0.0) & (g < 0)] = c
            c += 1
    return g


def separates_copies(order, g):
    """Per split in live index order ((i, j), i < j, row-major: taxa ordering[i+1 .. j]): does it have copies of one taxon on both sides?"""
    n = len(g)
    gp = g[np.asarray(order[1:]) - 1]                 # group per cycle position; split (i, j) = positions i .. j-1
    iu = np.triu_indices(n, 1)
    sep = np.zeros(len(iu[0]), dtype=bool)
    for c in np.unique(gp):
        cnt = np.concatenate([[0], np.cumsum(gp == c)])
        inside = cnt[iu[1]] - cnt[iu[0]]
        sep |= (inside > 0) & (inside < cnt[-1])
    return sep


def trivial_split_indices(n):
    """Live indices of the n trivial splits: (i, i+1) = {ordering[i+1]} for i = 0 .. n-2, and (0, n-1) = all but ordering[n]."""
    k = lambda i, j: (2 * n - i - 1) * i // 2 + (j - i - 1)
    return sorted({k(i, i + 1) for i in range(n - 1)} | {k(0, n - 1)})


def constant_expected(n):
    e = np.zeros(W.npairs(n))
    e[trivial_split_indices(n)] = 0.5
    return e


def dense_violation(D, order, x):
    """common.kkt_violation restated with the dense live design matrix in long double: (max -x, max |g| on x > 0, max -g on x <= 0)
    with g = A^T (A x - d), the last two relative to max |A^T d|."""
    A = W.live_design_matrix(D.shape[0], order).astype(np.longdouble)
    d = W.packed_distances(D).astype(np.longdouble)
    xl = np.asarray(x, dtype=np.longdouble)
    g = A.T @ (A @ xl - d)
    scale = np.abs(A.T @ d).max()
    pos = xl > 0
    return (float(-xl.min()), float(np.abs(g[pos]).max(initial=0.0) / scale), float((-g[~pos]).max(initial=0.0) / scale))


def certify(D, order, w, st, what):
    """The solver's own certificate and the solver-independent one on the host (scale-free)."""
    assert st["certified"] == 1, (what, st)
    v = kkt_violation(D, order, w)
    assert v < 1e-9, (what, v, st)
    return v


# ---------------------------------------------------------------------------------------------------------------- 1. the certificate (CPU)
@pytest.mark.parametrize("n,seed", [(5, 1), (12, 2), (33, 3), (48, 4)])
def test_cpu_certificate_matches_a_dense_long_double_evaluation_and_has_teeth(oracle, n, seed):
    D = oracle.synth(n, seed)
    order = oracle.run(D)[0]
    xs = np.array(nnls(D, order, ("uniform53", n, seed)))
    pos = np.nonzero(xs > 0)[0]
    zero = np.nonzero(xs == 0)[0]
    assert len(pos) and len(zero)
    up = xs.copy()
    up[pos[np.argmax(xs[pos])]] *= 1.0 + 1e-6                  # one positive weight, a millionth too large
    inn = xs.copy()
    inn[zero[len(zero) // 2]] = 1e-6 * xs.max()                # one zero weight, a millionth of the largest
    for name, x in (("optimum", xs), ("positive weight * (1 + 1e-6)", up), ("zero weight -> 1e-6 max", inn)):
        v = kkt_violation(D, order, x)
        want = dense_violation(D, order, x)
        print(f"[edges] certificate n={n} {name}: helper {v:.3e}, dense long double {max(want):.3e} {want}")
        assert abs(v - max(want)) <= 1e-12, (n, name, v, want)
    assert kkt_violation(D, order, xs) < 1e-12
    assert kkt_violation(D, order, up) > 1e-9
    assert kkt_violation(D, order, inn) > 1e-9


# ---------------------------------------------------------------------------------------------------------------- 3. CPU pre-checks of the degenerate classes
@pytest.mark.parametrize("n,seed", [(8, 1), (17, 2), (33, 3), (48, 4)])
def test_cpu_tree_metric_is_reproduced_by_2n_minus_3_splits(oracle, n, seed):
    """Dyadic branch lengths >= 1/64: an exact additive metric; the Neighbor-Net order is compatible with the tree, so the unique
    optimum reproduces the distances with the tree's 2n - 3 edges.  Both CPU references agree (the GPU tests rely on it)."""
    D = inputs.make(n, "tree", seed, oracle)
    order = oracle.run(D)[0]
    for name, x in (("nnls", nnls(D, order)), ("oracle", W.split_weights(D, order)[0])):
        res, dmax = residual(D, order, x)
        assert res <= 1e-9 * dmax, (n, name, res, dmax)
        assert int((x > 1e-6).sum()) == 2 * n - 3, (n, name, int((x > 1e-6).sum()))


def test_cpu_duplicated_taxa_are_not_separated(oracle):
    """Identical rows: at the optimum the splits with copies of one taxon on both sides carry no weight (dense NNLS, 32 taxa:
    measured 4.8e-16 of a largest weight of 1.0)."""
    n, seed = 32, 16
    D = inputs.make(n, "dup", seed, oracle)
    order = oracle.run(D)[0]
    g = duplicate_groups(D)
    assert (np.bincount(g) == 4).all()
    sep = separates_copies(order, g)
    assert 0 < sep.sum() < len(sep)
    xs = nnls(D, order)
    print(f"[edges] dup n={n}: max weight of a split that separates copies {xs[sep].max():.3e}, max weight {xs.max():.3e}")
    assert xs[sep].max() <= 1e-9 * xs.max(), (xs[sep].max(), xs.max())
    assert kkt_violation(D, order, xs) < 1e-12


def test_cpu_outgroup_oracle_distance_to_the_optimum(oracle):
    """The figure behind the tolerance of the GPU comparison at 300 taxa (ORACLE_OUTGROUP_REL above)."""
    n, seed = 48, 13
    D = inputs.make(n, "outgroup", seed, oracle)
    order = oracle.run(D)[0]
    xs = nnls(D, order)
    xl, _ = W.split_weights(D, order)
    rel = float(np.abs(xl - xs).max() / xs.max())
    print(f"[edges] outgroup n={n}: oracle to dense NNLS optimum {np.abs(xl - xs).max():.4e} absolute, {rel:.4e} of max(w) = {xs.max():.6e}")
    assert int((xs > 0.5 * inputs.OUTGROUP_DIST).sum()) == 3          # the three pendant weights
    assert 0.5 * ORACLE_OUTGROUP_REL < rel <= ORACLE_OUTGROUP_REL, rel


def test_cpu_constant_matrix_gives_the_trivial_splits_one_half(oracle):
    n = 8
    D = np.ones((n, n)) - np.eye(n)
    xs = nnls(D, identity_order(n))
    assert np.abs(xs - constant_expected(n)).max() < 1e-12
    for m in (2, 3, 8, 65):
        assert len(trivial_split_indices(m)) == (1 if m == 2 else m)


# ---------------------------------------------------------------------------------------------------------------- 2. power-of-two scaling (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize("n,seed,dist", [(257, 6, "uniform53"), (600, 7, "uniform53"), (513, 6, "treenoise")])
def test_gpu_power_of_two_scaling_is_exact(hip_api, oracle, n, seed, dist):
    """D -> ldexp(D, k) commutes with every fp64 operation of the solver, H is made of integers and every threshold is relative to
    max|A^T d| or to the objective: the weights are ldexp(w, k) bit for bit, on the same route with the same counters, while the
    objective (quadratic in the scale) stays a normal double: 2|k| + log2(n^4 max|D|^2) < 1000."""
    import fastneighbornet_amd as fa
    D = inputs.make(n, dist, seed, oracle)
    order = fa.canonical_order(D)
    w0, st0 = fa.split_weights(D, order)
    w1, st1 = fa.split_weights(D, order)
    assert (w0.view(np.int64) == w1.view(np.int64)).all(), "the unscaled solve is not reproducible: nothing below is attributable to scaling"
    assert st0["method"] == "from below"
    certify(D, order, w0, st0, (n, dist, 0))
    dmax = float(np.abs(D).max())
    for k in (-400, -60, 60, 400):
        assert 2 * abs(k) + np.log2(float(n) ** 4 * dmax ** 2) < 1000
        Dk = np.ldexp(D, k)
        wk, stk = fa.split_weights(Dk, order)
        certify(Dk, order, wk, stk, (n, dist, k))
        same = {c: (st0[c], stk[c]) for c in COUNTERS}
        print(f"[edges] scaling n={n} {dist} k={k}: {int((wk.view(np.int64) != np.ldexp(w0, k).view(np.int64)).sum())} weights differ, counters {same}")
        assert stk["method"] == st0["method"], (k, stk)
        assert all(a == b for a, b in same.values()), (k, same)
        assert (wk.view(np.int64) == np.ldexp(w0, k).view(np.int64)).all(), (k, float(np.abs(np.ldexp(wk, -k) - w0).max()))


# ---------------------------------------------------------------------------------------------------------------- 3. degenerate input classes (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize("dist,n,seed", [("tree", 64, 5), ("tree", 257, 5), ("tree", 601, 5), ("dup", 64, 16), ("dup", 257, 16), ("dup", 601, 16),
                                         ("outgroup", 300, 13), ("outgroup", 1030, 13)])
def test_gpu_degenerate_input_classes(hip_api, oracle, dist, n, seed):
    """The exact tie classes of tests/inputs.py.  Tied multipliers reach k_candidates' atomics and a sort by key only, so run-to-run
    bit identity is not asserted here; the optimum is unique and every property below is one of the optimum."""
    import fastneighbornet_amd as fa
    D = inputs.make(n, dist, seed, oracle)
    order = fa.canonical_order(D)
    w, st = fa.split_weights(D, order)
    v = certify(D, order, w, st, (dist, n))
    print(f"[edges] {dist} n={n}: {st['method']}, {st['nsplits']} splits, violation {v:.2e}, {st['t_solve_s']:.3f} s")
    assert (w >= 0).all()
    assert st["nsplits"] == int((w > 1e-6).sum())
    assert st["giveup_reason"] == 0
    if dist == "tree":
        res, dmax = residual(D, order, w)
        assert res <= 1e-9 * dmax, (res, dmax)
        assert int((w > 1e-6).sum()) == 2 * n - 3
    if dist == "dup":
        sep = separates_copies(order, duplicate_groups(D))
        assert sep.any() and w[sep].max() <= 1e-9 * w.max(), (float(w[sep].max()), float(w.max()))
    if dist == "outgroup":
        assert int((w > 0.5 * inputs.OUTGROUP_DIST).sum()) == 3
        if n == 300:
            ref, _ = W.split_weights(D, order)
            dist_to_oracle = float(np.abs(w - ref).max() / w.max())
            print(f"[edges] outgroup n={n}: GPU to CPU oracle {dist_to_oracle:.3e} of max(w) = {w.max():.6e}")
            # measured at 48 taxa (CPU, oracle to the dense optimum): 1.322e-07 of max(w); times 10
            assert dist_to_oracle <= 10 * ORACLE_OUTGROUP_REL, dist_to_oracle


# ---------------------------------------------------------------------------------------------------------------- 4. forced solver paths (GPU)
PATH_INPUTS = [(64, 4, "uniform53"), (257, 6, "uniform53"), (1030, 8, "uniform53"), (513, 6, "treenoise")]
_default_runs = {}


def path_input(oracle, n, seed, dist):
    """(D, order, weights, stats) of the default run (no knob set), once per input."""
    import fastneighbornet_amd as fa
    key = (n, seed, dist)
    if key not in _default_runs:
        D = inputs.make(n, dist, seed, oracle)
        order = fa.canonical_order(D)
        w, st = fa.split_weights(D, order)
        assert st["method"] == "from below"
        certify(D, order, w, st, ("default", key))
        w.setflags(write=False)
        _default_runs[key] = (D, order, w, st)
    return _default_runs[key]


def run_with_knobs(monkeypatch, oracle, n, seed, dist, knobs):
    """The default run (knobs unset), then the run with `knobs`; the latter must end certified, from below, and at 64 taxa at the
    dense optimum.  monkeypatch takes the knobs out again."""
    import fastneighbornet_amd as fa
    for k in ("FNN_SW_PANEL", "FNN_SW_KFRAC", "FNN_SW_RFRAC", "FNN_SW_NMS", "FNN_SW_REVIVE", "FNN_SW_REVIVE_MINF", "FNN_SW_NO_REFERENCE_ROUTE"):
        monkeypatch.delenv(k, raising=False)
    D, order, w0, st0 = path_input(oracle, n, seed, dist)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    w, st = fa.split_weights(D, order)
    for k in knobs:
        monkeypatch.delenv(k)
    show = ("free_set_peak", "capacity") + COUNTERS
    print(f"[edges] path n={n} {dist} {knobs}: default { {c: st0[c] for c in show} } knob { {c: st[c] for c in show} }")
    assert st["method"] == "from below", st
    certify(D, order, w, st, (knobs, n, dist))
    assert st["giveup_reason"] == 0
    if n == 64:
        xs = nnls(D, order, (dist, n, seed, "gpu order"))
        assert np.abs(w - xs).max() <= 1e-6 * max(1.0, xs.max()), (knobs, float(np.abs(w - xs).max()))
    return st0, st


@pytest.mark.gpu
@pytest.mark.parametrize("n,seed,dist", PATH_INPUTS)
def test_gpu_forced_path_narrow_panels(hip_api, oracle, monkeypatch, n, seed, dist):
    """FNN_SW_PANEL=64: the factor lives in many panels and entering blocks straddle panel boundaries; at 1030 taxa the free set
    exceeds the 2048 columns of one chunk of k_tri_times_small."""
    st0, st = run_with_knobs(monkeypatch, oracle, n, seed, dist, {"FNN_SW_PANEL": "64"})
    assert st["free_set_peak"] > 64, st                # more than one panel
    if n == 1030:
        assert st["free_set_peak"] > 2048, st


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", [{"FNN_SW_KFRAC": "0.001"}, {"FNN_SW_KFRAC": "0.001", "FNN_SW_PANEL": "64"}], ids=["kfrac", "kfrac+panel"])
def test_gpu_forced_path_small_blocks(hip_api, oracle, monkeypatch, knobs):
    """FNN_SW_KFRAC=0.001 at 257 taxa: kmin = max(8, n / 32) = 8, so every block has at most SMALLK = 8 splits and takes
    k_tri_times_small / k_t_times_tri_small; once with narrow panels."""
    n, seed, dist = PATH_INPUTS[1]
    st0, st = run_with_knobs(monkeypatch, oracle, n, seed, dist, knobs)
    assert 0 < st["entered"] <= 8 * st["outer_iterations"], st          # one block of <= 8 per step
    assert st["outer_iterations"] > st0["outer_iterations"], (st0, st)


@pytest.mark.gpu
@pytest.mark.parametrize("n,seed,dist", PATH_INPUTS)
def test_gpu_forced_path_largest_blocks(hip_api, oracle, monkeypatch, n, seed, dist):
    """FNN_SW_KFRAC=1.0: the largest blocks, with Schur screening and take-backs."""
    st0, st = run_with_knobs(monkeypatch, oracle, n, seed, dist, {"FNN_SW_KFRAC": "1.0"})
    assert st["screened_out"] > 0 or st["departed"] > 0, st


@pytest.mark.gpu
@pytest.mark.parametrize("n,seed,dist", PATH_INPUTS)
def test_gpu_forced_path_frequent_rebuilds(hip_api, oracle, monkeypatch, n, seed, dist):
    """FNN_SW_RFRAC=0.02: refactor() as soon as 2 % of the factor has departed."""
    st0, st = run_with_knobs(monkeypatch, oracle, n, seed, dist, {"FNN_SW_RFRAC": "0.02"})
    assert st["refactorizations"] > st0["refactorizations"], (st0, st)


@pytest.mark.gpu
@pytest.mark.parametrize("n,seed,dist", PATH_INPUTS)
def test_gpu_forced_path_departed_columns_pile_up(hip_api, oracle, monkeypatch, n, seed, dist):
    """FNN_SW_RFRAC=0.9: departed columns stay in the factor up to the buffer rule (their Gram factor, k_gather_cols_tri).  Either
    the certified optimum or a clean FNN_ECAPACITY - never an uncertified FNN_OK (FNN_SW_NO_REFERENCE_ROUTE keeps the call from
    answering a give-up with the reference's conjugate-gradient route, which is not certified)."""
    from fastneighbornet_amd._capi import FnnError
    try:
        st0, st = run_with_knobs(monkeypatch, oracle, n, seed, dist, {"FNN_SW_RFRAC": "0.9", "FNN_SW_NO_REFERENCE_ROUTE": "1"})
    except FnnError as e:
        print(f"[edges] path n={n} {dist} RFRAC=0.9: {e} {e.stats}")
        assert e.code == -6 and e.stats["giveup_reason"] != 0, (e, e.stats)
        st = e.stats
    assert st["departed"] > 0, st


@pytest.mark.gpu
@pytest.mark.parametrize("n,seed,dist", PATH_INPUTS)
@pytest.mark.parametrize("knob,value", [("FNN_SW_NMS", "0"), ("FNN_SW_NMS", "8"), ("FNN_SW_REVIVE", "0"), ("FNN_SW_REVIVE", "1")])
def test_gpu_forced_path_candidate_radius_and_revival(hip_api, oracle, monkeypatch, knob, value, n, seed, dist):
    """FNN_SW_NMS: every entry above the threshold is a candidate (0) / local maxima within Chebyshev distance 8;
    FNN_SW_REVIVE: departed splits come back through rebuilds only (0) / at the start of every step (1)."""
    run_with_knobs(monkeypatch, oracle, n, seed, dist, {knob: value})


# ---------------------------------------------------------------------------------------------------------------- 5. ABI edges (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3, 4])
def test_gpu_two_three_and_four_taxa(hip_api, oracle, n):
    import fastneighbornet_amd as fa
    for seed in (1, 2, 3):
        D = oracle.synth(n, seed)
        for order in (identity_order(n), random_order(n, 10 * n + seed)):
            w, st = fa.split_weights(D, order)
            xs = nnls(D, order)
            assert np.abs(w - xs).max() <= 1e-12 * np.abs(D).max(), (n, seed, order, w, xs, st)
            assert (w >= 0).all() and st["certified"] == 1, st
            if n == 2:
                assert w.shape == (1,) and w[0] == D[0, 1]


@pytest.mark.gpu
def test_gpu_orderings_that_are_not_the_neighbor_net_order(hip_api, oracle):
    import fastneighbornet_amd as fa
    n = 33
    D = oracle.synth(n, 3)
    order = random_order(n, 33)
    w, st = fa.split_weights(D, order)
    xs = nnls(D, order)
    assert np.abs(w - xs).max() <= 1e-6 * max(1.0, xs.max()), (float(np.abs(w - xs).max()), st)
    certify(D, order, w, st, n)
    n = 257
    D = oracle.synth(n, 6)
    order = random_order(n, 257)
    w, st = fa.split_weights(D, order)
    certify(D, order, w, st, n)
    assert (w >= 0).all() and st["nsplits"] == int((w > 1e-6).sum())


def raw_call(D_padded, n, ld, order):
    """fnn_split_weights_f64 through the C ABI on a buffer with row stride `ld` -> (status, weights, route)."""
    import fastneighbornet_amd as fa
    from fastneighbornet_amd import _capi
    w = np.zeros(W.npairs(n))
    st = _capi.FnnSwStats()
    rc = fa.api().split_weights_f64(D_padded.ctypes.data_as(C.POINTER(C.c_double)), n, ld, order.ctypes.data_as(C.POINTER(C.c_int32)), 0,
                                    w.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st))
    return rc, w, st


@pytest.mark.gpu
@pytest.mark.parametrize("n,seed", [(9, 2), (257, 6)])
def test_gpu_row_stride_larger_than_n(hip_api, oracle, n, seed):
    import fastneighbornet_amd as fa
    D = oracle.synth(n, seed)
    order = np.ascontiguousarray(fa.canonical_order(D), dtype=np.int32)
    w0, st0 = fa.split_weights(D, order)
    ld = n + 5
    P = np.full((n, ld), np.nan)
    P[:, :n] = D
    rc, w, st = raw_call(P, n, ld, order)
    assert rc == 0 and st.certified == 1 and st.route == ("closed form", "from below", "reference").index(st0["method"])
    assert (w.view(np.int64) == w0.view(np.int64)).all()
    rc, _, _ = raw_call(np.ascontiguousarray(D), n, n - 1, order)
    assert rc == -1                                                    # FNN_EINVAL


@pytest.mark.gpu
def test_gpu_all_zero_and_constant_matrices(hip_api, oracle):
    import fastneighbornet_amd as fa
    w, st = fa.split_weights(np.zeros((8, 8)), identity_order(8))
    assert (w == 0.0).all() and st["method"] == "closed form" and st["certified"] == 1 and st["nsplits"] == 0, st
    for n in (8, 65):
        D = np.ones((n, n)) - np.eye(n)
        w, st = fa.split_weights(D, identity_order(n))
        assert (w == constant_expected(n)).all(), (n, np.nonzero(w != constant_expected(n))[0][:8])
        assert st["method"] == "closed form" and st["certified"] == 1 and st["nsplits"] == n, st


@pytest.mark.gpu
@pytest.mark.parametrize("n,seed", [(12, 7), (300, 5)])
@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_gpu_non_finite_distances_are_refused(hip_api, oracle, n, seed, bad):
    """A NaN or an infinity among the distances used to come back as FNN_OK with NaN weights by the closed-form route (no
    comparison with a NaN is true, so no weight counted as negative).  Now: FNN_EINVAL before any route is chosen."""
    import fastneighbornet_amd as fa
    from fastneighbornet_amd._capi import FnnError
    D = oracle.synth(n, seed)
    order = fa.canonical_order(D)
    a, b = 1, n - 2
    D[a, b] = D[b, a] = bad
    for call in (lambda: fa.split_weights(D, order), lambda: fa.split_weights_sparse(D, order)):
        with pytest.raises(FnnError) as ei:
            call()
        assert ei.value.code == -1 and "FNN_EINVAL" in str(ei.value) and "distances" in str(ei.value), ei.value

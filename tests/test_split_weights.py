"""Circular split weights.  CPU part: the oracle (oracle/csw_oracle.c, a
restatement of CircularSplitWeights.java with the distance re-ordering restored) is pinned
mathematically - against a dense non-negative least-squares solve of the reference's LIVE design
matrix (FastNN.java:405-437; the optimum is unique) and against the known weights of synthetic
circular metrics.  GPU part: fnn_split_weights_f64 against the oracle."""
import numpy as np
import pytest

from common import kkt_violation
from oracle import csw_oracle as W


def circ_instance(n, seed, density=0.4):
    """Random hidden circular order + random non-negative split weights -> (D, ordering, weights)."""
    rng = np.random.default_rng(seed)
    order = np.concatenate([[0, 1], 2 + rng.permutation(n - 1)]).astype(np.int32)
    A = W.live_design_matrix(n, order)
    w = rng.random(A.shape[1]) * (rng.random(A.shape[1]) < density)
    b = A @ w
    D = np.zeros((n, n))
    k = 0
    for a in range(n):
        for c in range(a + 1, n):
            D[a, c] = D[c, a] = b[k]
            k += 1
    return D, order, w


def test_operators_are_adjoint_and_match_the_dense_matrix():
    rng = np.random.default_rng(1)
    for n in (4, 5, 8, 13):
        ident = np.arange(n + 1, dtype=np.int32)
        A_live = W.live_design_matrix(n, ident)
        # live column k=(i,j) <-> fast split: (i-1,j-1) for i>=1, (j-1,n-1) for i=0
        cols = []
        for i in range(n):
            for j in range(i + 1, n):
                fi, fj = (i - 1, j - 1) if i >= 1 else (j - 1, n - 1)
                cols.append((2 * n - fi - 3) * fi // 2 + fj - 1)
        A_fast = np.zeros_like(A_live)
        A_fast[:, cols] = A_live
        x = rng.random(W.npairs(n))
        y = rng.random(W.npairs(n))
        assert np.allclose(W.calculate_ab(n, x), A_fast @ x, rtol=1e-12, atol=1e-12)
        assert np.allclose(W.calculate_atx(n, y), A_fast.T @ y, rtol=1e-12, atol=1e-12)
        assert abs(W.calculate_ab(n, x) @ y - x @ W.calculate_atx(n, y)) < 1e-9


def test_oracle_matches_dense_nnls_of_the_live_design_matrix(oracle):
    import scipy.optimize as so
    for n, seed in [(4, 1), (5, 2), (6, 3), (8, 4), (11, 5), (14, 6)]:
        D = oracle.synth(n, seed)
        order, _, _ = oracle.run(D)
        A = W.live_design_matrix(n, order)
        xs, _ = so.nnls(A, W.packed_distances(D), maxiter=200000)
        xl, st = W.split_weights(D, order)
        assert np.abs(xs - xl).max() < 1e-6 * max(1.0, np.abs(xs).max()), (n, np.abs(xs - xl).max())
        assert (xl >= 0).all()


def test_oracle_recovers_known_circular_weights():
    for n, seed in [(6, 1), (9, 2), (15, 3), (24, 4)]:
        D, order, w = circ_instance(n, seed)
        xl, st = W.split_weights(D, order)
        assert np.abs(xl - w).max() < 1e-9, (n, np.abs(xl - w).max())


def fast_x(n, live):
    """live index order (FastNN.java:405-419) -> the fast algorithm's packed upper triangle"""
    x = np.zeros(W.npairs(n))
    k = 0
    for i in range(n):
        for j in range(i + 1, n):
            fi, fj = (i - 1, j - 1) if i >= 1 else (j - 1, n - 1)
            x[(2 * n - fi - 3) * fi // 2 + fj - 1] = live[k]
            k += 1
    return x


@pytest.mark.gpu
def test_gpu_split_weights_reach_the_nnls_optimum(hip_api, oracle):
    """north_star: split weights within 1e-6 relative.  The reference's live path solves the dense problem to the
    optimum (FastNN.java:401-454); so: 1e-6 against scipy's Lawson-Hanson on the live design matrix wherever that is
    computable, and the Kuhn-Tucker certificate beyond (it needs no second solver)."""
    import fastneighbornet_amd as fa
    import scipy.optimize as so
    for n, seed, dist in [(5, 1, "uniform53"), (9, 2, "uniform53"), (12, 7, "dec4"), (20, 8, "uniform53"), (33, 3, "uniform53"),
                          (48, 9, "dec4"), (64, 4, "uniform53")]:
        D = oracle.synth(n, seed, dist)
        order = fa.canonical_order(D)
        got, st = fa.split_weights(D, order)
        xs, _ = so.nnls(W.live_design_matrix(n, order), W.packed_distances(D), maxiter=10 ** 7)
        assert np.abs(got - xs).max() <= 1e-6 * max(1.0, np.abs(xs).max()), (n, np.abs(got - xs).max(), st)
        assert (got >= 0).all() and st["nsplits"] == int((xs > 1e-6).sum())
        assert st["method"] == "from below"
        # the CPU oracle (the reference's conjugate-gradient method) is a little short of that optimum, by its own
        # stopping rule: pin it where it is
        ref, _ = W.split_weights(D, order)
        assert np.abs(ref - xs).max() < 2e-5
    for n, seed in [(150, 5), (257, 6), (600, 7)]:
        D = oracle.synth(n, seed)
        order = fa.canonical_order(D)
        got, st = fa.split_weights(D, order)
        assert kkt_violation(D, order, got) < 1e-9, (n, kkt_violation(D, order, got), st)
    # the reference's own method (from above) is still there and agrees with its CPU restatement
    import os
    os.environ["FNN_SW_REFERENCE_METHOD"] = "1"
    try:
        for n, seed, tol in [(12, 7, 1e-6), (33, 3, 2e-5), (64, 4, 2e-5)]:
            D = oracle.synth(n, seed)
            order = fa.canonical_order(D)
            ref, st_ref = W.split_weights(D, order)
            got, st = fa.split_weights(D, order)
            assert st["method"] == "reference" and np.abs(got - ref).max() < tol, (n, np.abs(got - ref).max(), st, st_ref)
    finally:
        os.environ.pop("FNN_SW_REFERENCE_METHOD", None)
    # circular metrics: the known weights come back (closed form where every split of the metric is positive,
    # from below or from above where zeros have to be found)
    # (n > 40: built with the prefix-sum operator - the dense live design matrix of 300 taxa has 2e9 entries and took the GPU box 140 s)
    for n, seed, dens in [(12, 7, 0.4), (40, 8, 0.4), (120, 9, 0.4), (300, 10, 0.05), (1024, 11, 1.0)]:
        D, order, w = circ_instance(n, seed, dens) if n <= 40 else circ_instance_fast(n, seed, dens)
        got, st = fa.split_weights(D, order)
        assert np.abs(got - w).max() < 1e-6 * max(1.0, w.max()), (n, np.abs(got - w).max(), st)


def circ_instance_fast(n, seed, density=1.0):
    """A large circular metric (a fraction `density` of the splits positive), built with the prefix-sum operator instead of the dense matrix."""
    rng = np.random.default_rng(seed)
    order = np.concatenate([[0, 1], 2 + rng.permutation(n - 1)]).astype(np.int32)
    x = rng.random(W.npairs(n)) + 0.01          # fast index space
    if density < 1.0:
        x *= rng.random(W.npairs(n)) < density
    dpos = W.calculate_ab(n, x)                 # distances between cycle POSITIONS
    D = np.zeros((n, n))
    iu = np.triu_indices(n, 1)
    P = np.zeros((n, n)); P[iu] = dpos; P = P + P.T
    tax = order[1:] - 1                          # position -> taxon
    D[np.ix_(tax, tax)] = P
    live = np.zeros(W.npairs(n))
    k = 0
    for i in range(n):
        for j in range(i + 1, n):
            fi, fj = (i - 1, j - 1) if i >= 1 else (j - 1, n - 1)
            live[k] = x[(2 * n - fi - 3) * fi // 2 + fj - 1]
            k += 1
    return D, order, live


def test_index_maps_agree():
    from common import live_to_fast
    rng = np.random.default_rng(3)
    for n in (5, 12, 40):
        live = rng.random(W.npairs(n))
        assert (live_to_fast(n, live) == fast_x(n, live)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n,seed,dist,budget_s", [(4096, 1, "uniform53", 10.0), (8192, 2, "uniform53", 40.0), (4096, 3, "dec4", 10.0),
                                                  (4096, 6, "treenoise", 15.0), (4096, 1, "neg", 10.0)])
def test_gpu_split_weights_kkt_at_baseline_sizes(hip_api, oracle, n, seed, dist, budget_s):
    """Beyond dense reach the weights are held to the solver-independent Kuhn-Tucker certificate (violation < 1e-9 of |A^T d|)
    and to a time budget: the block active-set method solves 4096 taxa in ~2 s and 8192 in ~6 s
    where the one-split-per-step solver of round 2 took 34 s and 203 s.  Tree + 5 % noise distances (what real data look
    like) have 3.8 n positive splits instead of 2.4 n; with negative entries d has negative components."""
    import fastneighbornet_amd as fa
    import inputs
    D = inputs.make(n, dist, seed, oracle)
    order = fa.canonical_order(D)
    got, st = fa.split_weights(D, order)
    assert st["method"] == "from below" and st["certified"] == 1 and st["giveup_reason"] == 0
    assert st["t_solve_s"] <= budget_s, st
    v = kkt_violation(D, order, got)
    assert v < 1e-9, (n, v, st)
    # the solver's own check (device operators) and the independent one (host, the oracle's operators) see the same violation
    assert st["kkt_violation"] < 1e-9 and abs(st["kkt_violation"] - v) <= 1e-10 + 0.5 * max(v, st["kkt_violation"]), (v, st)
    assert (got >= 0).all() and st["nsplits"] == int((got > 1e-6).sum())


@pytest.mark.gpu
def test_gpu_split_weights_argument_errors(hip_api, oracle):
    import fastneighbornet_amd as fa
    from fastneighbornet_amd._capi import FnnError
    D = oracle.synth(8, 1)
    bad = np.array([0, 1, 2, 3, 4, 5, 6, 7, 7], dtype=np.int32)   # not a permutation
    with pytest.raises(FnnError):
        fa.split_weights(D, bad)


@pytest.mark.gpu
def test_config5_end_to_end_32768(hip_api, oracle, hostlib_nexus):
    """BASELINE.json configs[4]: 32768 taxa end to end on one MI355X - circular order, circular split weights, Nexus document
    (FastNN.java:369-491).  The order must be the oracle's golden; the weights are solved from below (block active-set
    method), pass the solver's own certificate AND the solver-independent Kuhn-Tucker check with the oracle's operators on
    the host (violation < 1e-9 of max|A^T d|); the document is written by the routine the CLI runs (printNexusFromWeights)
    with nsplits = the number of weights above the reference's 1e-6 threshold (FastNN.java:455).  Time budgets: weights
    <= 100 s of device time, document <= 30 s."""
    import ctypes as C
    import hashlib
    import json
    import os
    import time
    import fastneighbornet_amd as fa
    from fastneighbornet_amd._capi import Handle
    n, seed = 32768, 1
    gold = {(c["n"], c["dist"], c["seed"]): c for c in
            json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_big.json")))["cases"]}[(n, "uniform53", seed)]
    with Handle(hip_api, n) as h:
        h.synth(seed, "uniform53")
        order, st = h.run()
    assert hashlib.sha256(order.tobytes()).hexdigest() == gold["order_sha256"]
    D = oracle.synth(n, seed)                      # the same matrix, generated on the host by the oracle's generator
    t0 = time.time()
    w, sw = fa.split_weights(D, order)
    t_w = time.time() - t0
    assert sw["method"] == "from below" and sw["certified"] == 1 and sw["kkt_violation"] < 1e-9, sw
    assert sw["t_solve_s"] <= 100.0, sw
    ns_expected = int((w > 1e-6).sum())
    assert (w >= 0).all() and sw["nsplits"] == ns_expected and 2.0 * n < ns_expected < 3.0 * n, (ns_expected, sw)
    names = b"".join((f"t{i + 1}".encode()).ljust(256, b"\0") for i in range(n))
    t0 = time.time()
    ns = hostlib_nexus.fnnh_write_nexus(b"/dev/null", n, D.ctypes.data_as(C.POINTER(C.c_double)), names,
                                        order.ctypes.data_as(C.POINTER(C.c_int32)), w.ctypes.data_as(C.POINTER(C.c_double)))
    t_doc = time.time() - t0
    assert ns == ns_expected and t_doc <= 30.0, (ns, ns_expected, t_doc)
    v = kkt_violation(D, order, w)
    print(f"config 5: order {st.t_total_s:.2f} s, weights {sw['t_solve_s']:.1f} s device / {t_w:.1f} s wall, document {t_doc:.1f} s, "
          f"{ns} splits, Kuhn-Tucker violation {v:.2e} (solver's own: {sw['kkt_violation']:.2e})")
    assert v < 1e-9, (v, sw)


@pytest.fixture(scope="module")
def hostlib_nexus():
    import ctypes as C
    import os
    from fastneighbornet_amd import build
    build.build()
    lib = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(build.__file__)), "libfastnn_host.so"))
    lib.fnnh_write_nexus.argtypes = [C.c_char_p, C.c_int32, C.POINTER(C.c_double), C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    lib.fnnh_write_nexus.restype = C.c_int32
    return lib


@pytest.mark.gpu
def test_gpu_split_weights_nearly_circular_inputs_and_the_capacity_status(hip_api, oracle, monkeypatch):
    """Distances whose optimum has far more positive splits than random or tree-like ones: a circular metric with 1 %
    multiplicative noise (tests/inputs.py: circ_noise) ends with ~20 n positive splits (measured: 21 877 at 1024 taxa, 41 034 at
    2048, 73 946 at 4096).  The block method's default factor (8 n splits at this size) cannot hold them: it gives up for
    CAPACITY and is run again with four times the capacity (as much as device memory holds: ~150 000 splits whatever n) -
    3.8 s at 1024 taxa where the reference's conjugate-gradient route took 80 s and stopped 1.5e-7 short of the Kuhn-Tucker
    conditions.  Where even the largest factor is too small (16384 taxa of this class: ~330 000 splits) the call returns
    FNN_ECAPACITY with the reason in the stats instead of running that route for hours; here the capacity is pinned to provoke it."""
    import time
    import fastneighbornet_amd as fa
    import inputs
    from fastneighbornet_amd._capi import FnnError
    n = 1024
    D = inputs.circ_noise(n, 11)
    order = fa.canonical_order(D)
    t0 = time.time()
    w, st = fa.split_weights(D, order)
    dt = time.time() - t0
    assert st["method"] == "from below" and st["certified"] == 1 and st["giveup_reason"] == 0, st
    assert st["capacity"] > 8 * n + 64 and st["nsplits"] > 15 * n, st      # the retry happened, and it was needed
    assert dt <= 20.0, (dt, st)
    assert kkt_violation(D, order, w) < 1e-9
    n2 = 2048
    D2 = inputs.circ_noise(n2, 12)
    order2 = fa.canonical_order(D2)
    monkeypatch.setenv("FNN_SW_CAP", "2")                                   # factor capacity 2 n + 1024 splits, no retry
    with pytest.raises(FnnError) as ei:
        fa.split_weights(D2, order2)
    assert ei.value.code == -6 and "FNN_ECAPACITY" in str(ei.value), ei.value
    assert ei.value.stats["giveup_reason"] == 1 and ei.value.stats["free_set_peak"] > 0, ei.value.stats
    monkeypatch.setenv("FNN_SW_REFERENCE_MAX_N", "4096")                    # ... and the reference's route where the caller allows it
    monkeypatch.setenv("FNN_SW_CAP", "0.05")
    D3 = inputs.circ_noise(96, 13)
    order3 = fa.canonical_order(D3)
    w3, st3 = fa.split_weights(D3, order3)
    assert st3["method"] == "reference" and st3["giveup_reason"] == 1 and kkt_violation(D3, order3, w3) < 1e-5, st3


@pytest.mark.gpu
def test_gpu_sparse_output_equals_the_dense_one(hip_api, oracle):
    """fnn_split_weights_sparse_f64 returns exactly the entries of the dense result above the threshold, in the order of the
    reference's list (ascending live index, FastNN.java:455-466) - also when the first call's room was too small."""
    import fastneighbornet_amd as fa
    for n, seed in [(9, 2), (257, 6), (1500, 7)]:
        D = oracle.synth(n, seed)
        order = fa.canonical_order(D)
        dense, st = fa.split_weights(D, order)
        for thr, cap in [(1e-6, 0), (0.01, 0), (1e-6, 3)]:
            idx, w, st2 = fa.split_weights_sparse(D, order, threshold=thr, capacity=cap)
            want = np.nonzero(dense > thr)[0]
            assert (idx == want).all() and (w == dense[want]).all(), (n, thr, cap)
            assert st2["nsplits"] == len(want) and st2["certified"] == 1


@pytest.mark.gpu
def test_gpu_buffer_pool_between_calls(hip_api, oracle):
    """The solver's large device buffers stay in a per-process pool between calls (hipMalloc of ~220 GB costs 0.5-4.8 s at 32768
    taxa): a second solve of the same size allocates next to nothing, gives bit-identical weights on the recycled (dirty) buffers,
    and fnn_split_weights_release_cache hands the memory back."""
    import fastneighbornet_amd as fa
    D = oracle.synth(3000, 5)
    order = fa.canonical_order(D)
    w1, st1 = fa.split_weights(D, order)
    w2, st2 = fa.split_weights(D, order)
    assert (w1.view(np.int64) == w2.view(np.int64)).all()
    assert st2["t_alloc_s"] < 0.05, (st1["t_alloc_s"], st2["t_alloc_s"])
    assert fa.api().split_weights_release_cache() == 0
    w3, st3 = fa.split_weights(D, order)
    assert (w1.view(np.int64) == w3.view(np.int64)).all()


@pytest.mark.gpu
def test_gpu_split_weights_report_a_result_that_fails_their_own_check(hip_api, oracle, monkeypatch):
    """FNN_EINEXACT: the call checks what it returns (g = A^T (A x - d) from the implicit operators) and does not claim the optimum for
    weights that fail - here provoked by a test hook that doubles one weight behind the solver's back."""
    import fastneighbornet_amd as fa
    from fastneighbornet_amd._capi import FnnError
    D = oracle.synth(200, 4)
    order = fa.canonical_order(D)
    good, st = fa.split_weights(D, order)
    assert st["certified"] == 1
    monkeypatch.setenv("FNN_SW_FAULT_PERTURB", "1")
    with pytest.raises(FnnError) as ei:
        fa.split_weights(D, order)
    assert ei.value.code == -7 and "Kuhn-Tucker" in str(ei.value)
    w, st2 = fa.split_weights(D, order, allow_inexact=True)       # the weights are there for a caller who wants them anyway
    assert st2["certified"] == 0 and st2["kkt_violation"] > 1e-9
    assert int((w != good).sum()) == 1

"""Relaxed mode with TIED row minima, and the mode's value range.

On uniform53 / dec4 matrices (tests/test_relaxed.py) a row minimum of Q(p, .) is attained by one row or by the two nodes of
one cluster.  k identical taxa make k - 1 rows tie bit for bit (inputs.dupk), which is what the rest of the row minimum is
for: a thread that finds more than two ties among its own slots and walks them again, ties collected from several threads,
waves and workgroups, their sort into position order, list entries past the first two, several mutual pairs with one drawn
by java.util.Random (a wrong count shifts the stream and every later event), and a list that is full (RL_TIES = 16, fnn_core.h):
17 ties end the run with FNN_ECAPACITY.  The reference for all of it is the oracle, event for event, bits of `best` included.

Every test asserts on its INPUT what the input is meant to provoke (inputs.first_event_ties, plain numpy), so that a
generator that drifts fails the precondition instead of silently testing nothing.
"""
import re

import numpy as np
import pytest

import inputs
from common import bits, compare_trajectory
from fastneighbornet_amd._capi import FnnError, Handle
from test_relaxed import TRAJ, compare

RL_TIES = 16              # fnn_core.h
CHUNK_SLOTS = 2 * 1024    # 2 * RL_T (fnn_hip.hip): a workgroup takes the row pass in chunks of RL_T slot PAIRS
DBL_MIN = float(np.finfo(np.float64).tiny)
DBL_MAX = float(np.finfo(np.float64).max)

DUPK_RUNS = [(k, n) for k in (3, 5, 8, 12, 16, 17) for n in (6 * k, 20 * k + 3)] + [(17, 600)]
OTHER_RUNS = [(dist, n) for dist in ("tree", "neg", "outgroup", "twovalued") for n in (33, 300)]
SCALED_RUNS = [(n, side) for n in (33, 300) for side in ("largest", "smallest")]
DEEP = [(17, 102), (8, 163)]


def dupk_checked(oracle, n, k, seed, rows=None):
    """inputs.dupk with its purpose asserted: (sampled) rows with exactly k - 1 tied row minima at the first event exist, and
    no row has more."""
    D = inputs.dupk(n, k, seed, oracle)
    cnt = np.array([len(t) for t in inputs.first_event_ties(D, rows)])
    assert (cnt == k - 1).any() and cnt.max() == k - 1, f"dupk({n}, {k}) no longer gives k - 1 tied row minima: {np.bincount(cnt)}"
    return D


def other_input(oracle, dist, n, seed):
    if dist == "twovalued":
        r = np.random.default_rng(seed)
        D = np.triu(r.integers(1, 3, (n, n)).astype(np.float64), 1)
        D = D + D.T
        assert set(np.unique(D)) == {0.0, 1.0, 2.0}
        return D
    return inputs.make(n, dist, seed, oracle)


def scale_exponent(D, side):
    """Power-of-two scalings commute with every fp64 operation of the algorithm while nothing overflows or goes subnormal
    (tests/test_value_range.py).  The largest value the algorithm forms is below 4 n max |D|: `largest` is the largest k at
    which that bound times 2^k is finite.  `smallest`: the issue's rule was the smallest k at which the same bound stays
    normal, but there the ENTRIES are subnormal (they are 4 n times smaller than the bound), ldexp(D, k) drops their low bits
    and the oracle itself leaves its trajectory - the relation is gone, and there is nothing to compare with.  What has to
    stay normal on the small side is the smallest thing formed, not the largest: a quarter ulp of the smallest non-zero
    entry (entries are averaged in twos and fours before anything rounds at a larger magnitude).  `smallest` is the smallest
    k at which that is normal; the oracle-against-oracle check of the test holds the choice to account."""
    n = D.shape[0]
    a = np.abs(D[D != 0])
    if side == "largest":
        top = 4.0 * n * float(a.max())
        k = int(np.floor(np.log2(DBL_MAX / top)))
        with np.errstate(over="ignore"):
            while np.isfinite(np.ldexp(top, k + 1)):
                k += 1
            while not np.isfinite(np.ldexp(top, k)):
                k -= 1
            assert np.isfinite(np.ldexp(top, k)) and not np.isfinite(np.ldexp(top, k + 1))
        return k
    low = float(np.spacing(a.min())) / 4.0
    k = int(np.ceil(np.log2(DBL_MIN / low)))
    while np.ldexp(low, k - 1) >= DBL_MIN:
        k -= 1
    while np.ldexp(low, k) < DBL_MIN:
        k += 1
    assert np.ldexp(low, k) >= DBL_MIN > np.ldexp(low, k - 1)
    return k


def scaled_case(oracle, n, side, seed, rseed):
    """uniform53 times 2^k with the premise checked on the oracle alone: same trajectory as unscaled, best times 2^k."""
    D = oracle.synth(n, seed, "uniform53")
    k = scale_exponent(D, side)
    assert (k > 900) if side == "largest" else (k < -900), k
    Dk = np.ldexp(D, k)
    assert np.isfinite(Dk).all() and (np.abs(Dk[Dk != 0]) >= DBL_MIN).all()
    o0, e0 = oracle.run_relaxed(D, rseed, 4)
    ok, ek = oracle.run_relaxed(Dk, rseed, 4)
    assert (o0 == ok).all()
    for f in TRAJ + ["entries"]:
        assert (e0[f] == ek[f]).all(), (k, f)
    want = np.ldexp(e0["best"], k)
    assert np.isfinite(want).all() and (np.abs(want[want != 0]) >= DBL_MIN).all()
    assert (bits(ek["best"]) == bits(want)).all(), k
    return Dk


def whole_dupk(api, oracle, k, n):
    compare(api, oracle, dupk_checked(oracle, n, k, 100 + k), 4000 + n, 4)


def whole_other(api, oracle, dist, n):
    compare(api, oracle, other_input(oracle, dist, n, 21), 5000 + n, 4)


def whole_scaled(api, oracle, n, side):
    compare(api, oracle, scaled_case(oracle, n, side, 22, 6000 + n), 6000 + n, 4)


def deep_dupk(api, oracle, k, n):
    compare_trajectory(api, oracle, dupk_checked(oracle, n, k, 200 + k), relaxed_seed=79, relaxed_min_active=4)


def step_together(api, oracle, D, seed, events, nodes_every=16):
    """Engine and oracle stepped together for the first `events` events: event key and bits of best at every event, node
    ids / partners / Sx bits at every `nodes_every`-th (a whole run of the oracle at these sizes would take minutes)."""
    st = oracle.Stepper(D, relaxed_seed=seed, relaxed_min_active=4)
    h = Handle(api, D.shape[0], relaxed_seed=seed, relaxed_min_active=4)
    try:
        h.set_matrix(D)
        h.begin()
        for k in range(events):
            eo, eg = st.step(), h.step()
            assert eo is not None and eg is not None, k
            assert eo.key() == eg.key(), (k, eo.key(), eg.key())
            assert bits([eo.best])[0] == bits([eg.best])[0], (k, eo.best, eg.best)
            assert eo.entries == eg.entries, k
            if k % nodes_every == 0 or k == events - 1:
                ids, _, nbr, sx = st.nodes()
                gi, gn, gs = h.nodes()
                assert (ids == gi).all() and (nbr == gn).all(), k
                assert (bits(sx) == bits(gs)).all(), k
    finally:
        h.close()
        st.close()


def spread_dupk(oracle, n, k, seed):
    """dupk whose ties are spread over the chunks of the row pass: taxon i starts in slot i (fnn_core.h init_thread:
    pslot[k] = k), so for EVERY one of 200 sampled rows the tied indices fall into at least two chunks."""
    rows = np.random.default_rng(seed).choice(n, 200, replace=False)
    D = inputs.dupk(n, k, seed, oracle)
    ties = inputs.first_event_ties(D, rows)
    cnt = np.array([len(t) for t in ties])
    assert (cnt == k - 1).any() and cnt.max() == k - 1, np.bincount(cnt)
    nchunks = np.array([len(set((t // CHUNK_SLOTS).tolist())) for t in ties])
    assert (nchunks >= 2).all(), f"rows whose ties sit in one chunk: {rows[nchunks < 2].tolist()}"
    return D


def same_thread_ties(oracle, n, seed):
    """n / 4 treenoise taxa, taxon j in the slots 2j, 2j + 1, 2j + 2048, 2j + 2049: with one workgroup these are the two slot
    pairs of thread j (pairs j and j + RL_T), so every row has its three tied row minima in ONE thread - the thread has to
    walk its slots a second time (rl_rowmin_block, more than two ties)."""
    assert n == 2 * CHUNK_SLOTS
    T = inputs.make(n // 4, "treenoise", seed, oracle)
    s = np.arange(n)
    idx = (s // 2) % (CHUNK_SLOTS // 2)
    D = np.ascontiguousarray(T[np.ix_(idx, idx)])
    rows = np.random.default_rng(seed).choice(n, 200, replace=False)
    for p, t in zip(rows, inputs.first_event_ties(D, rows)):
        assert len(t) == 3 and (((t // 2) % (CHUNK_SLOTS // 2)) == (p // 2) % (CHUNK_SLOTS // 2)).all(), (p, t)
    return D


def overflow_inputs(oracle):
    D18 = inputs.dupk(108, 18, 31, oracle)
    assert max(len(t) for t in inputs.first_event_ties(D18)) == RL_TIES + 1
    C = np.full((33, 33), 0.25)
    np.fill_diagonal(C, 0.0)
    assert all(len(t) == 32 for t in inputs.first_event_ties(C))
    return D18, C


def check_overflow_error(e):
    """FNN_ECAPACITY, with the mode, the limit, the usual cause and the way out in the message; device code 20 (the list), not
    23 (a hand-over between workgroups that failed or ran into its deadline)."""
    msg = str(e)
    assert e.code == -6 and msg.startswith("FNN_ECAPACITY: "), msg
    assert "Relaxed mode" in msg and f"{RL_TIES} tied row minima" in msg, msg
    assert f"more than {RL_TIES + 1} identical taxa" in msg and "constant matrix" in msg and "-mode Canonical" in msg, msg
    assert "unreachable" not in msg
    assert re.findall(r"device code (\d+)", msg) == ["20"], msg


def run_expecting_overflow(api, D, seed=7):
    with Handle(api, D.shape[0], relaxed_seed=seed, relaxed_min_active=4) as h:
        h.set_matrix(D)
        with pytest.raises(FnnError) as ei:
            h.run()
    check_overflow_error(ei.value)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the emulation (the shared control flow of relaxed_find with a plain loop for the row minimum) against the oracle

def test_first_event_ties_is_the_criterion_of_the_first_event(oracle):
    """the helper against a direct double loop, on a matrix with ties (dupk) and one without"""
    for D in (inputs.dupk(23, 5, 3, oracle), oracle.synth(17, 4)):
        n = D.shape[0]
        S = D.sum(axis=1)
        every = inputs.first_event_ties(D)
        for p, got in enumerate(every):
            q = {j: ((n - 2.0) * D[p, j] - S[p]) - S[j] for j in range(n) if j != p}
            lo = min(q.values())
            assert got.tolist() == [j for j in sorted(q) if q[j] == lo]
        assert [t.tolist() for t in inputs.first_event_ties(D, [3, 5])] == [every[3].tolist(), every[5].tolist()]


def test_dupk_leaves_dup_alone(oracle):
    """dupk(k = 4) is "dup" (whose matrix hash the big goldens pin), and k copies of a taxon are identical rows"""
    assert (inputs.dupk(203, 4, 8, oracle) == inputs.make(203, "dup", 8, oracle)).all()
    D = inputs.dupk(60, 5, 9, oracle)
    assert sorted(np.unique(D, axis=0, return_counts=True)[1].tolist()) == [5] * 12


@pytest.mark.parametrize("k,n", DUPK_RUNS)
def test_emulation_dupk_matches_oracle(emu_api, oracle, k, n):
    whole_dupk(emu_api, oracle, k, n)


@pytest.mark.parametrize("dist,n", OTHER_RUNS)
def test_emulation_other_classes_match_oracle(emu_api, oracle, dist, n):
    whole_other(emu_api, oracle, dist, n)


@pytest.mark.parametrize("n,side", SCALED_RUNS)
def test_emulation_scaled_matches_oracle(emu_api, oracle, n, side):
    whole_scaled(emu_api, oracle, n, side)


@pytest.mark.parametrize("k,n", DEEP)
def test_emulation_dupk_deep_state_matches_oracle(emu_api, oracle, k, n):
    deep_dupk(emu_api, oracle, k, n)


def test_emulation_ties_within_one_threads_slots(emu_api, oracle):
    """(the input of the GPU test below: the emulation pins that the oracle's trajectory is reachable by the shared code)"""
    step_together(emu_api, oracle, same_thread_ties(oracle, 4096, 41), 4100, 40)


def test_emulation_refuses_a_full_tie_list_by_name(emu_api, oracle):
    D18, C = overflow_inputs(oracle)
    run_expecting_overflow(emu_api, D18)
    run_expecting_overflow(emu_api, C)
    with Handle(emu_api, 108) as h:  # the Canonical mode takes the same matrix
        h.set_matrix(D18)
        assert (h.run()[0] == oracle.run(D18)[0]).all()


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the workgroup's row minimum (rl_rowmin_block, RlBlockEnv::rowmin in fnn_hip.hip) against the oracle

@pytest.mark.gpu
@pytest.mark.parametrize("k,n", DUPK_RUNS)
def test_gpu_dupk_matches_oracle(hip_api, oracle, k, n):
    whole_dupk(hip_api, oracle, k, n)


@pytest.mark.gpu
@pytest.mark.parametrize("dist,n", OTHER_RUNS)
def test_gpu_other_classes_match_oracle(hip_api, oracle, dist, n):
    whole_other(hip_api, oracle, dist, n)


@pytest.mark.gpu
@pytest.mark.parametrize("n,side", SCALED_RUNS)
def test_gpu_scaled_matches_oracle(hip_api, oracle, n, side):
    whole_scaled(hip_api, oracle, n, side)


@pytest.mark.gpu
@pytest.mark.parametrize("k,n", DEEP)
def test_gpu_dupk_deep_state_matches_oracle(hip_api, oracle, k, n):
    deep_dupk(hip_api, oracle, k, n)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [2, 3, 16])
@pytest.mark.parametrize("k,n", [(17, 4200), (12, 6200)])
def test_gpu_ties_across_workgroups(hip_api, oracle, monkeypatch, grid, k, n):
    """tie lists merged from several workgroups' records: every sampled row has its ties in at least two chunks of the row
    pass, k = 17 fills the list to the last entry.  The first 80 events."""
    monkeypatch.setenv("FNN_RELAXED_GRID", str(grid))
    step_together(hip_api, oracle, spread_dupk(oracle, n, k, 300 + k), 7000 + n, 80)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [2, 3])
def test_gpu_ties_across_workgroups_whole_run(hip_api, oracle, monkeypatch, grid):
    monkeypatch.setenv("FNN_RELAXED_GRID", str(grid))
    rows = np.random.default_rng(5).choice(2100, 200, replace=False)
    compare(hip_api, oracle, dupk_checked(oracle, 2100, 8, 51, rows), 8100, 64)


@pytest.mark.gpu
def test_gpu_ties_within_one_threads_slots(hip_api, oracle, monkeypatch):
    """more than two ties among ONE thread's slots: the thread walks its slots a second time.  One workgroup (the default
    below 12 288 live nodes); the first 40 events, while most clusters still sit where they started."""
    monkeypatch.delenv("FNN_RELAXED_GRID", raising=False)
    step_together(hip_api, oracle, same_thread_ties(oracle, 4096, 41), 4100, 40)


@pytest.mark.gpu
def test_gpu_refuses_a_full_tie_list_by_name(hip_api, oracle, monkeypatch):
    """one workgroup: 17 ties are refused with FNN_ECAPACITY; the constant matrix too; afterwards a fresh handle runs the
    Relaxed mode as if nothing had happened, and the Canonical mode takes the refused matrix"""
    monkeypatch.delenv("FNN_RELAXED_GRID", raising=False)
    D18, C = overflow_inputs(oracle)
    run_expecting_overflow(hip_api, D18)
    run_expecting_overflow(hip_api, C)
    compare(hip_api, oracle, oracle.synth(300, 61), 62, 4)
    with Handle(hip_api, 108) as h:
        h.set_matrix(D18)
        assert (h.run()[0] == oracle.run(D18)[0]).all()


@pytest.mark.gpu
def test_gpu_refuses_a_full_tie_list_across_workgroups(hip_api, oracle, monkeypatch):
    """three workgroups: no single record is over the limit, the merged list is.  The error comes at the first event, as
    code 20 and not as a failed hand-over; the next handle (with its own mailbox) runs to the oracle's order."""
    monkeypatch.setenv("FNN_RELAXED_GRID", "3")
    n = 4200
    D = inputs.dupk(n, 18, 32, oracle)
    ties = inputs.first_event_ties(D, np.random.default_rng(6).choice(n, 200, replace=False))
    assert max(len(t) for t in ties) == RL_TIES + 1
    # (the merged list overflows although every workgroup's own share fits)
    assert any(len(t) == RL_TIES + 1 and np.bincount(t // CHUNK_SLOTS).max() <= RL_TIES for t in ties)
    with Handle(hip_api, n, relaxed_seed=9, relaxed_min_active=4) as h:
        h.set_matrix(D)
        h.begin()
        with pytest.raises(FnnError) as ei:
            h.step()
    check_overflow_error(ei.value)
    compare(hip_api, oracle, oracle.synth(300, 61), 62, 4)

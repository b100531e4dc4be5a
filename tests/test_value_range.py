"""The screened default mode at the edges of the value range.

D -> ldexp(D, k) commutes with every fp64 operation of the algorithm as long as nothing overflows or goes subnormal, so
the committed goldens (tests/golden/oracle_big.json) hold for the scaled matrices too: the same order and trajectory,
and every scan minimum equal to ldexp(golden best, k) bit for bit.  The engine's screening pass (k_screen, k_resolve,
k_emit; fnn_core.h "Screening") works on fp32 row sums and a bf16 copy of the matrix, which see very different numbers
at such scales: float row sums that overflow to inf while max |D| < 1e37 (k_band, k_all: the engine once screened there,
and the emulation diverged from the oracle; screening now needs max |D| (3n + 64) < 1e37), past that (k_off), the largest
scale that still screens (k_edge), entries in the fp32 / bf16 subnormal range (-140) and entries that are 0 in float
(-900).  The CPU tests pin the premise: the oracle obeys the relation.
"""
import json
import os

import numpy as np
import pytest

import inputs
from fastneighbornet_amd._capi import Handle

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TRAJ_FIELDS = ["m_before", "c_before", "cx_id", "cy_id", "x_id", "y_id", "kind", "u_id"]
KNAMES = ["k_band", "k_all", "k_off", "k_edge", "k_m60", "k_m140", "k_m900"]
DBL_MIN = float(np.finfo(np.float64).tiny)


def golden(n, dist, seed):
    doc = json.load(open(os.path.join(GOLD, "oracle_big.json")))
    c = {(c["n"], c["dist"], c["seed"]): c for c in doc["cases"]}[(n, dist, seed)]
    return c, np.load(os.path.join(GOLD, c["npz"]))


_mat = {}


def matrix(n, dist, seed, oracle):
    """The golden's input matrix (host side, checked against its hash) and its exponents; one matrix kept at a time."""
    key = (n, dist, seed)
    if key not in _mat:
        _mat.clear()
        c, _ = golden(n, dist, seed)
        D = inputs.make(n, dist, seed, oracle)
        assert inputs.sha_big(D) == c["matrix_sha256"], "the input generator drifted from the committed golden"
        _mat[key] = (D, inputs.scale_exponents(D))
    return _mat[key]


def check_against_golden(ev, order, n_events, sum_entries, c, z, k):
    """Trajectory, order and counters as in the golden; every scan minimum is the golden's times 2^k, bit for bit."""
    traj = np.stack([ev[f] for f in TRAJ_FIELDS], axis=1)
    want = np.ldexp(z["best_bits"].view(np.float64), k)
    assert (np.abs(want[want != 0]) >= DBL_MIN).all() and np.isfinite(want).all(), "the relation does not hold at this k"
    best = np.ascontiguousarray(ev["best"]).view(np.int64)
    wbits = want.view(np.int64)
    kk = min(len(traj), len(z["traj"]))
    bad = np.nonzero((traj[:kk] != z["traj"][:kk]).any(axis=1) | (best[:kk] != wbits[:kk]))[0]
    assert bad.size == 0, (f"k={k}: first diverging event {bad[0]}: got {traj[bad[0]].tolist()} best {ev['best'][bad[0]]!r} "
                           f"oracle {z['traj'][bad[0]].tolist()} best {want[bad[0]]!r}")
    assert len(traj) == c["n_events"] and n_events == c["n_events"] and sum_entries == c["sum_entries"]
    assert (order == z["order"]).all()


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the premise.  The oracle itself obeys the relation, so the GPU test below checks the engine and not a false premise.

@pytest.mark.parametrize("n,dist,seed", [(4096, "uniform53", 1), (4096, "tree", 5)])
def test_oracle_obeys_power_of_two_scaling_at_golden_sizes(oracle, n, dist, seed):
    c, z = golden(n, dist, seed)
    D, ks = matrix(n, dist, seed, oracle)
    for name in ("k_band", "k_all", "k_edge", "k_m140"):
        k = ks[name]
        order, ev, se = oracle.run(np.ldexp(D, k), threads=8)
        check_against_golden(ev, order, len(ev), se, c, z, k)


@pytest.mark.parametrize("dist,seed", [("uniform53", 1), ("dec4", 2), ("tree", 3), ("treenoise", 4), ("neg", 5),
                                       ("circnoise", 6), ("outgroup", 7), ("dup", 8)])
def test_oracle_obeys_power_of_two_scaling_small(oracle, dist, seed):
    n = 600
    D = inputs.make(n, dist, seed, oracle)
    o0, e0, s0 = oracle.run(D)
    ks = inputs.scale_exponents(D, band=(0.0, 1.0))
    for k in ks.values():
        o, e, s = oracle.run(np.ldexp(D, k))
        assert (o == o0).all() and s == s0, k
        for f in TRAJ_FIELDS + ["entries"]:
            assert (e[f] == e0[f]).all(), (k, f)
        want = np.ldexp(e0["best"], k)
        assert (np.abs(want[want != 0]) >= DBL_MIN).all()
        assert (e["best"].view(np.int64) == want.view(np.int64)).all(), k


def test_scale_exponents_land_where_intended(oracle):
    """(CPU) the exponents of the GPU sweep: k_band splits the float row sums, k_all overflows all of them below the screening
    limit, k_off is past it, and the small exponents put the entries where the sweep says."""
    for n, dist, seed in [(4096, "uniform53", 1), (4096, "dec4", 1), (4096, "tree", 5), (4096, "treenoise", 6)]:
        D, ks = matrix(n, dist, seed, oracle)
        dmax = float(np.abs(D).max())
        assert 0.1 <= inputs.float_rowsum_overflow(D, ks["k_band"]) <= 0.9
        assert np.ldexp(dmax, ks["k_band"]) < inputs.SCREEN_DMAX_LIMIT
        assert inputs.float_rowsum_overflow(D, ks["k_all"]) == 1.0
        assert np.ldexp(dmax, ks["k_all"]) < inputs.SCREEN_DMAX_LIMIT <= np.ldexp(dmax, ks["k_off"])
        assert inputs.screens(D, ks["k_edge"]) and not inputs.screens(D, ks["k_edge"] + 1) and ks["k_edge"] < ks["k_band"]
        assert inputs.float_rowsum_overflow(D, ks["k_edge"] + 5) == 0.0
        assert all(inputs.screens(D, ks[k]) for k in ("k_m60", "k_m140", "k_m900"))
        with np.errstate(under="ignore"):
            small = np.ldexp(D[D != 0], ks["k_m140"]).astype(np.float32)
            assert (np.abs(small) < np.finfo(np.float32).tiny).all()           # every nonzero entry is a float subnormal (or 0)
            assert (np.ldexp(D, ks["k_m900"]).astype(np.float32) == 0).all()   # every entry is 0 in float


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the default mode (screening, lookahead windows) on the scaled matrices against the goldens.

GPU_CASES = [(4096, "uniform53", 1), (4096, "dec4", 1), (4096, "tree", 5), (4096, "treenoise", 6), (16384, "uniform53", 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("kname", KNAMES)
@pytest.mark.parametrize("n,dist,seed", GPU_CASES)
def test_scaled_default_mode_matches_oracle_golden(hip_api, oracle, n, dist, seed, kname):
    c, z = golden(n, dist, seed)
    D, ks = matrix(n, dist, seed, oracle)
    k = ks[kname]
    frac = inputs.float_rowsum_overflow(D, k)
    if kname == "k_band":
        assert 0.1 <= frac <= 0.9
    with Handle(hip_api, n, record_events=True) as h:
        h.set_matrix(np.ldexp(D, k))
        order, st = h.run()
        ev = h.events()
    print(json.dumps({"n": n, "dist": dist, "seed": seed, "k": kname, "kval": k, "overflow": round(frac, 3),
                      "n_screen_events": st.n_screen_events, "n_rescan_units": st.n_rescan_units,
                      "n_base_scans": st.n_base_scans, "n_window_hits": st.n_window_hits}))
    check_against_golden(ev, order, st.n_events, st.sum_entries, c, z, k)
    if inputs.screens(D, k):
        assert st.n_screen_events > 0, "the screened default mode did not run"
        if n >= 16384 and kname in ("k_m140", "k_m900"):
            # bounds collapsed to the slack: every unit is a candidate, more than k_resolve's list holds (RES_LIST = 4096,
            # fnn_hip.hip), so its overflow branch - all workgroups share the rescans - served the large events
            assert st.n_rescan_units > 4096 * st.n_screen_events, (st.n_rescan_units, st.n_screen_events)
    else:  # float row sums could overflow: the plain fp64 scan for every event
        assert st.n_screen_events == 0 and st.n_window_hits == 0, "screening must stay off when a float of its bound can overflow"
    assert st.n_handover_retries == 0


def test_outgroup_slack_exceeds_the_spread_of_q(oracle):
    """(CPU) the outgroup class does what it is for: at the first event the screening slack screen_delta (fnn_core.h,
    proportional to max |D|) exceeds the whole spread of Q, so k_resolve's threshold admits every unit."""
    for n, seed in [(4096, 13), (8192, 14)]:
        D = inputs.make(n, "outgroup", seed, oracle)
        S = D.sum(axis=1)
        lo, hi = np.inf, -np.inf
        for r0 in range(0, n, 1024):
            Q = (n - 2) * D[r0:r0 + 1024] - S[r0:r0 + 1024, None] - S[None, :]
            Q[np.arange(Q.shape[0]), np.arange(r0, r0 + Q.shape[0])] = np.nan
            lo, hi = min(lo, np.nanmin(Q)), max(hi, np.nanmax(Q))
        delta = 2.0 * 2.0 ** -24 * np.abs(D).max() * (7.0 * (n - 2) + 6.0 * n)
        assert 2.0 * delta > hi - lo, (delta, hi - lo)

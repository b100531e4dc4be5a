"""The decide step's record for k_update (packed plan + prefetched block of the involved slots, fnn_core.h: UpdPre) on the GPU:
bit-exact parity with the oracle through common.compare_trajectory - event records, Sx, the consumers of T and the live matrix
after every few events - on every path that writes or reads the record, and the record's own counters (fnn_debug_update_pre).

Stepping (compare_trajectory) closes every event with k_finalize, so the exact row sum of the newest cluster is never pending
when the next event is decided; only whole runs defer it into the next k_track, where the prefetch has to leave it out
(UpdPre::mask).  The window cases therefore run each input both ways: stepped for the deep comparison, and as a whole run
against the oracle's trajectory for the counters."""
import ctypes as C

import numpy as np
import pytest

from common import bits, compare_trajectory, tree_metric
from fastneighbornet_amd._capi import Handle

pytestmark = pytest.mark.gpu


@pytest.fixture
def windows_on(monkeypatch):
    """Screening and lookahead windows at small sizes: the knobs are read when a handle is created."""
    monkeypatch.setenv("FNN_SCREEN_MIN_N", "8")
    monkeypatch.setenv("FNN_SCREEN_MIN_M", "8")


def update_pre(api, h):
    api._fn("debug_update_pre", C.c_int32, [C.c_void_p, C.POINTER(C.c_int64)])
    out = (C.c_int64 * 4)()
    api.check(api.debug_update_pre(h._h, out))
    return {"consumed": out[0], "masked": out[1], "stale": out[2]}


_REF = {}


def reference(oracle, key, make):
    """(D, order, events, sum of entries) of the oracle, computed once per input."""
    if key not in _REF:
        D = make()
        _REF[key] = (D,) + tuple(oracle.run(D, threads=4))
    return _REF[key]


def whole_run(api, ref, **kw):
    """One fnn_run against the oracle's trajectory; returns the run's statistics and the record's counters."""
    D, o_ref, ev_ref, se = ref
    n = D.shape[0]
    with Handle(api, n, record_events=True, **kw) as h:
        h.set_matrix(D)
        order, st = h.run()
        ev = h.events()
        pre = update_pre(api, h)
    assert (order == o_ref).all()
    assert st.n_events == len(ev_ref) and st.sum_entries == se
    for f in ("m_before", "c_before", "cx_id", "cy_id", "x_id", "y_id", "kind", "u_id", "entries"):
        assert (ev[f] == ev_ref[f]).all(), f
    assert (bits(ev["best"]) == bits(ev_ref["best"])).all()
    assert pre["stale"] == 0
    assert pre["consumed"] == st.n_events  # every event's update took its plan and its block from the record
    return st, pre


@pytest.mark.parametrize("n,seed,dist", [(300, 2, "uniform53"), (300, 3, "dec4"), (601, 4, "uniform53"), (601, 5, "dec4")])
def test_window_events(hip_api, oracle, windows_on, n, seed, dist):
    """The decide step in k_track's tail: stepped (deep), then as a whole run, where the newest cluster's exact row sum is
    still pending when the next event is decided and the update must take it from the chain workgroup's word."""
    ref = reference(oracle, (n, seed, dist), lambda: oracle.synth(n, seed, dist))
    compare_trajectory(hip_api, oracle, ref[0], deep=True, deep_every=7)
    st, pre = whole_run(hip_api, ref)
    assert st.n_window_hits > 0
    assert pre["masked"] > 0
    assert st.n_handover_retries == 0


@pytest.mark.parametrize("n,seed,dist", [(300, 2, "uniform53"), (300, 3, "dec4"), (601, 4, "uniform53"), (601, 5, "dec4")])
def test_scan_events(hip_api, oracle, n, seed, dist):
    """The same inputs without windows: every event scans, k_decide leaves the record, nothing is ever pending."""
    ref = reference(oracle, (n, seed, dist), lambda: oracle.synth(n, seed, dist))
    compare_trajectory(hip_api, oracle, ref[0], deep=True, deep_every=7)
    st, pre = whole_run(hip_api, ref)
    assert st.n_window_hits == 0 and pre["masked"] == 0


@pytest.mark.parametrize("dist", ["uniform53", "dec4"])
def test_finish_and_smallest_sizes(hip_api, oracle, windows_on, dist):
    """The special finish (its own branch of the decide step) and the extremes of the number of involved slots."""
    for n in (4, 5, 8, 9, 33, 65):
        for seed in (1, 2):
            D = oracle.synth(n, seed, dist)
            compare_trajectory(hip_api, oracle, D, deep=True)
            whole_run(hip_api, (D,) + tuple(oracle.run(D)))


@pytest.mark.parametrize("exact", [False, True])
def test_tie_rich_tree(hip_api, oracle, windows_on, exact):
    """An additive tree metric: exact ties of the criterion, uncertified 4-candidate choices - the exact ComputeRx sums (and, in
    the whole run, their helper workgroups) run between the decide step's loads and the record."""
    n = 300
    ref = reference(oracle, (n, "tree"), lambda: tree_metric(n, 2))
    compare_trajectory(hip_api, oracle, ref[0], deep=True, deep_every=5, force_exact_rx=exact)
    st, pre = whole_run(hip_api, ref, force_exact_rx=exact)
    assert st.n_rx_exact > 0
    assert st.n_window_hits > 0


def test_stalled_launches(hip_api, oracle, windows_on):
    """Long windows over few tracked pairs give out early: the launches up to the next scheduled scan stall - no decide step, the
    record in memory is the previous event's - and must apply nothing."""
    n = 601
    ref = reference(oracle, (n, 4, "uniform53"), lambda: oracle.synth(n, 4, "uniform53"))
    st, pre = whole_run(hip_api, ref, lookahead=64, lookahead_pairs=16)
    assert st.n_stalled_events > 0
    assert st.n_window_hits > 0

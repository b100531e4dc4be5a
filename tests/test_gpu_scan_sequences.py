"""GPU: launch sequences that scan carry k_track with its chain workgroup and ONE tracking workgroup (plus the helper
workgroups of the exact ComputeRx sums), and the chain workgroup hands its sum over without a release fence and takes
the short form for few addends.  Whole runs - scheduled scans, window events and the end game in one run - against the
oracle, and a committed golden whose run takes the exact re-sweep (the reader of the chain workgroup's flag)."""
import hashlib
import json
import os

import numpy as np
import pytest

import inputs
from common import bits, compare_trajectory
from fastneighbornet_amd._capi import Handle

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ("m_before", "c_before", "cx_id", "cy_id", "x_id", "y_id", "kind", "u_id", "entries")


def whole_run_against_oracle(api, oracle, D):
    """One run without host round trips per event (batches of launch sequences, the row sum beside the next event's
    tracking): the order and every event's record, scan minimum included, must be the oracle's."""
    n = D.shape[0]
    o_ref, ev_ref, se = oracle.run(D, threads=8)
    with Handle(api, n, record_events=True) as h:
        h.set_matrix(D)
        order, st = h.run()
        ev = h.events()
    assert (order == o_ref).all()
    assert st.n_events == len(ev_ref) and st.sum_entries == se
    for f in FIELDS:
        assert (ev[f] == ev_ref[f]).all(), f
    assert (bits(ev["best"]) == bits(ev_ref["best"])).all()
    assert st.n_handover_retries == 0
    return st


def test_run_across_the_thresholds(hip_api, oracle, monkeypatch):
    """2500 taxa with the screening pass on (it is off below 4096 taxa by default): scheduled scans and window events while
    at least min(2048, n / 4) = 625 nodes are live, the end game below; the row sums cross CH_SHORT_M on the way."""
    monkeypatch.setenv("FNN_SCREEN_MIN_N", "8")
    D = oracle.synth(2500, 5, "uniform53")
    st = whole_run_against_oracle(hip_api, oracle, D)
    assert st.n_base_scans > 10 and st.n_window_hits > 1000, (st.n_base_scans, st.n_window_hits)
    # event by event, with the nodes' exact row sums (Sx bits) every 61st event
    compare_trajectory(hip_api, oracle, D, deep=True, deep_every=61)


def test_run_with_helper_workgroups(hip_api, oracle, monkeypatch):
    """An additive tree metric with dyadic branch lengths (exact ties of the criterion: the <= 4 ComputeRx sums are evaluated
    exactly, by k_track's helper workgroups once a batch has needed them), screening on: the slim grid with helpers."""
    monkeypatch.setenv("FNN_SCREEN_MIN_N", "8")
    D = inputs.make(1024, "tree", 5, oracle)
    st = whole_run_against_oracle(hip_api, oracle, D)
    print("helpers run:", "rx_exact", st.n_rx_exact, "base_scans", st.n_base_scans, "window_hits", st.n_window_hits)
    # the helpers are launched from the batch after one that evaluated exact sums: without such sums this run would exercise the
    # slim grid without helpers only.  (Base scans come every few dozen events through the whole run, so some follow that batch.)
    assert st.n_rx_exact > 0, st.n_rx_exact
    assert st.n_base_scans > 10 and st.n_window_hits > 0, (st.n_base_scans, st.n_window_hits)
    compare_trajectory(hip_api, oracle, D, deep=True, deep_every=61)


def test_golden_that_takes_the_exact_resweep(hip_api, oracle):
    """The tree-metric golden at 4096 taxa (tests/golden/oracle_big.json: 4096, "tree", seed 5).  Its ties make swept pairs
    compete with the window's best pair, so the deciding workgroup waits for the chain workgroup's flag and sweeps again
    with the exact sum (n_sweeps_exact > 0): the hand-over without the writer's fence is taken, and the order is the golden's."""
    n, dist, seed = 4096, "tree", 5
    c = {(c["n"], c["dist"], c["seed"]): c for c in json.load(open(os.path.join(GOLD, "oracle_big.json")))["cases"]}[(n, dist, seed)]
    D = inputs.make(n, dist, seed, oracle)
    assert inputs.sha_big(D) == c["matrix_sha256"], "the input generator drifted from the committed golden"
    with Handle(hip_api, n) as h:
        h.set_matrix(D)
        order, st = h.run()
    assert hashlib.sha256(order.tobytes()).hexdigest() == c["order_sha256"]
    assert st.n_handover_retries == 0
    assert st.n_sweeps_exact > 0

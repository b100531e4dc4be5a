"""The continuous event feed on the GPU (fnn_engine.h: agglomerate_feed; fnn_hip.hip: feed_post, HipBackend::feed_*): whole runs
whose host follows the records that k_update (or, without windows, k_finalize) posts into pinned host memory instead of
draining the stream per batch.  Order and the whole event log must equal the oracle's at every depth and with the feed off;
a handle that has run before must give what a fresh one gives (a stale mailbox or generation would show there); an error in
the device state must come back as an error, not as a hang."""
import hashlib
import json
import os
import time

import numpy as np
import pytest

import inputs
from common import bits
from fastneighbornet_amd._capi import FnnError, Handle
from test_gpu_update_plan import reference, windows_on  # noqa: F401  (the fixture, and the oracle's results once per input)

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ("m_before", "c_before", "cx_id", "cy_id", "x_id", "y_id", "kind", "u_id", "entries")
INPUTS = {"uniform53": lambda o: o.synth(601, 4, "uniform53"), "dec4": lambda o: o.synth(601, 5, "dec4"),
          "tree": lambda o: inputs.make(601, "tree", 3, o)}


def ref601(oracle, dist):
    key = (601, 4, "uniform53") if dist == "uniform53" else ((601, 5, "dec4") if dist == "dec4" else (601, "tree", 3, "inputs"))
    return reference(oracle, key, lambda: INPUTS[dist](oracle))


def run_and_compare(api, ref, handle=None, **kw):
    """One fnn_run; order and every event record equal the oracle's.  Returns the run's statistics."""
    D, o_ref, ev_ref, se = ref
    n = D.shape[0]
    h = handle if handle is not None else Handle(api, n, record_events=True, **kw)
    try:
        h.set_matrix(D)
        order, st = h.run()
        ev = h.events()
    finally:
        if handle is None:
            h.close()
    assert (order == o_ref).all()
    assert st.n_events == len(ev_ref) and st.sum_entries == se
    for f in FIELDS:
        assert (ev[f] == ev_ref[f]).all(), f
    assert (bits(ev["best"]) == bits(ev_ref["best"])).all()
    return st


@pytest.mark.parametrize("dist", ["uniform53", "dec4", "tree"])
@pytest.mark.parametrize("depth", ["1", "2", None, "4096", "off"])
def test_order_and_event_log_at_every_depth(hip_api, oracle, windows_on, monkeypatch, dist, depth):  # noqa: F811
    if depth == "off":
        monkeypatch.setenv("FNN_FEED", "0")
    elif depth is not None:
        monkeypatch.setenv("FNN_FEED_DEPTH", depth)
    st = run_and_compare(hip_api, ref601(oracle, dist))
    assert st.n_window_hits > 0
    assert st.n_handover_retries == 0


def test_windows_that_give_out_early(hip_api, oracle, windows_on, monkeypatch):  # noqa: F811
    """lookahead = 64 over 16 wanted pairs (test_gpu_update_plan.test_stalled_launches): sequences stall until the host hears
    of it.  With one sequence in flight the host hears after one; in batches it hears at the end of the window's schedule:
    the feed must stall less - which also shows that it is the feed that ran."""
    ref = ref601(oracle, "uniform53")
    st = run_and_compare(hip_api, ref, lookahead=64, lookahead_pairs=16)
    assert st.n_stalled_events > 0 and st.n_window_hits > 0
    monkeypatch.setenv("FNN_FEED_DEPTH", "1")
    one = run_and_compare(hip_api, ref, lookahead=64, lookahead_pairs=16)
    monkeypatch.setenv("FNN_FEED", "0")
    off = run_and_compare(hip_api, ref, lookahead=64, lookahead_pairs=16)
    print("stalled sequences: default depth", st.n_stalled_events, "depth 1", one.n_stalled_events, "batches", off.n_stalled_events)
    assert 0 < one.n_stalled_events < off.n_stalled_events


@pytest.mark.parametrize("n", [4, 5, 9])
def test_runs_shorter_than_the_depth(hip_api, oracle, windows_on, n):  # noqa: F811
    for dist, seed in (("uniform53", 1), ("dec4", 2)):
        D = oracle.synth(n, seed, dist)
        run_and_compare(hip_api, (D,) + tuple(oracle.run(D)))


def test_later_runs_on_one_handle_equal_a_fresh_handle(hip_api, oracle, windows_on):  # noqa: F811
    """Two different matrices on one handle, then the first again: the mailbox and its generation start afresh every time."""
    a, b = ref601(oracle, "uniform53"), ref601(oracle, "dec4")
    with Handle(hip_api, 601, record_events=True) as h:
        for ref in (a, b, a):
            used = run_and_compare(hip_api, ref, handle=h)
            fresh = run_and_compare(hip_api, ref)
            assert (used.n_events, used.n_window_hits, used.n_base_scans) == (fresh.n_events, fresh.n_window_hits, fresh.n_base_scans)


def test_without_windows_k_finalize_posts(hip_api, oracle):
    """300 taxa as they come: no screening copy, no windows, every event scans and k_finalize closes it - and posts."""
    ref = reference(oracle, (300, 2, "uniform53"), lambda: oracle.synth(300, 2, "uniform53"))
    st = run_and_compare(hip_api, ref)
    assert st.n_window_hits == 0


def test_an_error_in_the_device_state_ends_the_run(hip_api, oracle, windows_on, monkeypatch):  # noqa: F811
    """FNN_FAULT_ERROR=0:40 (the status word 99 written into the device state after event 40, read when the ranks are set - one
    rank here): the records carry it, the host stops feeding and reports it - well inside the wait limit - and the handle goes."""
    monkeypatch.setenv("FNN_FAULT_ERROR", "0:40")
    monkeypatch.setenv("FNN_FEED_WAIT_MS", "20000")
    D = ref601(oracle, "uniform53")[0]
    t0 = time.perf_counter()
    with Handle(hip_api, 601) as h:
        h.comm_init_host(1, 0, lambda send: [send])
        h.set_matrix(D)
        with pytest.raises(FnnError) as ei:
            h.run()
    assert "code 99" in str(ei.value)
    assert time.perf_counter() - t0 < 10.0
    monkeypatch.delenv("FNN_FAULT_ERROR")
    run_and_compare(hip_api, ref601(oracle, "uniform53"))  # (and the next handle runs as if nothing had been)


def test_golden_4096(hip_api, oracle):
    n, dist, seed = 4096, "uniform53", 1
    c = {(c["n"], c["dist"], c["seed"]): c for c in json.load(open(os.path.join(GOLD, "oracle_big.json")))["cases"]}[(n, dist, seed)]
    D = inputs.make(n, dist, seed, oracle)
    assert inputs.sha_big(D) == c["matrix_sha256"], "the input generator drifted from the committed golden"
    with Handle(hip_api, n) as h:
        h.set_matrix(D)
        order, st = h.run()
    assert hashlib.sha256(order.tobytes()).hexdigest() == c["order_sha256"]
    assert st.n_window_hits > 0 and st.n_handover_retries == 0

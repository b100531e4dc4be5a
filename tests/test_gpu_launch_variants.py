"""Every kernel variant the HIP backend can select, on the GPU: the environment switches that choose between k_screen<NT, SCHED>,
k_scan<NT>, k_track<HELP> / k_decide<HELP> and the deferred / immediate close of an event are read when a handle is created,
so each case is a fresh child process with the switch set.  n = 300 with the screening pass forced on down to 64 live nodes
(FNN_SCREEN_MIN_N=8, FNN_SCREEN_MIN_M=64: screened events with windows first, plain fp64 scans at the end), whole runs of two
inputs: uniform53 seed 1, and an additive tree metric with dyadic branch lengths, whose exact ties make the run compute exact
ComputeRx sums - the helper workgroups of k_track / k_decide.  Under every switch the order and the recorded events must be
the oracle's, and no hand-over between workgroups may have needed a second try.  The last case sets two switches at once: it is
the only way to k_screen<false, false>."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 300
FIELDS = ("m_before", "c_before", "cx_id", "cy_id", "x_id", "y_id", "kind", "u_id", "entries")

CHILD = r'''
import os, sys
sys.path.insert(0, os.environ["FNN_ROOT"])
import numpy as np
import fastneighbornet_amd as fa
from fastneighbornet_amd._capi import Handle
ref = np.load(sys.argv[1])
a = fa.api()
for name in ("uniform53", "tree"):
    D = ref[name + "_D"]
    with Handle(a, D.shape[0], record_events=True) as h:
        h.set_matrix(D)
        order, st = h.run()
        ev = h.events()
    assert (order == ref[name + "_order"]).all(), name
    assert st.n_events == len(ref[name + "_best"]) and st.sum_entries == int(ref[name + "_se"]), name
    for f in %r:
        assert (ev[f] == ref[name + "_" + f]).all(), (name, f)
    assert (ev["best"].view(np.int64) == ref[name + "_best"].view(np.int64)).all(), name
    assert st.n_handover_retries == 0, (name, st.n_handover_retries)
    print("RUN", name, "screen_events", st.n_screen_events, "window_hits", st.n_window_hits, "rx_exact", st.n_rx_exact,
          "plain_launches", st.plain_launches)
    assert st.n_screen_events > 0 and st.n_window_hits > 0, name   # screened events (k_screen, k_track) and window events ran
    assert st.n_events > 64 + 3                                      # ... and events below FNN_SCREEN_MIN_M: the plain scan (k_scan)
    if name == "tree":
        assert st.n_rx_exact > 0, name   # exact ComputeRx sums: the next batch of events launches the HELP variants
print("VARIANT_OK")
''' % (FIELDS,)


@pytest.fixture(scope="module")
def reference(oracle, tmp_path_factory):
    """Both inputs with the oracle's order and events, computed once and handed to every child as one file."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import inputs
    out = {}
    for name, D in (("uniform53", oracle.synth(N, 1, "uniform53")), ("tree", inputs.make(N, "tree", 5, oracle))):
        order, ev, se = oracle.run(D)
        out[name + "_D"], out[name + "_order"], out[name + "_se"] = D, order, np.int64(se)
        for f in FIELDS + ("best",):
            out[name + "_" + f] = ev[f]
    path = str(tmp_path_factory.mktemp("launch_variants") / "reference.npz")
    np.savez(path, **out)
    return path


@pytest.mark.parametrize("switch", [None, "FNN_SCAN_NT=0", "FNN_UNSCHED_SCANS=1", "FNN_RX_HELPERS=0", "FNN_NO_DEFER=1",
                                    "FNN_SCAN_NT=0 FNN_UNSCHED_SCANS=1"])
def test_run_equals_oracle_under_switch(reference, switch):
    env = dict(os.environ, FNN_ROOT=ROOT, FNN_SCREEN_MIN_N="8", FNN_SCREEN_MIN_M="64")
    for name in ("FNN_SCAN_NT", "FNN_UNSCHED_SCANS", "FNN_RX_HELPERS", "FNN_NO_DEFER"):
        env.pop(name, None)
    for assignment in (switch or "").split():
        name, value = assignment.split("=")
        env[name] = value
    r = subprocess.run([sys.executable, "-c", CHILD, reference], env=env, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "VARIANT_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]

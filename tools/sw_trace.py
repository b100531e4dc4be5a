"""Development aid: the path and the bits of the one-problem split-weight solver on a fixed list of cases, one JSON line each
(sha256 of the weight bytes, method and route, every integer counter of the stats, the two float fields as float.hex()).
Two builds that print the same lines took the same path to the same bits.  The cases are the smallest at which each path of the
block method runs (tests/test_split_weights_edges.py: PATH_INPUTS under each FNN_SW_* setting of that file; tests/
test_split_weights.py: the capacity retry, the pinned capacity, the reference's route) - input classes whose run-to-run bit
identity the suite asserts; the tied classes (tree, dup) are left out: their candidate order goes through atomics.

    python tools/sw_trace.py > trace.jsonl
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fastneighbornet_amd as fa  # noqa: E402
from fastneighbornet_amd._capi import FnnError, Handle  # noqa: E402
import inputs  # noqa: E402  (tests/inputs.py: the input classes of the suite)


class DeviceSynth:
    """What tests/inputs.py asks of its generator module: the SplitMix64 classes, here from the engine's own
    device generator."""
    @staticmethod
    def synth(n, seed, dist="uniform53"):
        with Handle(fa.api(), n) as h:
            h.synth(seed, dist)
            return h.matrix()


PATH_INPUTS = [(64, 4, "uniform53"), (257, 6, "uniform53"), (1030, 8, "uniform53"), (513, 6, "treenoise")]
KNOBS = [{}, {"FNN_SW_PANEL": "64"}, {"FNN_SW_KFRAC": "0.001"}, {"FNN_SW_KFRAC": "1.0"}, {"FNN_SW_RFRAC": "0.02"},
         {"FNN_SW_RFRAC": "0.9", "FNN_SW_NO_REFERENCE_ROUTE": "1"}, {"FNN_SW_NMS": "0"}, {"FNN_SW_NMS": "8"}, {"FNN_SW_REVIVE": "0"},
         {"FNN_SW_REVIVE": "1"}]
INTS = ("outer_iterations", "refactorizations", "solves", "entered", "screened_out", "departed", "nsplits", "capacity", "free_set_peak",
        "n_set_aside", "giveup_reason", "certified")
# Left out: with FNN_SW_NMS=0 every entry above the threshold is a candidate; at these two sizes they outnumber the candidate
# list, and which of them the list keeps depends on the order of the appending atomics: two runs of ONE build differ
# (profiles/r15/README.md).  --all runs them too.
NOT_REPRODUCIBLE = {(1030, "FNN_SW_NMS", "0"), (513, "FNN_SW_NMS", "0")}
ALL_KNOBS = sorted({k for kn in KNOBS for k in kn} | {"FNN_SW_CAP", "FNN_SW_REFERENCE_MAX_N", "FNN_SW_LOG", "FNN_SW_REFERENCE_METHOD",
                                                       "FNN_SW_ALLOW_REFERENCE_ROUTE", "FNN_SW_FAULT_PERTURB"})


def trace(case, D, order, knobs):
    for k in ALL_KNOBS:
        os.environ.pop(k, None)
    os.environ.update(knobs)
    line = {"case": case, "knobs": knobs}
    try:
        w, st = fa.split_weights(D, order)
        line.update(status="FNN_OK", sha256=hashlib.sha256(w.tobytes()).hexdigest(), method=st["method"], route=int(st["route"]))
    except FnnError as e:  # a clean give-up is a result: its stats are printed
        st = e.stats
        line.update(status=f"error {e.code}", sha256=None, method=None, route=int(st["route"]))
    for k in knobs:
        del os.environ[k]
    line.update({k: int(st[k]) for k in INTS if k in st})
    line.update({k: float(st[k]).hex() for k in ("final_threshold_rel", "kkt_violation")})
    print(json.dumps(line, sort_keys=True), flush=True)


def main():
    for n, seed, dist in PATH_INPUTS:
        D = inputs.make(n, dist, seed, DeviceSynth)
        order = fa.canonical_order(D)
        for knobs in KNOBS:
            if "--all" not in sys.argv and any((n, k, v) in NOT_REPRODUCIBLE for k, v in knobs.items()):
                continue
            trace(f"{dist} n={n} seed={seed}", D, order, knobs)
    for n, seed, knobs in [(1024, 11, {}), (2048, 12, {"FNN_SW_CAP": "2"}), (96, 13, {"FNN_SW_CAP": "0.05", "FNN_SW_REFERENCE_MAX_N": "4096"})]:
        D = inputs.circ_noise(n, seed)
        trace(f"circ_noise n={n} seed={seed}", D, fa.canonical_order(D), knobs)


if __name__ == "__main__":
    main()

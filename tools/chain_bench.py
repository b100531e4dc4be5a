"""Development aid: duration of the exact chain-sum kernel (FNN_CHAIN_TIME=1).

Per size: the form the engine takes (with the record form's phase split, stamped by thread 0), then the record form
and the short form forced (FNN_CHAIN_FORM=2 / 3: their crossover), then the first form stopped after the loads +
prefix / the automata / the segmented scan (FNN_CHAIN_STOP=1..3) with --first-form.  Sizes: the command line, or 512 4096 32768."""
import sys, os, ctypes as C
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import fastneighbornet_amd as fa
a = fa.api()
os.environ["FNN_CHAIN_TIME"] = "1"
rng = np.random.default_rng(1)
first_form = "--first-form" in sys.argv[1:]
sizes = [int(x) for x in sys.argv[1:] if x != "--first-form"] or [512, 4096, 32768]


def run(v, label):
    out = C.c_double(); st = (C.c_int32 * 4)()
    print(f"m={len(v)} {label}:", flush=True)
    a.check(a.test_chain_sum(0, v.ctypes.data_as(C.POINTER(C.c_double)), len(v), 1, 32, C.byref(out), st))
    return st


for m in sizes:
    v = rng.random(m) + 2.0**-10
    os.environ.pop("FNN_CHAIN_STOP", None)
    os.environ.pop("FNN_CHAIN_FORM", None)
    st = run(v, "engine's form")
    print(f"[fnn] stats: runs={st[0]} mixed={st[1]} run_fail={st[2]} thread_fail={st[3]}", flush=True)
    for form in (2, 3):
        if form == 3 and m > 2048:
            continue
        os.environ["FNN_CHAIN_FORM"] = str(form)
        run(v, "record form" if form == 2 else "short form")
    os.environ.pop("FNN_CHAIN_FORM", None)
    if first_form:
        for stop in (1, 2, 3):
            os.environ["FNN_CHAIN_STOP"] = str(stop)
            run(v, f"first form, stop_after={stop}")

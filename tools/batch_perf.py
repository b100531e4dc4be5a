"""Many small problems: the batch call against the loop over fnn_canonical_order_f64.

B = 1024 uniform53 problems at n = 32, 64, 128 and fnn_batch_lds_max_n().  For each n: (a) one
fnn_canonical_order_batch_f64 call, (b) the loop of fnn_canonical_order_f64 over the same matrices - the only way to do
this job without the batch call.  Prints one JSON line: both times, their ratio, the kernel's own time and the derived
microseconds per event per resident workgroup (t_kernel_s * resident / events, resident = min(B, CUs * workgroups that
fit one CU's LDS)).  The floor to meet at n = 64: (a) at least 16 times faster than (b).

    python tools/batch_perf.py [--batch 1024] [--sizes 32,64,128,max,141,256,512,1024] [--loop-problems 0] [--threads 0]
                               [--route auto|global|engine] [--batches 1,4,16,64,256,1024]

--loop-problems K times the loop on the first K problems only and scales (0: all of them); --threads sets
FNN_BATCH_THREADS (256 / 512 / 1024) to compare workgroup sizes; --route sets FNN_BATCH_ROUTE for the batch call (auto:
unset, the call routes by n and batch).

Sizes above fnn_batch_lds_max_n() are the crossover table of the global-memory kernel: for each n and
each B of --batches, the first B of the --batch problems once with FNN_BATCH_ROUTE=global and once with
FNN_BATCH_ROUTE=engine - the loop over one reused handle, the only path for these sizes before the kernel existed - on the
first min(B, K) problems, scaled to B.  Orders are compared problem by problem.  The floor to meet at n = 256, B = 1024: the
kernel's route at least 16 times faster."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastneighbornet_amd as fa  # noqa: E402
from fastneighbornet_amd import _capi  # noqa: E402

LDS_PER_CU, CUS = 163840, 256
GLOBAL_WAVES_PER_CU = 16   # by the registers of k_small_global (profiles/r08/README.md)


def uniform53(a, B, n):
    """B uniform53 matrices, seeds 1 ... B, from the engine's own device generator."""
    D = np.empty((B, n, n))
    with _capi.Handle(a, n) as h:
        for b in range(B):
            h.synth(b + 1, "uniform53")
            D[b] = h.matrix()
    return D


def timed_route(a, route, D, B):
    """One batch call over the first B problems of D under FNN_BATCH_ROUTE=route (None: unset)."""
    n = D.shape[1]
    if route:
        os.environ["FNN_BATCH_ROUTE"] = route
    else:
        os.environ.pop("FNN_BATCH_ROUTE", None)
    try:
        t0 = time.perf_counter()
        orders, _, _, st = _capi.run_batch(a, D.ctypes.data, n, n, n * n, B)
        return time.perf_counter() - t0, orders, st
    finally:
        os.environ.pop("FNN_BATCH_ROUTE", None)


def crossover(a, D, batches, K):
    """The global-memory kernel against the engine loop at one n above the LDS limit, per batch count."""
    n, rows = D.shape[1], []
    timed_route(a, "global", D, min(D.shape[0], 4))       # warm-up: module load, first launch of either route
    timed_route(a, "engine", D, 1)
    for B in batches:
        if B > D.shape[0]:
            continue
        t_g, o_g, st = timed_route(a, "global", D, B)
        Ke = min(B, K) if K > 0 else B
        t_e, o_e, se = timed_route(a, "engine", D, Ke)
        assert st.n_global == B and se.n_fallback == Ke
        # (k_small_global holds 98 VGPRs: four waves per SIMD, 16 per CU - one workgroup of 1024 threads, not the two that LDS admits)
        resident = min(-(-B // st.chunks), CUS * max(1, min(LDS_PER_CU // st.lds_bytes, GLOBAL_WAVES_PER_CU * 64 // st.block_threads)))
        rows.append({
            "n": n, "batch": B, "t_global_s": round(t_g, 6), "t_engine_s": round(t_e * B / Ke, 6), "engine_problems_timed": Ke,
            "speedup": round(t_e * B / Ke / t_g, 2), "t_kernel_s": round(st.t_kernel_s, 6), "t_upload_s": round(st.t_upload_s, 6),
            "chunks": st.chunks, "events": int(st.n_events), "block_threads": st.block_threads, "lds_bytes": st.lds_bytes,
            "resident_workgroups": resident,
            "us_per_event_per_resident_workgroup": round(st.t_kernel_s * 1e6 * resident / max(st.n_events, 1), 3),
            "orders_equal": bool((o_g[:Ke] == o_e).all())})
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--sizes", default="32,64,128,max,141,256,512,1024")
    ap.add_argument("--loop-problems", type=int, default=0)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--route", choices=("auto", "global", "engine"), default="auto")
    ap.add_argument("--batches", default="1,4,16,64,256,1024")
    args = ap.parse_args()
    route = None if args.route == "auto" else args.route
    if args.threads:
        os.environ["FNN_BATCH_THREADS"] = str(args.threads)
    a = fa.api()
    nmax = a.batch_lds_max_n()
    out = {"batch": args.batch, "lds_max_n": nmax, "global_max_n": a.batch_global_max_n(), "route": args.route, "sizes": [], "crossover": []}
    opts = _capi.FnnOpts()
    for tok in args.sizes.split(","):
        n = nmax if tok == "max" else int(tok)
        D = uniform53(a, args.batch, n)
        if n > nmax:
            out["crossover"] += crossover(a, D, [int(b) for b in args.batches.split(",")], args.loop_problems)
            continue
        timed_route(a, route, D, min(args.batch, 8))           # warm-up: module load, first launch
        t_batch, orders, st = timed_route(a, route, D, args.batch)
        K = args.loop_problems if 0 < args.loop_problems < args.batch else args.batch
        one = np.zeros(n + 1, dtype=np.int32)
        a.check(a.canonical_order_f64(D[0].ctypes.data_as(C.POINTER(C.c_double)), n, n, C.byref(opts), one.ctypes.data_as(C.POINTER(C.c_int32)), None))
        same = True
        t0 = time.perf_counter()
        for b in range(K):
            a.check(a.canonical_order_f64(D[b].ctypes.data_as(C.POINTER(C.c_double)), n, n, C.byref(opts),
                                          one.ctypes.data_as(C.POINTER(C.c_int32)), None))
            same = same and bool((one == orders[b]).all())
        t_loop = (time.perf_counter() - t0) * args.batch / K
        resident = min(args.batch, CUS * max(1, min(LDS_PER_CU // st.lds_bytes, 32 * 64 // st.block_threads)))
        out["sizes"].append({
            "n": n, "t_batch_s": round(t_batch, 6), "t_loop_s": round(t_loop, 6), "loop_problems_timed": K,
            "speedup": round(t_loop / t_batch, 2), "t_kernel_s": round(st.t_kernel_s, 6), "t_upload_s": round(st.t_upload_s, 6),
            "events": int(st.n_events), "block_threads": st.block_threads, "lds_bytes": st.lds_bytes, "resident_workgroups": resident,
            "us_per_event_per_resident_workgroup": round(st.t_kernel_s * 1e6 * resident / max(st.n_events, 1), 3),
            "orders_equal": same})
    f64 = [s for s in out["sizes"] if s["n"] == 64]
    if f64:
        out["floor_16x_at_64_met"] = bool(f64[0]["speedup"] >= 16.0)
    f256 = [r for r in out["crossover"] if r["n"] == 256 and r["batch"] == 1024]
    if f256:
        out["floor_16x_at_256_met"] = bool(f256[0]["speedup"] >= 16.0)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

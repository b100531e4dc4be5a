"""Circular split weights of many small problems: the batch call against the loop over fnn_split_weights_f64 (DESIGN.md
section 12).

B uniform53 problems per size, their circular orders from fnn_canonical_order_batch_f64.  For each (n, B): (a) one
fnn_split_weights_batch_f64 call, (b) the loop of fnn_split_weights_f64 over the same problems - the only way to do this job
without the batch call; all B problems are timed at n = 64, the first min(B, 16) elsewhere, scaled to B.  The weights are
compared problem by problem (largest difference relative to max(1, max weight)).  Prints one JSON line per (n, B) on
stderr as it goes and one JSON document at the end.

    python tools/splits_batch_perf.py [--shapes 32:1024,64:1024,128:1024,max:1024,64:1,64:16,64:256] [--loop-problems 16]
                                      [--threads 0]

--threads sets FNN_BATCH_THREADS (256 / 512 / 1024) to compare workgroup sizes.  The batch call runs under
FNN_SW_BATCH_ROUTE=kernel, so that batches below fnn_split_weights_batch_min_batch(n) are timed on the kernel too (that
threshold comes from this table); "default_route" says where the call would send the shape without the switch."""
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


def uniform53(a, B, n):
    """B uniform53 matrices, seeds 1 ... B, from the engine's own device generator."""
    D = np.empty((B, n, n))
    with _capi.Handle(a, n) as h:
        for b in range(B):
            h.synth(b + 1, "uniform53")
            D[b] = h.matrix()
    return D


def one_call(a, D, order):
    n = D.shape[0]
    w = np.zeros(n * (n - 1) // 2)
    st = _capi.FnnSwStats()
    a.check(a.split_weights_f64(D.ctypes.data_as(C.POINTER(C.c_double)), n, n, order.ctypes.data_as(C.POINTER(C.c_int32)), 0,
                                w.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st)))
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32:1024,64:1024,128:1024,max:1024,64:1,64:16,64:256")
    ap.add_argument("--loop-problems", type=int, default=16)
    ap.add_argument("--threads", type=int, default=0)
    args = ap.parse_args()
    if args.threads:
        os.environ["FNN_BATCH_THREADS"] = str(args.threads)
    os.environ["FNN_SW_BATCH_ROUTE"] = "kernel"
    a = fa.api()
    nmax = a.split_weights_batch_max_n()
    out = {"max_n": nmax, "rows": []}
    cache = {}
    for tok in args.shapes.split(","):
        ns, bs = tok.split(":")
        n, B = (nmax if ns == "max" else int(ns)), int(bs)
        if n not in cache or cache[n][0].shape[0] < B:
            D = uniform53(a, B, n)
            cache[n] = (D, np.ascontiguousarray(fa.canonical_order_batch(D), dtype=np.int32))
        D, orders = cache[n][0][:B], cache[n][1][:B]
        _capi.run_splits_batch(a, D.ctypes.data, n, n, n * n, min(B, 4), orders[:min(B, 4)])   # warm-up: module load, first launch
        t0 = time.perf_counter()
        w, sw, st = _capi.run_splits_batch(a, D.ctypes.data, n, n, n * n, B, orders)
        t_batch = time.perf_counter() - t0
        K = B if n == 64 else min(B, args.loop_problems)
        one_call(a, D[0], orders[0])                                                               # warm-up of the one-problem solver
        diff = 0.0
        t0 = time.perf_counter()
        ws = [one_call(a, D[b], orders[b]) for b in range(K)]
        t_loop = (time.perf_counter() - t0) * B / K
        for b in range(K):
            diff = max(diff, float(np.abs(ws[b] - w[b]).max() / max(1.0, np.abs(ws[b]).max())))
        row = {"n": n, "batch": B, "default_route": "kernel" if B >= a.split_weights_batch_min_batch(n) else "loop", "t_batch_s": round(t_batch, 6), "t_loop_s": round(t_loop, 6), "loop_problems_timed": K,
               "speedup": round(t_loop / t_batch, 2), "t_kernel_s": round(st.t_kernel_s, 6), "t_upload_s": round(st.t_upload_s, 6),
               "chunks": st.chunks, "block_threads": st.block_threads, "lds_bytes": st.lds_bytes, "workspace_bytes": st.workspace_bytes,
               "capacity": st.capacity, "n_kernel": st.n_kernel, "n_closed_form": st.n_closed_form, "n_fallback": st.n_fallback,
               "steps_mean": round(float(sw["outer_iterations"].mean()), 1), "free_set_peak_max": int(sw["free_set_peak"].max()),
               "departed_mean": round(float(sw["departed"].mean()), 1), "kkt_max": float(sw["kkt_violation"].max()),
               "max_rel_weight_difference": diff}
        print(json.dumps(row), file=sys.stderr, flush=True)
        out["rows"].append(row)
    out["default_kernel_route_always_faster"] = bool(all(r["speedup"] > 1.0 for r in out["rows"] if r["default_route"] == "kernel"))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

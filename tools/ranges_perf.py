"""Alignment distances over site ranges against the counts route.

A scan of random 4-state alignments at about 10 % divergence with windows of `--width` sites every `--step` sites: n = 32, 64, 140
taxa, L = 10 000, 100 000 and 1 000 000 sites, without and with 2 % missing bytes, models p, k2p and tn93.  For each shape:
  (a) fnn_alignment_distances_ranges_device_f64 into a tensor on the GPU (`range_distances(out="torch")`), the better of two calls;
  (b) what a caller did before: the 0/1 counts of the windows as a numpy array, then
      fnn_alignment_distances_model_batch_device_f64 on them (`alignment_distances_batch(out="torch")`), the better of two calls
      (one call where the counts take more than 1 GB);
and for each the whole route to host orders (fnn_canonical_order_batch_device_f64 on that tensor).  The host clock stops after
calls that have synchronised their stream.  Where both ran, matrices and orders are compared, equal bitwise.  Where the counts of
(b) would not fit into the host's available memory the record says "does not fit"; where they are larger than --b-max-bytes it
says "not run" - in both cases with the byte count.  Prints one JSON line per shape.

    python tools/ranges_perf.py [--sizes 32,64,140] [--sites 10000,100000,1000000] [--missing 0,0.02] [--models p,k2p,tn93]
                                [--width 1000] [--step 250] [--b-max-bytes N] [--out FILE]

--out appends the JSON lines to FILE as well."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # first: torch's HIP runtime then serves the product's library too (as in bench.py)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastneighbornet_amd as fa  # noqa: E402
from dist_perf import alignment  # noqa: E402


def route_a(seq, starts, ends, model):
    t0 = time.perf_counter()
    T, st = fa.range_distances(seq, starts, ends, out="torch", model=model)
    t1 = time.perf_counter()
    orders = fa.canonical_order_batch(T)
    t2 = time.perf_counter()
    return T, orders, st, t1 - t0, t2 - t0


def route_b(seq, starts, ends, model):
    t0 = time.perf_counter()
    s = np.arange(seq.shape[1], dtype=np.int64)[None, :]
    counts = ((starts[:, None] <= s) & (s < ends[:, None])).astype(np.uint16)
    tc = time.perf_counter()
    T, st = fa.alignment_distances_batch(seq, counts, out="torch", model=model)
    t1 = time.perf_counter()
    orders = fa.canonical_order_batch(T)
    t2 = time.perf_counter()
    return T, orders, dict(st, t_counts_s=tc - t0), t1 - t0, t2 - t0


def available_bytes():
    for line in open("/proc/meminfo"):
        if line.startswith("MemAvailable:"):
            return int(line.split()[1]) * 1024
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32,64,140")
    ap.add_argument("--sites", default="10000,100000,1000000")
    ap.add_argument("--missing", default="0,0.02")
    ap.add_argument("--models", default="p,k2p,tn93")
    ap.add_argument("--width", type=int, default=1000)
    ap.add_argument("--step", type=int, default=250)
    ap.add_argument("--b-max-bytes", type=int, default=0, help="skip route (b) where its counts are larger (0: no limit but the host's memory)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    models = args.models.split(",")
    for miss in (0.0, 0.02):   # warm both routes: the runtime, the kernels' code objects
        for model in models:
            w = alignment(8, 512, 1, miss)
            ws, we = fa.window_ranges(512, 100, 25)
            route_a(w, ws, we, model)
            route_b(w, ws, we, model)
    for L in [int(x) for x in args.sites.split(",")]:
        starts, ends = fa.window_ranges(L, args.width, args.step)
        B = len(starts)
        counts_bytes = 2 * B * L
        for miss in [float(x) for x in args.missing.split(",")]:
            for n in [int(x) for x in args.sizes.split(",")]:
                seq = alignment(n, L, 1000 + n + L, miss)
                for model in models:
                    rec = {"model": model, "n": n, "L": L, "B": B, "width": args.width, "step": args.step, "missing": miss, "b_counts_bytes": counts_bytes}
                    a = None
                    for _ in range(2):
                        T, o, st, t_call, t_route = route_a(seq, starts, ends, model)
                        if a is None or t_call < a["t_call"]:
                            a = {"t_call": t_call, "t_route": t_route, "st": st}
                        a["D"], a["o"] = T.cpu().numpy(), o
                        del T
                    st = a["st"]
                    rec.update({"chunks": st["chunks"], "n_site_blocks": st["n_site_blocks"], "n_site_blocks_dense": st["n_site_blocks_dense"],
                                "a_t_kernel_ms": st["t_kernel_s"] * 1e3, "a_t_upload_ms": st["t_upload_s"] * 1e3, "a_t_call_ms": a["t_call"] * 1e3,
                                "a_t_route_ms": a["t_route"] * 1e3, "a_kernel_us_per_window": st["t_kernel_s"] * 1e6 / B})
                    if counts_bytes > 0.5 * available_bytes():
                        rec["b_status"] = "does not fit"
                    elif args.b_max_bytes and counts_bytes > args.b_max_bytes:
                        rec["b_status"] = "not run"
                    else:
                        rec["b_status"] = "ran"
                        b = None
                        for _ in range(2 if counts_bytes <= 10 ** 9 else 1):
                            T, o, st, t_call, t_route = route_b(seq, starts, ends, model)
                            if b is None or t_call < b["t_call"]:
                                b = {"t_call": t_call, "t_route": t_route, "st": st}
                            b["D"], b["o"] = T.cpu().numpy(), o
                            del T
                        rec.update({"b_chunks": b["st"]["chunks"], "b_t_counts_ms": b["st"]["t_counts_s"] * 1e3, "b_t_kernel_ms": b["st"]["t_kernel_s"] * 1e3,
                                    "b_t_upload_ms": b["st"]["t_upload_s"] * 1e3, "b_t_call_ms": b["t_call"] * 1e3, "b_t_route_ms": b["t_route"] * 1e3,
                                    "kernel_b_over_a": b["st"]["t_kernel_s"] / a["st"]["t_kernel_s"], "call_b_over_a": b["t_call"] / a["t_call"],
                                    "route_b_over_a": b["t_route"] / a["t_route"],
                                    "matrices_bitwise_equal": bool((a["D"].view(np.int64) == b["D"].view(np.int64)).all()),
                                    "orders_equal": bool((a["o"] == b["o"]).all())})
                    line = json.dumps(rec)
                    print(line, flush=True)
                    if args.out:
                        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                        with open(args.out, "a") as f:
                            f.write(line + "\n")


if __name__ == "__main__":
    main()

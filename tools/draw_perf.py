"""Bootstrap replicates drawn on the device against the counts route.

B = 1024 bootstrap replicates of random 4-state alignments at about 10 % divergence at section 14's twelve shapes: n = 32, 64,
140 taxa, L = 1000 and 10000 sites, once without and once with 2 % missing bytes.  For each shape, in one run, alternating, the
better of two calls each:
  (a) fnn_bootstrap_distances_batch_device_f64 into a tensor on the GPU (the replicates drawn by k_draw);
  (b) what the call replaces: fnn_bootstrap_counts on the host, then fnn_alignment_distances_batch_device_f64 on those counts
      into a tensor on the GPU;
and for each the whole route from the alignment to host orders (fnn_canonical_order_batch_device_f64 on that tensor).  The host
clock stops after calls that have synchronised their stream.  The matrices and orders of (a) and (b) are compared, equal
bitwise.  Prints one JSON line per shape.

    python tools/draw_perf.py [--batch 1024] [--sizes 32,64,140] [--sites 1000,10000] [--missing 0,0.02] [--model p|jc69|k2p] [--out FILE]

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


def route_a(seq, B, seed, model):
    t0 = time.perf_counter()
    T, st = fa.bootstrap_distances(seq, B, seed, out="torch", model=model)
    t1 = time.perf_counter()
    orders = fa.canonical_order_batch(T)
    t2 = time.perf_counter()
    return T, orders, st, t1 - t0, t2 - t0


def route_b(seq, B, seed, model):
    t0 = time.perf_counter()
    counts = fa.bootstrap_counts(seq.shape[1], B, seed)
    tc = time.perf_counter()
    T, st = fa.alignment_distances_batch(seq, counts, out="torch", model=model)
    t1 = time.perf_counter()
    orders = fa.canonical_order_batch(T)
    t2 = time.perf_counter()
    st = dict(st, t_counts_s=tc - t0)
    return T, orders, st, t1 - t0, t2 - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--sizes", default="32,64,140")
    ap.add_argument("--sites", default="1000,10000")
    ap.add_argument("--missing", default="0,0.02")
    ap.add_argument("--model", default="p", choices=["p", "jc69", "k2p"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, seed = args.batch, 7
    # warm both routes: the runtime, the kernels' code objects
    for miss in (0.0, 0.02):
        route_a(alignment(8, 256, 1, miss), 64, 1, args.model)
        route_b(alignment(8, 256, 1, miss), 64, 1, args.model)
    lines = []
    for miss in [float(x) for x in args.missing.split(",")]:
        for n in [int(x) for x in args.sizes.split(",")]:
            for L in [int(x) for x in args.sites.split(",")]:
                seq = alignment(n, L, 1000 + n + L, miss)
                best = {}
                for _ in range(2):   # (alternating; the better of two runs of each route, by the distance call's time)
                    for name, fn in (("a", route_a), ("b", route_b)):
                        T, o, st, t_call, t_route = fn(seq, B, seed, args.model)
                        if name not in best or t_call < best[name]["t_call"]:
                            best[name] = {"t_call": t_call, "t_route": t_route, "st": st}
                        best[name]["D"], best[name]["o"] = T.cpu().numpy(), o
                        del T
                a, b = best["a"], best["b"]
                rec = {"model": args.model, "n": n, "L": L, "B": B, "missing": miss, "draw_route": a["st"]["draw_route"], "max_count": a["st"]["max_count"],
                       "digit_passes": a["st"]["digit_passes"], "chunks": a["st"]["chunks"],
                       "a_t_draw_ms": a["st"]["t_draw_s"] * 1e3, "a_t_kernel_ms": a["st"]["t_kernel_s"] * 1e3, "a_t_upload_ms": a["st"]["t_upload_s"] * 1e3,
                       "a_t_call_ms": a["t_call"] * 1e3, "a_t_route_ms": a["t_route"] * 1e3,
                       "b_t_counts_ms": b["st"]["t_counts_s"] * 1e3, "b_t_kernel_ms": b["st"]["t_kernel_s"] * 1e3, "b_t_upload_ms": b["st"]["t_upload_s"] * 1e3,
                       "b_t_call_ms": b["t_call"] * 1e3, "b_t_route_ms": b["t_route"] * 1e3,
                       "call_b_over_a": b["t_call"] / a["t_call"], "route_b_over_a": b["t_route"] / a["t_route"],
                       "matrices_bitwise_equal": bool((a["D"].view(np.int64) == b["D"].view(np.int64)).all()),
                       "orders_equal": bool((a["o"] == b["o"]).all())}
                line = json.dumps(rec)
                print(line, flush=True)
                lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

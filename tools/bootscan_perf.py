"""Bootscan in one call against the loop over windows.

A scan of random 4-state alignments at about 10 % divergence with windows of `--width` sites every `--step` sites and `--replicates`
bootstrap replicates inside every window, the window's original data in front: n = 32, 64, 140 taxa, L = 10 000, 100 000 and
1 000 000 sites, without and with 2 % missing bytes, models p, k2p and tn93.  For each shape:
  (a) fnn_bootscan_distances_device_f64 into a tensor on the GPU (`bootscan_distances(out="torch")`), the better of two calls;
  (b) the way to the same bytes before it: `bootstrap_distances(seq[:, s:e], R, seed_w, lead=1, out="torch")` once per window, each
      result copied into its place in one tensor (the better of two loops up to 500 windows, one loop above);
  (c) where the counts fit --c-max-bytes: `bootscan_counts` as a numpy array, then `alignment_distances_batch(out="torch")` on them;
and for (a) and (b) the whole route to host orders (`canonical_order_batch` on the tensor) up to --route-max-problems problems.  The
host clock stops after calls that have synchronised their stream.  Matrices are compared on the GPU, equal bitwise.  A shape whose output
tensor is larger than --max-out-bytes is skipped with a record that says so.  Prints one JSON line per shape.

    python tools/bootscan_perf.py [--sizes 32,64,140] [--sites 10000,100000,1000000] [--missing 0,0.02] [--models p,k2p,tn93]
                                  [--width 1000] [--step 250] [--replicates 100] [--out FILE]

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

M64 = 2 ** 64 - 1


def splitmix64_at(seed, k):
    z = (seed + (k + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def route_a(seq, starts, ends, R, seed, model, orders):
    t0 = time.perf_counter()
    T, st = fa.bootscan_distances(seq, starts, ends, R, seed, lead=1, out="torch", model=model)
    t1 = time.perf_counter()
    if orders:
        fa.canonical_order_batch(T.reshape(-1, T.shape[2], T.shape[3]))
    t2 = time.perf_counter()
    return T, st, t1 - t0, (t2 - t0) if orders else None


def route_b(seq, starts, ends, R, seed, model, orders):
    n, W = seq.shape[0], len(starts)
    t0 = time.perf_counter()
    T = torch.empty((W, R + 1, n, n), dtype=torch.float64, device="cuda:0")
    t_draw = t_kernel = 0.0
    for w in range(W):
        D, st = fa.bootstrap_distances(np.ascontiguousarray(seq[:, starts[w]:ends[w]]), R, splitmix64_at(seed & M64, w), lead=1, out="torch", model=model)
        T[w] = D
        t_draw += st["t_draw_s"]
        t_kernel += st["t_kernel_s"]
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    if orders:
        fa.canonical_order_batch(T.reshape(-1, n, n))
    t2 = time.perf_counter()
    return T, {"t_draw_s": t_draw, "t_kernel_s": t_kernel}, t1 - t0, (t2 - t0) if orders else None


def route_c(seq, starts, ends, R, seed, model):
    t0 = time.perf_counter()
    counts = fa.bootscan_counts(seq.shape[1], starts, ends, R, seed, lead=1)
    tc = time.perf_counter()
    T, st = fa.alignment_distances_batch(seq, counts, out="torch", model=model)
    t1 = time.perf_counter()
    return T, dict(st, t_counts_s=tc - t0), t1 - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32,64,140")
    ap.add_argument("--sites", default="10000,100000,1000000")
    ap.add_argument("--missing", default="0,0.02")
    ap.add_argument("--models", default="p,k2p,tn93")
    ap.add_argument("--width", type=int, default=1000)
    ap.add_argument("--step", type=int, default=250)
    ap.add_argument("--replicates", type=int, default=100)
    ap.add_argument("--seed", type=int, default=2021)
    ap.add_argument("--max-out-bytes", type=int, default=16 * 10 ** 9)
    ap.add_argument("--c-max-bytes", type=int, default=2 * 10 ** 9)
    ap.add_argument("--route-max-problems", type=int, default=50000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    models, R = args.models.split(","), args.replicates
    for miss in (0.0, 0.02):   # warm every route: the runtime, the kernels' code objects
        for model in models:
            w = alignment(8, 512, 1, miss)
            ws, we = fa.window_ranges(512, 100, 25)
            route_a(w, ws, we, 3, 1, model, True)
            route_b(w, ws, we, 3, 1, model, True)
            route_c(w, ws, we, 3, 1, model)
    for L in [int(x) for x in args.sites.split(",")]:
        starts, ends = fa.window_ranges(L, args.width, args.step)
        W = len(starts)
        B = W * (R + 1)
        for miss in [float(x) for x in args.missing.split(",")]:
            for n in [int(x) for x in args.sizes.split(",")]:
                out_bytes = 8 * B * n * n
                if out_bytes > args.max_out_bytes:
                    rec = {"n": n, "L": L, "W": W, "R": R, "missing": miss, "status": "skipped: the output tensor is larger than --max-out-bytes",
                           "out_bytes": out_bytes}
                    print(json.dumps(rec), flush=True)
                    if args.out:
                        with open(args.out, "a") as f:
                            f.write(json.dumps(rec) + "\n")
                    continue
                seq = alignment(n, L, 1000 + n + L, miss)
                orders = B <= args.route_max_problems
                for model in models:
                    rec = {"model": model, "n": n, "L": L, "W": W, "R": R, "problems": B, "width": args.width, "step": args.step, "missing": miss,
                           "status": "ran", "c_counts_bytes": 2 * B * L}
                    a = None
                    for _ in range(2):
                        T, st, t_call, t_route = route_a(seq, starts, ends, R, args.seed, model, orders)
                        if a is None or t_call < a["t_call"]:
                            a = {"t_call": t_call, "t_route": t_route, "st": st}
                        a["T"] = T
                        del T
                    st = a["st"]
                    rec.update({"chunks": st["chunks"], "n_host_chunks": st["n_host_chunks"], "max_count": st["max_count"],
                                "n_site_blocks": st["n_site_blocks"], "n_site_blocks_dense": st["n_site_blocks_dense"],
                                "a_t_draw_ms": st["t_draw_s"] * 1e3, "a_t_kernel_ms": st["t_kernel_s"] * 1e3, "a_t_upload_ms": st["t_upload_s"] * 1e3,
                                "a_t_call_ms": a["t_call"] * 1e3, "a_t_route_ms": a["t_route"] * 1e3 if orders else None})
                    b = None
                    for _ in range(2 if W <= 500 else 1):
                        T, st, t_call, t_route = route_b(seq, starts, ends, R, args.seed, model, orders)
                        if b is None or t_call < b["t_call"]:
                            b = {"t_call": t_call, "t_route": t_route, "st": st}
                        b["T"] = T
                        del T
                    rec.update({"b_t_draw_ms": b["st"]["t_draw_s"] * 1e3, "b_t_kernel_ms": b["st"]["t_kernel_s"] * 1e3, "b_t_call_ms": b["t_call"] * 1e3,
                                "b_t_route_ms": b["t_route"] * 1e3 if orders else None, "call_b_over_a": b["t_call"] / a["t_call"],
                                "route_b_over_a": b["t_route"] / a["t_route"] if orders else None,
                                "b_matrices_bitwise_equal": torch.equal(a["T"].view(torch.int64), b["T"].view(torch.int64))})
                    del b
                    if 2 * B * L <= args.c_max_bytes:
                        T, st, t_call = route_c(seq, starts, ends, R, args.seed, model)
                        rec.update({"c_t_counts_ms": st["t_counts_s"] * 1e3, "c_t_kernel_ms": st["t_kernel_s"] * 1e3, "c_t_call_ms": t_call * 1e3,
                                    "call_c_over_a": t_call / a["t_call"],
                                    "c_matrices_bitwise_equal": torch.equal(a["T"].view(torch.int64).reshape(-1), T.view(torch.int64).reshape(-1))})
                        del T
                    else:
                        rec["c_status"] = "not run: the counts are larger than --c-max-bytes"
                    del a
                    line = json.dumps(rec)
                    print(line, flush=True)
                    if args.out:
                        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                        with open(args.out, "a") as f:
                            f.write(line + "\n")


if __name__ == "__main__":
    main()

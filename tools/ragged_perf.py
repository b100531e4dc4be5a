"""Ragged batches: one call for problems of different sizes against the best a caller could do without it (DESIGN.md
section 13).

`--count` uniform53 problems whose sizes are drawn uniformly from lo ... hi by `--seed`, for every lo:hi of `--ranges`.  Both
halves of a run - the circular orders, then the split weights of those orders - are timed separately, all problems timed, for

  (a) ragged    one fnn_canonical_order_ragged_f64 / fnn_split_weights_ragged_f64 call
  (b) grouped   the problems grouped by size (stacked before the clock starts) and the same-size entry called once per
                distinct size; the weights once by the call's own rule (groups below fnn_split_weights_batch_min_batch(n) go
                problem by problem through the one-problem solver) and once with FNN_SW_BATCH_ROUTE=kernel (every group on
                the kernel: the faster of the two is the figure to beat)

Each leg is warmed up once and then timed `--reps` times, the legs taking turns; the figure is the median, the spread is
reported.  The results of (a) and (b) are compared problem by problem.  `--grouped-only` runs (b) alone and needs nothing of
the ragged calls: that is how leg (b) is taken from a build without them.  Unless `--grouped-only`, the size classes of (a)
are listed per half: block size and LDS per launch (from one-problem calls' statistics), the workgroups that fit a CU at a
time (160 KiB of LDS, 2048 threads), the problems in the class and the kernel time of the class launched alone.

    python tools/ragged_perf.py [--ranges 8:140,8:64] [--count 1024] [--seed 7] [--reps 3] [--grouped-only] [--streams N]
                                [--skip LEG,LEG]

--streams sets FNN_RAGGED_STREAMS (1 ... 4); --skip leaves legs out (grouped_orders, grouped_weights_default_route,
grouped_weights_kernel_route, ragged_orders, ragged_weights).  Prints one JSON line per range on stderr as it goes and one JSON document at the
end."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastneighbornet_amd as fa  # noqa: E402
from fastneighbornet_amd import _capi  # noqa: E402

CU_LDS_BYTES, CU_THREADS = 163840, 2048


def problems(a, sizes):
    """One uniform53 matrix per entry of sizes, seed = index + 1, from the engine's own device generator."""
    mats = [None] * len(sizes)
    for n in sorted(set(sizes)):
        with _capi.Handle(a, n) as h:
            for b in [b for b, m in enumerate(sizes) if m == n]:
                h.synth(b + 1, "uniform53")
                mats[b] = h.matrix()
    return mats


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def summary(ts):
    return {"median_s": round(statistics.median(ts), 6), "min_s": round(min(ts), 6), "max_s": round(max(ts), 6)}


def class_table(half, sizes, mats, orders):
    """The size classes of the ragged call for this half, from the product's own statistics."""
    def call(idx):
        if half == "orders":
            return _capi.run_ragged(fa.api(), *fa.canonical.ragged_layout([mats[b] for b in idx])[:4])[3]
        base, off, ns, lds = fa.canonical.ragged_layout([mats[b] for b in idx])[:4]
        return _capi.run_splits_ragged(fa.api(), base, off, ns, [orders[b] for b in idx], lds)[2]
    os.environ["FNN_SW_BATCH_ROUTE"] = "kernel"                     # (one problem of 140 taxa is below the default crossover)
    shape = {}
    for n in sorted(set(sizes)):
        if n >= (4 if half == "orders" else 2):
            st = call([sizes.index(n)])
            if st.chunks == 1:
                r = min(CU_LDS_BYTES // st.lds_bytes, CU_THREADS // st.block_threads)
                shape[n] = (st.block_threads, 1 << (r.bit_length() - 1))
    rows = []
    for key in sorted(set(shape.values()), key=lambda k: (-k[0], k[1])):
        members = [n for n in shape if shape[n] == key]
        idx = [b for b, n in enumerate(sizes) if n in members]
        call(idx)
        st = call(idx)
        rows.append({"n_from": min(members), "n_to": max(members), "problems": len(idx), "launches": st.chunks, "block_threads": st.block_threads,
                     "lds_bytes": st.lds_bytes, "workgroups_per_cu": min(CU_LDS_BYTES // st.lds_bytes, CU_THREADS // st.block_threads),
                     "t_kernel_alone_s": round(st.t_kernel_s, 6)})
    os.environ.pop("FNN_SW_BATCH_ROUTE", None)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranges", default="8:140,8:64")
    ap.add_argument("--count", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--grouped-only", action="store_true")
    ap.add_argument("--streams", type=int, default=0)
    ap.add_argument("--skip", default="", help="comma-separated legs to leave out, e.g. grouped_weights_default_route")
    args = ap.parse_args()
    if args.streams:
        os.environ["FNN_RAGGED_STREAMS"] = str(args.streams)
    a = fa.api()
    out = {"count": args.count, "seed": args.seed, "reps": args.reps, "streams": args.streams or "default", "rows": []}
    for tok in args.ranges.split(","):
        lo, hi = (int(x) for x in tok.split(":"))
        sizes = [int(n) for n in np.random.default_rng(args.seed).integers(lo, hi + 1, args.count)]
        mats = problems(a, sizes)
        groups = {n: [b for b, m in enumerate(sizes) if m == n] for n in sorted(set(sizes))}
        stacks = {n: np.stack([mats[b] for b in idx]) for n, idx in groups.items()}   # (the caller's grouping is not timed)

        def grouped_orders():
            return {n: fa.canonical_order_batch(stacks[n]) for n in groups}

        def grouped_weights(o, route=None):
            if route:
                os.environ["FNN_SW_BATCH_ROUTE"] = route
            try:
                return {n: fa.split_weights_batch(stacks[n], o[n]) for n in groups}
            finally:
                os.environ.pop("FNN_SW_BATCH_ROUTE", None)

        legs = {"grouped_orders": grouped_orders}
        g_orders = grouped_orders()                                                     # warm-up, and the orders the weight legs use
        legs["grouped_weights_default_route"] = lambda: grouped_weights(g_orders)
        legs["grouped_weights_kernel_route"] = lambda: grouped_weights(g_orders, "kernel")
        orders = [None] * args.count
        for n, idx in groups.items():
            for k, b in enumerate(idx):
                orders[b] = np.ascontiguousarray(g_orders[n][k], dtype=np.int32)
        if not args.grouped_only:
            legs["ragged_orders"] = lambda: fa.canonical_order_ragged(mats)
            legs["ragged_weights"] = lambda: fa.split_weights_ragged(mats, orders)
        for k in args.skip.split(","):
            legs.pop(k, None)
        times, last = {k: [] for k in legs}, {}
        for k, fn in legs.items():
            if k != "grouped_orders":
                fn()                                                                    # warm-up
        for _ in range(args.reps):                                                      # the legs take turns
            for k, fn in legs.items():
                t, last[k] = timed(fn)
                times[k].append(t)
        row = {"n_from": lo, "n_to": hi, "problems": args.count, "distinct_sizes": len(groups), "entries": sum(n * n for n in sizes),
               "times": {k: summary(v) for k, v in times.items()}}
        gw = {k: last[k] for k in last if k.startswith("grouped_weights")}
        row["grouped_weights_fallbacks"] = {k: int(sum(v[n][1]["call"]["n_fallback"] for n in groups)) for k, v in gw.items()}
        if not args.grouped_only:
            ro, (rw, rs) = last["ragged_orders"], last["ragged_weights"]
            row["orders_equal"] = bool(all((ro[b] == orders[b]).all() for b in range(args.count)))
            kern = last.get("grouped_weights_kernel_route") or {}
            diff, same = 0.0, 0
            for n, idx in (groups.items() if kern else ()):
                for k, b in enumerate(idx):
                    w = kern[n][0][k]
                    diff = max(diff, float(np.abs(w - rw[b]).max() / max(1.0, np.abs(w).max())) if w.size else 0.0)
                    same += int(w.tobytes() == rw[b].tobytes())
            if kern:
                row["weights_bit_equal_to_grouped_kernel_route"] = same
                row["weights_max_rel_difference"] = diff
            row["ragged_weights_call"] = {k: rs["call"][k] for k in ("chunks", "n_kernel", "n_closed_form", "n_fallback", "block_threads", "lds_bytes", "t_kernel_s", "t_upload_s")}
            st = _capi.run_ragged(a, *fa.canonical.ragged_layout(mats)[:4])[3]
            row["ragged_orders_call"] = {k: getattr(st, k) for k in ("chunks", "n_lds", "n_global", "n_fallback", "block_threads", "lds_bytes", "t_kernel_s", "t_upload_s")}
            best_w = min([row["times"][k]["median_s"] for k in row["times"] if k.startswith("grouped_weights")], default=None)
            if "grouped_orders" in row["times"]:
                row["speedup_orders"] = round(row["times"]["grouped_orders"]["median_s"] / row["times"]["ragged_orders"]["median_s"], 2)
            if best_w is not None:
                row["speedup_weights"] = round(best_w / row["times"]["ragged_weights"]["median_s"], 2)
            if "grouped_orders" in legs:                                                # (left out of a run that times the ragged legs alone)
                row["classes_orders"] = class_table("orders", sizes, mats, orders)
                row["classes_weights"] = class_table("weights", sizes, mats, orders)
        print(json.dumps(row), file=sys.stderr, flush=True)
        out["rows"].append(row)
    if not args.grouped_only:
        out["ragged_not_slower"] = bool(all(r.get("speedup_orders", 1.0) >= 1.0 and r.get("speedup_weights", 1.0) >= 1.0 for r in out["rows"]))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

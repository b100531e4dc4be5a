"""Split support of a bootstrap run: the table on the device against numpy on the host.

B = 1024 bootstrap replicates (fa.bootstrap: distances, orders and split weights on the device) of random 4-state alignments at
about 10 % divergence, n = 32, 64, 140 taxa, L = 1000 sites.  For each shape, on the orders and weights that bootstrap() returns:
  (a)  split_support on the host arrays, kernel route, the whole call;
  (a') the same on a torch tensor on the GPU (the device entry);
  (h)  the host route (an ordered map in plain C++);
  (b)  what a user of the library without this stage does: the same table from numpy in its best vectorised form -
       positives -> (i, j) -> prefix bitsets gathered per record -> fold -> np.unique(axis=0, return_inverse=True) ->
       bincount / np.add.at - on the threads the machine gives.
The tables of (a), (a') and (h) must be equal byte for byte.  (b)'s keys and counts must be equal as sets; its sums may differ
in the last bits, because the order of np.add.at is not the contract: the number of differing sums is reported, not fixed.
Prints one JSON line per shape: the three calls, (b), (b) / (a), the stages of the kernel route and what bootstrap() itself takes.

    python tools/support_perf.py [--batch 1024] [--sizes 32,64,140] [--sites 1000] [--out FILE] [--only-a]
    python tools/support_perf.py --crossover 2,4,8,16,32,64,128,256 [--sizes 32,64,140] [--out FILE]

--only-a runs route (a) alone (for a kernel trace of one shape); --out appends the JSON lines to FILE as well; --crossover times
the kernel route against the host route on the first B problems of one run per n (where fnn_split_support_min_work() comes from)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # first: torch's HIP runtime then serves the product's library too (as in bench.py)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastneighbornet_amd as fa  # noqa: E402


def alignment(n, L, seed):
    r = np.random.default_rng(seed)
    base = r.integers(0, 4, L)
    seq = np.where(r.random((n, L)) < 0.1, r.integers(0, 4, (n, L)), base[None, :])
    return np.frombuffer(b"ACGT", dtype=np.uint8)[seq].copy()


def numpy_table(orders, W, threshold, lead):
    """(keys (S, words) uint64, count, weight_sum), rows in np.unique's order (sorted by key)."""
    B, n = orders.shape[0], orders.shape[1] - 1
    words = (n + 63) // 64
    b, k = np.nonzero(W > threshold)
    iu, ju = np.triu_indices(n, 1)
    i, j = iu[k], ju[k]
    # prefix bitsets of every problem: P[b, p, w] = taxa at positions 1 ... p
    t = orders[:, 1:].astype(np.int64) - 1
    one = np.zeros((B, n, words), dtype=np.uint64)
    np.put_along_axis(one, (t // 64)[:, :, None], (np.uint64(1) << (t % 64).astype(np.uint64))[:, :, None], axis=2)
    P = np.zeros((B, n + 1, words), dtype=np.uint64)
    np.bitwise_or.accumulate(one, axis=1, out=P[:, 1:, :])
    keys = P[b, j] ^ P[b, i]
    flip = (keys[:, 0] & np.uint64(1)).astype(bool)
    mask = np.full(words, ~np.uint64(0), dtype=np.uint64)
    if n % 64:
        mask[-1] = (np.uint64(1) << np.uint64(n % 64)) - np.uint64(1)
    keys[flip] = ~keys[flip] & mask
    uniq, inv = np.unique(keys, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    tally = b >= lead
    count = np.bincount(inv[tally], minlength=len(uniq))
    wsum = np.zeros(len(uniq))
    np.add.at(wsum, inv[tally], W[b[tally], k[tally]])
    return uniq, count, wsum


def timed(f, reps=2):
    best, out = None, None
    for _ in range(reps):   # (the better of two runs)
        t0 = time.perf_counter()
        out = f()
        dt = time.perf_counter() - t0
        best = dt if best is None or dt < best else best
    return best, out


def with_route(route, f):
    old = os.environ.get("FNN_SUPPORT_ROUTE")
    os.environ["FNN_SUPPORT_ROUTE"] = route
    try:
        return f()
    finally:
        if old is None:
            del os.environ["FNN_SUPPORT_ROUTE"]
        else:
            os.environ["FNN_SUPPORT_ROUTE"] = old


def crossover(args, thr, lead):
    """Where the kernel route starts to win: both routes on the first `batch` problems of one bootstrap run per n, the better
    of three runs each; one JSON line per (n, batch) with batch * n * n next to the two times."""
    batches = [int(x) for x in args.crossover.split(",")]
    lines = []
    for n in [int(x) for x in args.sizes.split(",")]:
        orders, W, _ = fa.bootstrap(alignment(n, 1000, 2000 + n), max(batches), 7)
        with_route("kernel", lambda: fa.split_support(orders[:4], W[:4], thr, lead))
        for b in batches:
            o, w = np.ascontiguousarray(orders[:b]), np.ascontiguousarray(W[:b])
            tk, (_, sk) = timed(lambda: with_route("kernel", lambda: fa.split_support(o, w, thr, lead)), reps=3)
            th, (_, sh) = timed(lambda: with_route("host", lambda: fa.split_support(o, w, thr, lead)), reps=3)
            line = json.dumps({"crossover": True, "n": n, "B": b, "work": b * n * n, "records": sk["n_records"], "t_kernel_route_ms": tk * 1e3,
                               "t_host_route_ms": th * 1e3, "kernel_method": sk["method"], "host_method": sh["method"],
                               "default_takes_kernel": bool(b * n * n >= fa.api().split_support_min_work())})
            print(line, flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--sizes", default="32,64,140")
    ap.add_argument("--sites", default="1000")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-a", action="store_true")
    ap.add_argument("--crossover", default=None, help="batches, e.g. 4,8,16,32,64,128: kernel route against host route per n")
    args = ap.parse_args()
    B, thr, lead = args.batch, 1e-6, 0
    if args.crossover:
        return crossover(args, thr, lead)
    # warm every route: the runtime, the kernels' code objects, numpy's thread pool
    o0, w0, _ = fa.bootstrap(alignment(12, 256, 1), 64, 1)
    with_route("kernel", lambda: fa.split_support(o0, w0))
    with_route("kernel", lambda: fa.split_support(o0, torch.from_numpy(w0).to("cuda:0")))
    numpy_table(o0, w0, thr, lead)
    lines = []
    for n in [int(x) for x in args.sizes.split(",")]:
        for L in [int(x) for x in args.sites.split(",")]:
            seq = alignment(n, L, 1000 + n + L)
            t_boot, (orders, W, _) = timed(lambda: fa.bootstrap(seq, B, 7), reps=1 if args.only_a else 2)
            ta, (tab_a, st) = timed(lambda: with_route("kernel", lambda: fa.split_support(orders, W, thr, lead)))
            rec = {"n": n, "L": L, "B": B, "records": st["n_records"], "splits": st["n_splits"], "words": st["words"], "chunks": st["chunks"],
                   "table_slots": st["table_slots"], "hash_retries": st["hash_retries"], "method": st["method"],
                   "t_kernels_ms": st["t_kernel_s"] * 1e3, "t_upload_ms": st["t_upload_s"] * 1e3, "t_call_ms": st["t_total_s"] * 1e3,
                   "t_a_ms": ta * 1e3, "t_bootstrap_ms": t_boot * 1e3, "weight_bytes": int(W.nbytes)}
            if not args.only_a:
                Wg = torch.from_numpy(W).to("cuda:0")
                torch.cuda.synchronize()
                tg, (tab_g, stg) = timed(lambda: with_route("kernel", lambda: fa.split_support(orders, Wg, thr, lead)))
                th, (tab_h, sth) = timed(lambda: with_route("host", lambda: fa.split_support(orders, W, thr, lead)))
                tb, (uk, uc, us) = timed(lambda: numpy_table(orders, W, thr, lead))
                same = all(tab_a[k].tobytes() == tab_g[k].tobytes() == tab_h[k].tobytes() for k in tab_a)
                # (b) against (a): as sets of (key, count); the sums where the keys meet
                order = np.lexsort(tab_a["keys"].T[::-1])
                ak, ac, asum = tab_a["keys"][order], tab_a["count"][order], tab_a["weight_sum"][order]
                sets_equal = ak.shape == uk.shape and bool((ak == uk).all()) and bool((ac == uc).all())
                rec.update({"t_a_device_ms": tg * 1e3, "t_a_device_kernels_ms": stg["t_kernel_s"] * 1e3, "t_host_route_ms": th * 1e3,
                            "t_b_numpy_ms": tb * 1e3, "ratio_b_over_a": tb / ta, "ratio_host_over_a": th / ta,
                            "tables_bytewise_equal": bool(same), "host_method": sth["method"],
                            "numpy_keys_and_counts_equal": sets_equal,
                            "numpy_sums_differing": int((asum.view(np.int64) != us.view(np.int64)).sum()) if sets_equal else -1,
                            "numpy_sums_max_rel_diff": float(np.max(np.abs(asum - us) / np.maximum(np.abs(asum), 1e-300))) if sets_equal and len(us) else 0.0})
                del Wg
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Bootstrap replicates from an alignment: distance matrices on the device against numpy on the host.

B = 1024 bootstrap replicates of random 4-state alignments at about 10 % divergence, n = 32, 64, 140 taxa, L = 1000 and
10000 sites, once without and once with 2 % missing bytes.  For each shape:
  (a) the product's route from a host alignment to host orders: fnn_alignment_distances_batch_device_f64 into a tensor on
      the GPU, then fnn_canonical_order_batch_device_f64 on that tensor;
  (b) what a user does without the distance call: the same B matrices with numpy in its best form - the 0/1 pair-by-site
      matrix times counts^T as ONE float64 matmul (two with missing bytes), on the threads the machine gives -, then
      fnn_canonical_order_batch_f64 through the host entry.
Matrices and orders of (a) and (b) are compared, equal bitwise.  Prints one JSON line per shape: the kernel's time, the
distance call's time, both routes and their ratio.  The condition: (a) faster than (b) at every shape.

--model jc69 | k2p runs both routes with that corrected distance - (b) then adds the transition matmul
and numpy's log1p, so its matrices agree to rounding, not bitwise: the largest relative difference is reported - and puts the
kernel times of all three models of the same run side by side (t_kernel_p_ms, t_kernel_jc69_ms, t_kernel_k2p_ms).

--model f81 | felsenstein84 | tn93 | logdet does the same on the 4 x 4 tables of state pairs - (b) then is numpy's
sixteen float64 matmuls, one per cell, plus numpy's logarithms - and puts the kernel's time beside the p and K2P kernels' of the
same run (t_kernel_p_ms, t_kernel_k2p_ms, t_kernel_<model>_ms).

--gamma SHAPE (with --model jc69 | k2p | f81 | felsenstein84 | tn93) runs route (a) with gamma-distributed
rates of that shape.  Route (b) then is what a user had to do before the shape existed: `pair_counts_batch` to the host (16 int64
per pair and replicate), the gamma formula with numpy's log1p and expm1 on 16 threads, `canonical_order_batch` on the host
matrices.  The gamma kernel's time stands beside the equal-rates kernel's of the same run (t_kernel_<model>_ms,
t_kernel_<model>_gamma_ms).

    python tools/dist_perf.py [--batch 1024] [--sizes 32,64,140] [--sites 1000,10000] [--missing 0,0.02] [--out FILE]
                              [--only-a] [--model p|jc69|k2p|f81|felsenstein84|tn93|logdet] [--gamma SHAPE]

--only-a runs route (a) alone (for a kernel trace of one shape); --out appends the JSON lines to FILE as well."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # first: torch's HIP runtime then serves the product's library too (as in bench.py)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastneighbornet_amd as fa  # noqa: E402


def alignment(n, L, seed, missing):
    r = np.random.default_rng(seed)
    base = r.integers(0, 4, L)
    seq = np.where(r.random((n, L)) < 0.1, r.integers(0, 4, (n, L)), base[None, :])
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[seq].copy()
    if missing:
        seq[r.random((n, L)) < missing] = 255
    return seq


def route_a(seq, counts, model="p", gamma=None):
    t0 = time.perf_counter()
    T, st = fa.alignment_distances_batch(seq, counts, out="torch", model=model, gamma_shape=gamma)
    t1 = time.perf_counter()
    orders = fa.canonical_order_batch(T)
    t2 = time.perf_counter()
    return T, orders, st, t1 - t0, t2 - t0


PAIR_MODELS = ("f81", "felsenstein84", "tn93", "logdet")


def numpy_pair_model(si, sj, w, model):
    """pairs x B distances from the sixteen cells of every pair's table, each one float64 matmul (exact: integers below 2^53)."""
    code = np.full(256, 255, dtype=np.uint8)
    code[[65, 67, 71, 84]] = (0, 1, 2, 3)
    ci, cj = code[si], code[sj]
    F = [[((ci == s) & (cj == t)).astype(np.float64) @ w for t in range(4)] for s in range(4)]
    r = [F[s][0] + F[s][1] + F[s][2] + F[s][3] for s in range(4)]
    c = [F[0][t] + F[1][t] + F[2][t] + F[3][t] for t in range(4)]
    v = r[0] + r[1] + r[2] + r[3]
    if model == "logdet":
        M = np.stack([np.stack([F[s][t] / v for t in range(4)], axis=-1) for s in range(4)], axis=-2)   # pairs x B x 4 x 4
        ls = sum(np.log(r[s] / v) + np.log(c[s] / v) for s in range(4))
        return -0.25 * (np.log(np.linalg.det(M)) - 0.5 * ls)
    g = [(r[s] + c[s]) / (2.0 * v) for s in range(4)]
    mism = v - (F[0][0] + F[1][1] + F[2][2] + F[3][3])
    if model == "f81":
        E = 1.0 - (g[0] * g[0] + g[1] * g[1] + g[2] * g[2] + g[3] * g[3])
        return -E * np.log1p(-(mism / v) / E)
    P1, P2 = (F[0][2] + F[2][0]) / v, (F[1][3] + F[3][1]) / v
    Q = mism / v - P1 - P2
    gR, gY = g[0] + g[2], g[1] + g[3]
    if model == "felsenstein84":
        A = g[1] * g[3] / gY + g[0] * g[2] / gR
        Bq = g[1] * g[3] + g[0] * g[2]
        Cq = gR * gY
        return -2.0 * A * np.log1p(-(P1 + P2) / (2.0 * A) - (A - Bq) * Q / (2.0 * A * Cq)) + 2.0 * (A - Bq - Cq) * np.log1p(-Q / (2.0 * Cq))
    k1, k2 = 2.0 * g[0] * g[2] / gR, 2.0 * g[3] * g[1] / gY
    k3 = 2.0 * (gR * gY - g[0] * g[2] * gY / gR - g[3] * g[1] * gR / gY)
    return -k1 * np.log1p(-P1 / k1 - Q / (2.0 * gR)) - k2 * np.log1p(-P2 / k2 - Q / (2.0 * gY)) - k3 * np.log1p(-Q / (2.0 * gR * gY))


def numpy_matrices(seq, counts, model="p"):
    n, B = seq.shape[0], counts.shape[0]
    iu, ju = np.triu_indices(n, 1)
    w = counts.astype(np.float64).T                                   # L x B
    si, sj = seq[iu], seq[ju]
    if model in PAIR_MODELS:
        d = numpy_pair_model(si, sj, w, model).T
        D = np.zeros((B, n, n))
        D[:, iu, ju] = d
        D[:, ju, iu] = d
        return D
    if (seq == 255).any():
        both = (si != 255) & (sj != 255)
        valid = both.astype(np.float64) @ w                           # pairs x B, exact: integers below 2^53
        mism = (both & (si != sj)).astype(np.float64) @ w
    else:
        mism = (si != sj).astype(np.float64) @ w
        valid = np.broadcast_to(w.sum(axis=0)[None, :], mism.shape)
    if model == "jc69":
        d = -(0.75 * np.log1p(-(4.0 * mism) / (3.0 * valid)))
    elif model == "k2p":                                              # (ACGT: the bytes' own transitions are A <-> G and C <-> T)
        code = np.zeros(256, dtype=np.uint8)
        code[[65, 67, 71, 84]] = (0, 1, 2, 3)
        pres = (si != 255) & (sj != 255)
        ts = (pres & ((code[si] ^ code[sj]) == 2)).astype(np.float64) @ w
        tv = mism - ts
        d = 0.5 * -np.log1p(-(2.0 * ts + tv) / valid) + 0.25 * -np.log1p(-(2.0 * tv) / valid)
    else:
        d = mism / valid
    d = d.T                                                           # B x pairs
    D = np.zeros((B, n, n))
    D[:, iu, ju] = d
    D[:, ju, iu] = d
    return D


GAMMA_THREADS = 16


def numpy_gamma_from_tables(F, model, alpha):
    """(b, n, n) distances of a slice of replicates from its int64 tables (b, n, n, 4, 4) with numpy's log1p and expm1."""
    F = F.astype(np.float64)
    n = F.shape[1]

    def g(y):
        with np.errstate(invalid="ignore", divide="ignore"):              # (the diagonal's zero tables; overwritten below)
            return alpha * np.expm1(-np.log1p(-y) / alpha)
    r, c = F.sum(axis=4), F.sum(axis=3)
    v = r.sum(axis=3)
    v = np.where(v == 0.0, 1.0, v)                                    # (the diagonal: zero tables)
    mism = v - np.trace(F, axis1=3, axis2=4)
    fr = (r + c) / (2.0 * v[..., None])
    fr = np.where(fr == 0.0, 0.25, fr)
    gA, gC, gG, gT = fr[..., 0], fr[..., 1], fr[..., 2], fr[..., 3]
    P1, P2 = (F[..., 0, 2] + F[..., 2, 0]) / v, (F[..., 1, 3] + F[..., 3, 1]) / v
    Q = mism / v - P1 - P2
    gR, gY = gA + gG, gC + gT
    if model == "jc69":
        D = 0.75 * g(4.0 * mism / (3.0 * v))
    elif model == "k2p":
        D = 0.5 * g(2.0 * (P1 + P2) + Q) + 0.25 * g(2.0 * Q)
    elif model == "f81":
        E = 1.0 - (gA * gA + gC * gC + gG * gG + gT * gT)
        D = E * g((mism / v) / E)
    elif model == "felsenstein84":
        A = gC * gT / gY + gA * gG / gR
        Bq = gC * gT + gA * gG
        Cq = gR * gY
        D = 2.0 * A * g((P1 + P2) / (2.0 * A) + (A - Bq) * Q / (2.0 * A * Cq)) - 2.0 * (A - Bq - Cq) * g(Q / (2.0 * Cq))
    else:
        k1, k2 = 2.0 * gA * gG / gR, 2.0 * gT * gC / gY
        k3 = 2.0 * (gR * gY - gA * gG * gY / gR - gT * gC * gR / gY)
        D = k1 * g(P1 / k1 + Q / (2.0 * gR)) + k2 * g(P2 / k2 + Q / (2.0 * gY)) + k3 * g(Q / (2.0 * gR * gY))
    D[:, np.arange(n), np.arange(n)] = 0.0
    return D


def route_b_gamma(seq, counts, model, alpha):
    """The parent's offer: the tables to the host, numpy's gamma formula on GAMMA_THREADS threads, the orders of the host matrices."""
    from concurrent.futures import ThreadPoolExecutor
    t0 = time.perf_counter()
    F, _ = fa.pair_counts_batch(seq, counts)
    t1 = time.perf_counter()
    B = F.shape[0]
    D = np.empty(F.shape[:3], dtype=np.float64)
    cuts = np.linspace(0, B, GAMMA_THREADS + 1).astype(int)

    def part(k):
        D[cuts[k]:cuts[k + 1]] = numpy_gamma_from_tables(F[cuts[k]:cuts[k + 1]], model, alpha)
    with ThreadPoolExecutor(GAMMA_THREADS) as ex:
        list(ex.map(part, range(GAMMA_THREADS)))
    t2 = time.perf_counter()
    orders = fa.canonical_order_batch(D)
    t3 = time.perf_counter()
    return D, orders, t1 - t0, t2 - t0, t3 - t0


def route_b(seq, counts, model="p"):
    t0 = time.perf_counter()
    D = numpy_matrices(seq, counts, model)
    t1 = time.perf_counter()
    orders = fa.canonical_order_batch(D)
    t2 = time.perf_counter()
    return D, orders, t1 - t0, t2 - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--sizes", default="32,64,140")
    ap.add_argument("--sites", default="1000,10000")
    ap.add_argument("--missing", default="0,0.02")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-a", action="store_true")
    ap.add_argument("--model", default="p", choices=["p", "jc69", "k2p"] + list(PAIR_MODELS))
    ap.add_argument("--gamma", type=float, default=None)
    args = ap.parse_args()
    if args.gamma is not None and args.model in ("p", "logdet"):
        ap.error("--gamma needs a model with a gamma form")
    B = args.batch
    # warm both routes: the runtime, the kernels' code objects, numpy's thread pool
    s0 = alignment(8, 256, 1, 0.0)
    c0 = fa.bootstrap_counts(256, 64, 1)
    beside = () if args.model == "p" else ("p", "k2p", args.model) if args.model in PAIR_MODELS else ("p", "jc69", "k2p")
    for m in sorted({"p", args.model} | set(beside)):
        route_a(s0, c0, m)
    if args.gamma is not None:
        route_a(s0, c0, args.model, args.gamma)
        route_b_gamma(s0, c0, args.model, args.gamma)
    else:
        route_b(s0, c0, args.model)
    lines = []
    for miss in [float(x) for x in args.missing.split(",")]:
        for n in [int(x) for x in args.sizes.split(",")]:
            for L in [int(x) for x in args.sites.split(",")]:
                seq = alignment(n, L, 1000 + n + L, miss)
                counts = fa.bootstrap_counts(L, B, 7)
                best = None
                for _ in range(2):   # (the better of two runs of each route)
                    T, oa, st, ta_call, ta = route_a(seq, counts, args.model, args.gamma)
                    if best is None or ta < best[0]:
                        best = (ta, ta_call, st)
                    Ta = T.cpu().numpy()
                    del T
                ta, ta_call, st = best
                rec = {"model": args.model, "n": n, "L": L, "B": B, "missing": miss, "digit_passes": st["digit_passes"], "has_missing": st["has_missing"],
                       "chunks": st["chunks"], "t_kernel_ms": st["t_kernel_s"] * 1e3, "t_upload_ms": st["t_upload_s"] * 1e3,
                       "t_call_ms": ta_call * 1e3, "t_route_a_ms": ta * 1e3, "out_bytes": B * n * n * 8}
                if args.model != "p":   # the kernels side by side: the better of two calls each
                    for m in beside:
                        rec[f"t_kernel_{m}_ms"] = min(fa.alignment_distances_batch(seq, counts, out="torch", model=m)[1]["t_kernel_s"] for _ in range(2)) * 1e3
                if args.gamma is not None:   # the gamma kernel beside the equal-rates one: alternating, the better of three calls each
                    tk = {None: [], args.gamma: []}
                    for _ in range(3):
                        for sh in (None, args.gamma):
                            tk[sh].append(fa.alignment_distances_batch(seq, counts, out="torch", model=args.model, gamma_shape=sh)[1]["t_kernel_s"])
                    rec.update({"gamma": args.gamma, f"t_kernel_{args.model}_ms": min(tk[None]) * 1e3,
                                f"t_kernel_{args.model}_gamma_ms": min(tk[args.gamma]) * 1e3, "n_pairs_times_B": n * (n - 1) // 2 * B})
                    if not args.only_a:
                        tb_best = None
                        for _ in range(2):
                            Db, ob, tb_tables, tb_np, tb = route_b_gamma(seq, counts, args.model, args.gamma)
                            if tb_best is None or tb < tb_best[0]:
                                tb_best = (tb, tb_tables, tb_np)
                        rec.update({"t_tables_to_host_ms": tb_best[1] * 1e3, "t_tables_and_numpy_ms": tb_best[2] * 1e3, "t_route_b_ms": tb_best[0] * 1e3,
                                    "ratio_b_over_a": tb_best[0] / ta, "tables_bytes": 16 * 8 * B * n * n,
                                    "matrices_bitwise_equal": bool((Ta.view(np.int64) == Db.view(np.int64)).all()),
                                    "orders_equal": bool((oa == ob).all()), "max_rel_diff": float(np.abs(Ta - Db).max() / np.abs(Db).max())})
                elif not args.only_a:
                    tb_best = None
                    for _ in range(2):
                        Db, ob, tb_np, tb = route_b(seq, counts, args.model)
                        if tb_best is None or tb < tb_best[0]:
                            tb_best = (tb, tb_np)
                    rec.update({"t_numpy_ms": tb_best[1] * 1e3, "t_route_b_ms": tb_best[0] * 1e3, "ratio_b_over_a": tb_best[0] / ta,
                                "matrices_bitwise_equal": bool((Ta.view(np.int64) == Db.view(np.int64)).all()),
                                "orders_equal": bool((oa == ob).all())})
                    if args.model != "p":
                        rec["max_rel_diff"] = float(np.abs(Ta - Db).max() / np.abs(Db).max())
                line = json.dumps(rec)
                print(line, flush=True)
                lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

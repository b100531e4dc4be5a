// fnn_small_global.h -- the batched path above the LDS limit: one workgroup runs a whole runNeighborNet for
// SMALL_LDS_MAX_N < n <= SMALL_GLOBAL_MAX_N with the n x n matrix in a per-problem working copy in GLOBAL memory and
// everything else (Sx, id, distID, partner, merge log, control block, staging arrays) in LDS.  DESIGN.md section 11.
//
// The sequence, the state and the arithmetic are those of fnn_small.h: a SmallView whose D points at the working copy
// serves every phase body that stays efficient there (pick, choice + subtract, the bookkeeping, the matrix update, the
// special finish, the output).  New bodies replace the ones in which single lanes walked the matrix - an LDS read is a
// few cycles, a dependent global load a few hundred nanoseconds:
//   global_scan_thread   a wave takes whole rows, its lanes consecutive positions: long contiguous row reads, the
//                        entries of four pairs per lane in flight at once
//   global_rx_stage/sum  ComputeRx: all threads gather the addends into four LDS arrays, then four lanes add them
//   global_add_stage/sum u.Sx: every position stages its addend and a "takes part" mark, then one lane adds them
//   global_init_sums     the same addends in the same order, four loads in flight per lane
// Waves hand matrix entries to each other through global memory across the workgroup barrier only (one CU, one L1,
// write-through stores); the pointer to the working copy is neither const nor __restrict__, so no load of it may move
// to the scalar cache or across a barrier.
#ifndef FNN_SMALL_GLOBAL_H
#define FNN_SMALL_GLOBAL_H

#include <cstring>
#include <memory>

#include "fnn_small.h"

namespace fnn {

constexpr int32_t SMALL_GLOBAL_MAX_N = 1024;  // also the engine's end-game threshold
constexpr int32_t SMALL_GLOBAL_STAGES = 4;    // Rx of Cx, Cx.nbr, Cy, Cy.nbr; array 0 also serves u.Sx

// The smallest batch that takes this route by default: the smallest measured batch from which it beat the engine loop
// (crossover table of DESIGN.md section 11: 4 problems win at 141, 256, 512, 640 and 768 taxa and lose at 1024, where 16
// win; nothing between 768 and 1024 was timed, so those sizes take the larger value).  Never below 4: three problems of
// 141 taxa stay on the engine loop.
FNN_HD constexpr int64_t small_global_min_batch(int32_t n) { return n <= 768 ? 4 : 16; }

struct GlobalLayout { int32_t ldw, off_sx, off_log, off_ctl, off_wred, off_id, off_did, off_pp, off_stage, off_mark, off_info, bytes; };

// Row stride of the working copy in doubles: the smallest value >= n that is 32 modulo 64.  Every row then starts on a
// 256-byte boundary (a wave's row read is whole lines) and consecutive rows are an ODD number of 256-byte units apart, so
// a walk down a column (the merge's D[P][X], the initial sums) moves over the memory channels instead of returning to one,
// which a power-of-two stride (n = 256, 512, 1024) would do.
FNN_HD constexpr int32_t small_global_ldw(int32_t n) { return (n + 31) / 64 * 64 + 32; }

FNN_HD constexpr GlobalLayout small_global_layout(int32_t n) {
    GlobalLayout L{};
    L.ldw = small_global_ldw(n);
    int32_t o = 0;
    L.off_sx = o;    o += n * 8;                                   // Sx per position
    L.off_stage = o; o += SMALL_GLOBAL_STAGES * n * 8;             // addends per position
    L.off_log = o;   o += (n > 3 ? n - 3 : 1) * (int32_t)sizeof(Agg3Rec);
    L.off_ctl = o;   o += (int32_t)sizeof(SmallCtl);
    L.off_wred = o;  o += SMALL_MAX_WAVES * (int32_t)sizeof(SmallCand);
    L.off_id = o;    o += n * 4;
    L.off_did = o;   o += n * 4;
    L.off_pp = o;    o += n * 4;
    L.off_mark = o;  o += n * 4;                                   // "takes part" per position
    L.off_info = o;  o += n * 4;                                   // the scan's word per position
    L.bytes = (o + 15) / 16 * 16;
    return L;
}
static_assert(small_global_layout(SMALL_GLOBAL_MAX_N).bytes <= SMALL_LDS_CAP, "the cap must fit the LDS of one workgroup");
// (LDS leaves room for two workgroups per CU at the cap; the kernel's registers currently admit one: DESIGN.md section 11)
static_assert(2 * small_global_layout(SMALL_GLOBAL_MAX_N).bytes <= SMALL_LDS_CAP, "LDS for two workgroups per CU at the cap");
static_assert(SMALL_GLOBAL_MAX_N <= 32767, "the scan's word holds two distIDs of 15 bits");

// doubles per problem in the working buffer
FNN_HD constexpr int64_t small_global_pitch(int32_t n) { return (int64_t)n * small_global_ldw(n); }

// Workgroup size by n.  Unmeasured choice (above the LDS limit only 1024 threads were timed): there the scan has
// thousands of pairs per wave and each costs a global load, so every wave the CU can hold for one workgroup is put to it.
inline int32_t small_global_block_threads(int32_t n) { return n <= 64 ? 256 : 1024; }

struct GlobalView : SmallView {
    double* stage;  // SMALL_GLOBAL_STAGES arrays of n
    int32_t* mark;
    int32_t* info;
    FNN_HD double& st(int32_t k, int32_t i) const { return stage[k * n + i]; }
};

// D: the problem's working copy (row stride small_global_ldw(n))
FNN_HD GlobalView small_global_view(unsigned char* base, double* D, int32_t n) {
    const GlobalLayout L = small_global_layout(n);
    GlobalView V;
    V.D = D;
    V.Sx = reinterpret_cast<double*>(base + L.off_sx);
    V.stage = reinterpret_cast<double*>(base + L.off_stage);
    V.log = reinterpret_cast<Agg3Rec*>(base + L.off_log);
    V.ctl = reinterpret_cast<SmallCtl*>(base + L.off_ctl);
    V.wred = reinterpret_cast<SmallCand*>(base + L.off_wred);
    V.id = reinterpret_cast<int32_t*>(base + L.off_id);
    V.did = reinterpret_cast<int32_t*>(base + L.off_did);
    V.pp = reinterpret_cast<int32_t*>(base + L.off_pp);
    V.mark = reinterpret_cast<int32_t*>(base + L.off_mark);
    V.info = reinterpret_cast<int32_t*>(base + L.off_info);
    V.n = n;
    V.ldm = L.ldw;
    return V;
}

// The caller's matrix (row stride ld) into the working copy; consecutive threads read consecutive addresses.
FNN_HD void global_copy(int tid, int nt, const GlobalView& V, const double* g, int64_t ld) {
    const int32_t n = V.n, tot = n * n;
    for (int32_t e = tid; e < tot; e += nt) {
        const int32_t r = e / n, c = e - r * n;
        V.D[r * V.ldm + c] = g[(int64_t)r * ld + c];
    }
}

// The scan's word of position p: -1 if p does not stand for its cluster (p.nbr.id < p.id), else p's distID in the low half
// and its partner's in the high half (its own again if it has none).  The scan evaluates m (m - 1) / 2 pairs per event and
// is bound by the instructions it issues, so what depends on ONE position only - three dependent LDS reads for "stands for
// its cluster", two for the partner's distID - is computed once per position and event (by the phase that runs last before
// the scan: the initial sums, then the add) and read back as one word per pair.
FNN_HD int32_t global_scan_word(const GlobalView& V, int32_t p) {
    if (!small_rep(V, p)) return -1;
    const int32_t q = V.pp[p];
    return V.did[p] | (V.did[q < 0 ? p : q] << 16);
}

// A.2 initial sums, as small_init_sums: Sx[k] = left-to-right sum of D[0][k], ..., D[k-1][k], D[k][k+1], ..., D[k][n-1].
// Down the column consecutive threads read consecutive addresses.  Along the row they are a row stride apart; every line
// a lane fetches serves its next 16 addends.  In both walks four loads are issued before their four additions (made in
// order), so a lane has four loads in flight instead of one.
FNN_HD void global_init_sums(int tid, int nt, const GlobalView& V) {
    const int32_t n = V.n;
    for (int32_t k = tid; k < n; k += nt) {
        double s = 0.0;
        int32_t j = 0;
        for (; j + 4 <= k; j += 4) {
            const double a = V.d(j, k), b = V.d(j + 1, k), c = V.d(j + 2, k), d = V.d(j + 3, k);
            s += a; s += b; s += c; s += d;
        }
        for (; j < k; j++) s += V.d(j, k);
        const double* row = &V.d(k, 0);
        j = k + 1;
        for (; j + 4 <= n; j += 4) {
            const double a = row[j], b = row[j + 1], c = row[j + 2], d = row[j + 3];
            s += a; s += b; s += c; s += d;
        }
        for (; j < n; j++) s += row[j];
        V.Sx[k] = s;
        V.info[k] = global_scan_word(V, k);
    }
}

// A.4 scan, this thread's share: wave w = tid / 64 takes the rows i = w, w + nt / 64, ..., lane l the columns j = l, l + 64,
// ... of each.  A wave-instruction then reads up to 64 consecutive positions of one matrix row (positions and distIDs
// agree until swap-with-last moves a node).  The thread visits its pairs i-ascending, j-ascending, so its own first
// strict minimum is its minimum under the total order.
//
// A pair costs one to four matrix entries, each a global load of a few hundred nanoseconds, so the lane takes
// SMALL_GLOBAL_SCAN_UNROLL columns at a time: all their entries are loaded first (a column that is out of range or not
// eligible loads from column 0 of the row, a valid address, and is dropped afterwards), then each pair is evaluated in
// column order.  CD(i, j) is small_cd's, operation for operation: `a`, `(a + c) / 2.0`, `(a + b) / 2.0` or
// `(((a + b) + c) + d) / 4.0` with a = D[P][Q], b = D[P][QN], c = D[PN][Q], d = D[PN][QN].  Which positions are
// eligible, and Q and QN, come from the scan's word (global_scan_word).
constexpr int32_t SMALL_GLOBAL_SCAN_UNROLL = 4;

FNN_HD SmallCand global_scan_thread(int tid, int nt, const GlobalView& V, int32_t m, int32_t c) {
    constexpr int32_t U = SMALL_GLOBAL_SCAN_UNROLL;
    SmallCand best{0.0, -1, -1};
    const double f = (double)c - 2.0;
    for (int32_t i = tid >> 6; i < m; i += nt >> 6) {
        const int32_t wi = V.info[i];
        if (wi < 0) continue;            // one node per cluster
        const int32_t pn = V.pp[i];      // (pn == j is the reference's `p.nbr == q`: the pair of one cluster is no candidate)
        const double sxi = V.Sx[i];
        const double* rowP = V.D + (wi & 0xFFFF) * V.ldm;
        const double* rowPN = V.D + (wi >> 16) * V.ldm;
        for (int32_t j0 = tid & 63; j0 < i; j0 += 64 * U) {
            bool ok[U];
            uint32_t Q[U], QN[U];
            double a[U], b[U], cc[U], d[U], sxj[U];
#pragma unroll
            for (int32_t u = 0; u < U; u++) {
                const int32_t j = j0 + 64 * u, wj = j < i ? V.info[j] : -1;
                ok[u] = wj >= 0 && j != pn;
                Q[u] = ok[u] ? (uint32_t)(wj & 0xFFFF) : 0u;
                QN[u] = ok[u] ? (uint32_t)(wj >> 16) : 0u;
                sxj[u] = V.Sx[ok[u] ? j : 0];
                a[u] = rowP[Q[u]];
                b[u] = rowP[QN[u]];
                cc[u] = d[u] = 0.0;
                if (pn >= 0) { cc[u] = rowPN[Q[u]]; d[u] = rowPN[QN[u]]; }  // (the same branch for the whole wave: pn belongs to the row)
            }
            // (selects, not branches: the lanes of a wave differ in all of this, and a sum of entries that are not needed is
            // harmless; each value that IS used comes from small_cd's own operations in small_cd's order)
#pragma unroll
            for (int32_t u = 0; u < U; u++) {
                const bool single = QN[u] == Q[u];
                double cd;
                if (pn < 0) cd = single ? a[u] : (a[u] + b[u]) / 2.0;
                else cd = single ? (a[u] + cc[u]) / 2.0 : (((a[u] + b[u]) + cc[u]) + d[u]) / 4.0;
                const double q = f * cd - sxi - sxj[u];
                const bool take = ok[u] && (best.i < 0 || q < best.q);
                best.q = take ? q : best.q;
                best.i = take ? i : best.i;
                best.j = take ? j0 + 64 * u : best.j;
            }
        }
    }
    return best;
}

// A.5 ComputeRx (:549-561), first half: position i stages its addend of each of the up to four sums - v or v / 2.0,
// exactly as small_rx computes it
FNN_HD void global_rx_stage(int tid, int nt, const GlobalView& V, int32_t m) {
    const SmallCtl& K = *V.ctl;
    const int32_t cx = K.pcx, cy = K.pcy, cxn = V.pp[cx], cyn = V.pp[cy];
    const int32_t z[4] = {cx, cxn, cy, cyn};
    for (int32_t i = tid; i < m; i += nt) {
        const int32_t P = V.did[i];
        const bool whole = i == cx || i == cxn || i == cy || i == cyn || V.pp[i] < 0;
        for (int32_t k = 0; k < 4; k++) {
            if (z[k] < 0) continue;
            const double v = V.d(V.did[z[k]], P);
            V.st(k, i) = whole ? v : v / 2.0;
        }
    }
}

// The sequential sum x[0] + x[1] + ... (from 0.0, in index order; `mark` given: only the marked ones) by ONE lane.  The
// additions are a dependent chain, the LDS reads are not: sixteen values are read before their additions, so the lane
// waits for LDS once per sixteen addends instead of once per addend.
constexpr int32_t SMALL_GLOBAL_SUM_UNROLL = 16;

FNN_HD double global_seq_sum(const double* x, const int32_t* mark, int32_t m) {
    constexpr int32_t U = SMALL_GLOBAL_SUM_UNROLL;
    double s = 0.0;
    int32_t i = 0;
    for (; i + U <= m; i += U) {
        double v[U];
        int32_t k[U];
#pragma unroll
        for (int32_t u = 0; u < U; u++) { v[u] = x[i + u]; k[u] = mark ? mark[i + u] : 1; }
#pragma unroll
        for (int32_t u = 0; u < U; u++) s = k[u] ? s + v[u] : s;
    }
    for (; i < m; i++)
        if (!mark || mark[i]) s += x[i];
    return s;
}

// ... second half: four lanes (the first of four waves) add them from LDS in position order, starting from 0.0
FNN_HD void global_rx_sum(int tid, int nt, const GlobalView& V, int32_t m) {
    if ((tid & 63) != 0 || (tid >> 6) >= 4) return;
    const SmallCtl& K = *V.ctl;
    const int32_t k = tid >> 6, cx = K.pcx, cy = K.pcy;
    const int32_t z = k == 0 ? cx : (k == 1 ? V.pp[cx] : (k == 2 ? cy : V.pp[cy]));
    if (z < 0) return;
    V.ctl->rx[k] = global_seq_sum(&V.st(k, 0), nullptr, m);
}

// A.5 add (updateClusterDistances :517-536), first half: position i adds CD(p, u) to its own cluster's sums as in
// small_add, and stages the value and whether it took part
FNN_HD void global_add_stage(int tid, int nt, const GlobalView& V) {
    const SmallCtl& K = *V.ctl;
    const int32_t m = K.m, pu = K.pu, pv = K.pv;
    for (int32_t i = tid; i < m; i += nt) {
        const bool takes = small_rep(V, i) && i != pu && i != pv;
        V.mark[i] = takes ? 1 : 0;
        if (takes) {
            const double v = small_cd(V, i, pu);
            V.Sx[i] += v;
            if (V.pp[i] >= 0) V.Sx[V.pp[i]] += v;
            V.st(0, i) = v;
        }
        V.info[i] = global_scan_word(V, i);  // (every merge's bookkeeping is done: the state the next scan sees)
    }
}

// ... second half: u.Sx is the sequential sum of the staged values in position order (one lane: the last thread, as in
// small_add); thread 0 emits the event
FNN_HD void global_add_sum(int tid, int nt, const GlobalView& V, Event* gev) {
    SmallCtl& K = *V.ctl;
    if (tid == nt - 1) {
        const double s = global_seq_sum(&V.st(0, 0), V.mark, K.m);
        V.Sx[K.pu] = s;
        V.Sx[K.pv] = s;
    }
    if (tid == 0) {
        if (gev && K.nev < V.n) gev[K.nev] = K.cur;  // (every event takes a cluster away: fewer than n events)
        K.nev++;
    }
}

// The whole problem: small_problem()'s sequence with the bodies above in place of scan, rx, add and the initial sums.
// `ex.all(f)` as there; `ex.scan_global` runs global_scan_thread and leaves one record per wave in V.wred.  What
// small_problem() says about the control words read between two phases holds here word for word: the added phases
// (rx_sum, add_sum) write rx, Sx, nev and the event only, none of which is read between phases.
template <class Exec>
FNN_HD void global_problem(Exec& ex, const GlobalView& V, Event* gev, int32_t* gmeta, Agg3Rec* glog) {
    ex.all([&](int tid, int nt) { small_init_nodes(tid, nt, V); });
    ex.all([&](int tid, int nt) { global_init_sums(tid, nt, V); });
    for (;;) {  // agglomNodes (:339-393)
        const int32_t m = V.ctl->m, c = V.ctl->c;
        if (m <= 3) break;
        if (m == 4 && c == 2) {
            ex.all([&](int tid, int nt) { small_finish_book(tid, nt, V, gev); });
            if (!V.ctl->err) ex.all([&](int tid, int nt) { small_agg3_matrix(tid, nt, V, 4); });
            break;
        }
        ex.scan_global(V, m, c);
        ex.all([&](int tid, int nt) { small_pick(tid, nt, V, m, c); });
        if (V.ctl->err) break;
        if (V.ctl->need_rx) {
            ex.all([&](int tid, int nt) { global_rx_stage(tid, nt, V, m); });
            ex.all([&](int tid, int nt) { global_rx_sum(tid, nt, V, m); });
        }
        ex.all([&](int tid, int nt) { small_subtract(tid, nt, V, m, c); });
        ex.all([&](int tid, int nt) { small_merge_book(tid, nt, V, m, c); });
        if (V.ctl->err) break;
        const int32_t kind = V.ctl->kind;
        if (kind != FNN_KIND_2WAY) ex.all([&](int tid, int nt) { small_agg3_matrix(tid, nt, V, m); });
        if (kind == FNN_KIND_4WAY) {
            ex.all([&](int tid, int nt) { small_merge_book2(tid, nt, V, m); });
            if (V.ctl->err) break;
            ex.all([&](int tid, int nt) { small_agg3_matrix(tid, nt, V, m - 1); });
        }
        ex.all([&](int tid, int nt) { global_add_stage(tid, nt, V); });
        ex.all([&](int tid, int nt) { global_add_sum(tid, nt, V, gev); });
    }
    ex.all([&](int tid, int nt) { small_output(tid, nt, V, gmeta, glog); });
}

// ------------------------------------------------------------------------------------------------ host side
// Which calls take this route (the C entry points ask before they choose between small_batch and small_global_batch).
// FNN_BATCH_ROUTE=global forces it for any 4 <= n <= SMALL_GLOBAL_MAX_N and any batch >= 1 (tests reach it at small n
// that way); FNN_BATCH_ROUTE=engine keeps every n above the LDS limit on the engine loop (tools/batch_perf.py).
inline bool small_global_route(int32_t n, int64_t batch) {
    const char* e = std::getenv("FNN_BATCH_ROUTE");
    if (e && !std::strcmp(e, "global")) return n >= 4 && n <= SMALL_GLOBAL_MAX_N && batch >= 1;
    if (e && !std::strcmp(e, "engine")) return false;
    return n > SMALL_LDS_MAX_N && n <= SMALL_GLOBAL_MAX_N && batch >= small_global_min_batch(n);
}

// fnn_canonical_order_batch[_device]_f64 on this route over a backend B (HIP: fnn_batch.hip; CPU driver:
// tests/emu/fnn_batch_global_emu.cpp): small_batch's open / alloc / h2d / d2h / validate / err and
//   run_global(src, src_ld, src_stride, work, cnt, n, threads, lds_bytes, meta, log, ev, &t_kernel_s)
// which runs problem b on the working copy at work + b * small_global_pitch(n), first copying it there from
// src + b * src_stride unless src == work.  The caller has checked small_global_route(n, batch).
//
// The caller's matrices are never written.  Host entry: the rows are packed straight into the working layout and
// uploaded, and the kernel runs in place in that buffer.  Device entry: the kernel copies each problem into a working
// buffer of the call's own.  Either buffer holds one chunk: at most SMALL_CHUNK_BYTES (2 GiB) of working copies, and
// at least one problem (8.25 MiB at n = 1024).
template <class B>
int32_t small_global_batch(B& be, const char* who, const double* D, bool on_device, int32_t n, int64_t ld, int64_t stride, int64_t batch,
                           const fnn_opts* o, int32_t* orders_out, fnn_event* events_out, int32_t* nevents_out, fnn_batch_stats* stats) {
    const double t0 = now_s();
    const std::string W = std::string(who) + ": ";
    fnn_batch_stats st{};
    st.lds_max_n = SMALL_LDS_MAX_N;
    fnn_opts opts{};
    if (o) opts = *o;
    if (opts.mode != FNN_MODE_CANONICAL && opts.mode != FNN_MODE_RELAXED) return fail(FNN_EINVAL, W + "unknown mode");
    if (n < 4 || n > SMALL_GLOBAL_MAX_N || batch < 1) return fail(FNN_EINVAL, W + "not a call for the global-memory route");
    if (!orders_out || !D) return fail(FNN_EINVAL, W + "NULL argument");
    if (ld < n || stride < (int64_t)n * ld) return fail(FNN_EINVAL, W + "needs ld >= n and stride >= n * ld");
    st.n_problems = batch;
    OrderStage out(batch, (size_t)batch * (size_t)(n + 1), events_out ? (size_t)batch * (size_t)n : 0);
    int32_t rc = be.open(opts.device);
    if (rc != FNN_OK) return fail(rc, W + be.err());
    const GlobalLayout L = small_global_layout(n);
    st.block_threads = small_global_block_threads(n);
    if (const int32_t v = batch_threads_switch()) st.block_threads = v;
    st.lds_bytes = L.bytes;
    const int64_t pitch = small_global_pitch(n);
    const int64_t chunk = batch_chunk(batch, 8 * pitch, true);
    int32_t* d_meta = (int32_t*)be.alloc(sizeof(int32_t) * SMALL_META_INTS * (size_t)chunk);
    Agg3Rec* d_log = (Agg3Rec*)be.alloc(sizeof(Agg3Rec) * (size_t)n * (size_t)chunk);
    Event* d_ev = events_out ? (Event*)be.alloc(sizeof(Event) * (size_t)n * (size_t)chunk) : nullptr;
    double* d_work = (double*)be.alloc(sizeof(double) * (size_t)pitch * (size_t)chunk);
    if (!d_meta || !d_log || (events_out && !d_ev) || !d_work) return fail(FNN_ENOMEM, W + "device allocation failed");
    // (not a std::vector: zero-filling up to 2 GiB costs more than the upload; the padding between rows is never read)
    std::unique_ptr<double[]> pack(on_device ? nullptr : new double[(size_t)pitch * (size_t)chunk]);
    std::vector<int32_t> meta((size_t)SMALL_META_INTS * (size_t)chunk);
    std::vector<Agg3Rec> log((size_t)n * (size_t)chunk);
    for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
        const int64_t cnt = batch - b0 < chunk ? batch - b0 : chunk;
        st.chunks++;
        const double* src = D + b0 * stride;
        int64_t kld = ld, kstride = stride;
        if (!on_device) {
            const double tu = now_s();
            for (int64_t b = 0; b < cnt; b++) pack_rows(&pack[(size_t)(b * pitch)], L.ldw, src + b * stride, ld, n);
            if (be.h2d(d_work, pack.get(), sizeof(double) * (size_t)(cnt * pitch)) != FNN_OK) return fail(FNN_EHIP, W + "upload failed (" + be.err() + ")");
            st.t_upload_s += now_s() - tu;
            src = d_work; kld = L.ldw; kstride = pitch;
        }
        if (opts.validate) {
            int64_t bad = -1;
            if (be.validate(src, n, kld, kstride, cnt, &bad) != FNN_OK) return fail(FNN_EHIP, W + "validate failed (" + be.err() + ")");
            if (bad >= 0) return fail_bad_matrix(W, b0 + bad);
        }
        double tk = 0.0;
        if (be.run_global(src, kld, kstride, d_work, cnt, n, st.block_threads, L.bytes, d_meta, d_log, d_ev, &tk) != FNN_OK)
            return fail(FNN_EHIP, W + "kernel failed (" + be.err() + ")");
        st.t_kernel_s += tk;
        if (be.d2h(meta.data(), d_meta, sizeof(int32_t) * SMALL_META_INTS * (size_t)cnt) != FNN_OK ||
            be.d2h(log.data(), d_log, sizeof(Agg3Rec) * (size_t)n * (size_t)cnt) != FNN_OK ||
            (d_ev && be.d2h(&out.evs[(size_t)b0 * (size_t)n], d_ev, sizeof(Event) * (size_t)n * (size_t)cnt) != FNN_OK))
            return fail(FNN_EHIP, W + "download failed (" + be.err() + ")");
        rc = small_collect(W, n, b0, cnt, meta.data(), log.data(), out.orders.data(), out.nev.data(), events_out ? out.evs.data() : nullptr, st);
        if (rc != FNN_OK) return rc;
        st.n_global += cnt;
    }
    out.commit(orders_out, events_out, nevents_out);
    st.t_total_s = now_s() - t0;
    if (stats) *stats = st;
    return FNN_OK;
}

}  // namespace fnn
#endif

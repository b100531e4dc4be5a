// fnn_small_splits.h -- batched circular split weights: one workgroup solves one whole non-negative least-squares problem
// min |A x - d|, x >= 0 over the n (n - 1) / 2 circular splits of one ordering, for 2 <= n <= SPLITS_MAX_N.  DESIGN.md
// section 12.
//
// The per-thread phase bodies (functions of (tid, nthreads, view)), the sequence that strings them through an executor
// (small_splits_problem) and the host side of the call (small_splits_batch<B>) live here, shared by the kernel
// (fnn_splits_batch.hip: the executor's barrier is __syncthreads()) and by the CPU driver of the tests
// (tests/emu/fnn_splits_batch_emu.cpp: a barrier is the end of a loop over tid).
//
// Method, step for step the one-problem solver's (fnn_splits.hip), on one workgroup's scale:
//   reorder      d[a][b] = D[ord[a+1]-1][ord[b+1]-1], a < b                                        (k_reorder)
//   closed form  x = A^-1 d, four reads per split; feasible: done                                   (k_unconstrained)
//   from below   Lawson-Hanson on the free set F from F = {} and x = 0, ONE split per step: the multiplier
//                w = A^T (d - A x) from 2-D prefix sums (k_ab, k_scan1, k_atx); the normal equations H_FF = L L^T held as
//                W = L^-1, appended to and never updated (h_entry); the ratio step when a weight would turn negative,
//                after which W is rebuilt from the first departed position on by appending again
//   certificate  g = A^T (A x - d) from the returned weights with the prefix-sum operators alone      (k_kkt)
//   output       live index order                                                                    (k_to_live)
// A problem that outgrows its factor, exceeds 40 n + 1000 steps or ends uncertified writes no weights and says so in its
// meta record; the host sends exactly those through the one-problem solver.
//
// State: the vectors over F (indices, x, s, c, z = W c, and three staging vectors), the row sums, the control block and one
// reduction record per wave sit in LDS (small_splits_layout); the five n x n grids, the mask and the factor sit in the
// problem's slice of a workspace in GLOBAL memory (small_splits_work).  Waves hand those to each other across the
// workgroup barrier only; the pointers are neither const nor __restrict__.
#ifndef FNN_SMALL_SPLITS_H
#define FNN_SMALL_SPLITS_H

#include <cmath>
#include <cstring>
#include <memory>

#include "fnn_small.h"

namespace fnn {

constexpr int32_t SPLITS_MAX_N = SMALL_LDS_MAX_N;  // the order batch's LDS limit (140): the everyday sizes of DESIGN.md section 11
static_assert(SPLITS_MAX_N <= 181, "grid indices i * n + j and live indices are int32, H entries below n^2 / 2");

// Splits the per-problem factor holds: uniform and tree-like distances end at <= 3.8 n and <= 2 n - 3 positive splits
// (fnn_splits.hip, split_weights_impl); 6 n leaves room for the peak on the way there.
FNN_HD constexpr int32_t small_splits_capacity(int32_t n) { return n * (n - 1) / 2 < 6 * n ? n * (n - 1) / 2 : 6 * n; }

// The smallest batch that takes the kernel by default: the smallest measured batch from which the call beat the loop over the
// one-problem solver at the upper end of each band of n (crossover table of DESIGN.md section 12: one problem wins at 32 taxa,
// 4 win at 64, 8 at 96, 16 at 128; at 140 taxa 16 won by 12 % only, so the band above 128 takes the next measured batch).  A
// workgroup's latency grows faster with n than the one-problem call's fixed cost, and it is the same for 1 or 256 problems.
FNN_HD constexpr int64_t small_splits_min_batch(int32_t n) { return n <= 32 ? 1 : (n <= 64 ? 4 : (n <= 96 ? 8 : (n <= 128 ? 16 : 32))); }

enum { SPLITS_ACT_APPEND = 0, SPLITS_ACT_DONE = 1, SPLITS_ACT_RECHECK = 2, SPLITS_ACT_GIVEUP = 3 };

struct SplitsCtl {
    double cmax, ll, lz, hkk, alpha, kkt;
    double dep;         // SplitsSwitches.dep
    int32_t max_steps;  // SplitsSwitches.steps, or 40 n + 1000
    int32_t nonfinite, neg, giveup, route, certified, action;
    int32_t f, ftot, leave, enter_pos;
    int32_t steps, outer, entered, departed, n_aside, peak, rechecked;
    int32_t aside_fresh, aside_rebuild, aside_enter, rechecks, releases;  // how often each safety-net path ran (never reset)
};
struct SplitsRec { double v; int32_t k, e; };  // value, tie key (lowest wins), payload; k < 0: none
struct SplitsMeta {
    double kkt;
    int32_t nonfinite, giveup, route, certified, outer, entered, departed, n_aside, peak;
    int32_t aside_fresh, aside_rebuild, aside_enter, rechecks, releases, steps, pad_;
};
static_assert(sizeof(SplitsMeta) == 72, "meta record layout");

// Test switches of the safety net (small_splits_switches reads them on the host; FNN_HD code only ever sees the values, and
// keeps them in the control block: the view stays as small as it was): the
// relative size of delta^2 = H_kk - l.l below which an appended split counts as numerically dependent on the factor, and
// the step limit (0: 40 n + 1000).
struct SplitsSwitches { double dep; int32_t steps, pad_; };
constexpr double SPLITS_DEP_REL = 1e-9;

FNN_HD bool splits_better(const SplitsRec& a, const SplitsRec& b) {  // a before b: larger value, then lower key
    if (a.k < 0) return false;
    return b.k < 0 || a.v > b.v || (a.v == b.v && a.k < b.k);
}

struct SplitsLayout { int32_t off_ctl, off_wred, off_rs, off_x, off_s, off_c, off_z, off_h, off_l, off_r, off_fi, bytes; };

FNN_HD constexpr SplitsLayout small_splits_layout(int32_t n, int32_t cap) {
    SplitsLayout L{};
    int32_t o = 0;
    L.off_ctl = o;  o += ((int32_t)sizeof(SplitsCtl) + 15) / 16 * 16;
    L.off_wred = o; o += SMALL_MAX_WAVES * (int32_t)sizeof(SplitsRec);
    L.off_rs = o;   o += n * 8;      // RS: prefix of the row sums of the symmetric completion
    L.off_x = o;    o += cap * 8;    // weights of the free set
    L.off_s = o;    o += cap * 8;    // the sub-problem's solution
    L.off_c = o;    o += cap * 8;    // c_F
    L.off_z = o;    o += cap * 8;    // z = W c_F
    L.off_h = o;    o += cap * 8;    // h = H[F, k]
    L.off_l = o;    o += cap * 8;    // l = W h
    L.off_r = o;    o += cap * 8;    // l^T W
    L.off_fi = o;   o += cap * 4;    // grid index i * n + j per member of F
    L.bytes = (o + 15) / 16 * 16;
    return L;
}
static_assert(small_splits_layout(SPLITS_MAX_N, small_splits_capacity(SPLITS_MAX_N)).bytes <= 65536, "LDS of one workgroup, without asking for more");

// The problem's slice of the workspace, in doubles: grids d, c = A^T d, x, P (prefix of x), y (A x - d, then its prefix), the
// mask (one byte per grid entry) and the factor W (cap x cap, row-major, lower triangle used).
struct SplitsWork { int64_t off_d, off_c, off_x, off_p, off_y, off_mask, off_w, pitch; };
FNN_HD constexpr SplitsWork small_splits_work(int32_t n, int32_t cap) {
    SplitsWork K{};
    const int64_t g = ((int64_t)n * n + 31) / 32 * 32;
    K.off_d = 0; K.off_c = g; K.off_x = 2 * g; K.off_p = 3 * g; K.off_y = 4 * g;
    K.off_mask = 5 * g;
    K.off_w = K.off_mask + (g / 8 + 31) / 32 * 32;
    K.pitch = (K.off_w + (int64_t)cap * cap + 31) / 32 * 32;
    return K;
}

struct SplitsView {
    SplitsCtl* ctl;
    SplitsRec* wred;
    double *rs, *xF, *sF, *cF, *zF, *hv, *lv, *rv;
    int32_t* Fi;
    double *gd, *gc, *gx, *gp, *gy, *W;
    uint8_t* mask;
    int32_t n, cap;
};

FNN_HD SplitsView small_splits_view(unsigned char* lds, double* work, int32_t n, int32_t cap) {
    const SplitsLayout L = small_splits_layout(n, cap);
    const SplitsWork K = small_splits_work(n, cap);
    SplitsView V;
    V.ctl = reinterpret_cast<SplitsCtl*>(lds + L.off_ctl);
    V.wred = reinterpret_cast<SplitsRec*>(lds + L.off_wred);
    V.rs = reinterpret_cast<double*>(lds + L.off_rs);
    V.xF = reinterpret_cast<double*>(lds + L.off_x);
    V.sF = reinterpret_cast<double*>(lds + L.off_s);
    V.cF = reinterpret_cast<double*>(lds + L.off_c);
    V.zF = reinterpret_cast<double*>(lds + L.off_z);
    V.hv = reinterpret_cast<double*>(lds + L.off_h);
    V.lv = reinterpret_cast<double*>(lds + L.off_l);
    V.rv = reinterpret_cast<double*>(lds + L.off_r);
    V.Fi = reinterpret_cast<int32_t*>(lds + L.off_fi);
    V.gd = work + K.off_d; V.gc = work + K.off_c; V.gx = work + K.off_x; V.gp = work + K.off_p; V.gy = work + K.off_y;
    V.mask = reinterpret_cast<uint8_t*>(work + K.off_mask);
    V.W = work + K.off_w;
    V.n = n; V.cap = cap;
    return V;
}

// ------------------------------------------------------------------------------------------------ phase bodies
FNN_HD bool splits_finite(double v) { return v - v == 0.0; }  // (false for NaN and the infinities)

// the live path's index of the fast algorithm's split (i, j), i < j (k_to_live read backwards)
FNN_HD int32_t splits_live_index(int32_t n, int32_t i, int32_t j) {
    const int32_t a = j == n - 1 ? 0 : i + 1, b = j == n - 1 ? i + 1 : j + 1;
    return (2 * n - a - 1) * a / 2 + (b - a - 1);
}

// H = A^T A in closed form (h_entry): pairs that the splits (i, j) and (k, l) both separate
FNN_HD double splits_h_entry(int32_t n, int32_t i, int32_t j, int32_t k, int32_t l) {
    const int32_t lo = i > k ? i : k, hi = j < l ? j : l;
    const double st = hi > lo ? (double)(hi - lo) : 0.0, s = (double)(j - i), t = (double)(l - k);
    return st * ((double)n - s - t + st) + (s - st) * (t - st);
}

FNN_HD double splits_p(const double* g, int32_t n, int32_t i, int32_t j) { return (i < 0 || j < 0) ? 0.0 : g[i * n + j]; }

// control block, mask, and the re-ordered distances (0 on and below the diagonal); a non-finite selected value is flagged
FNN_HD void splits_reorder(int tid, int nt, const SplitsView& V, const double* D, int64_t ld, const int32_t* ord) {
    const int32_t n = V.n, tot = n * n;
    for (int32_t e = tid; e < tot; e += nt) {
        const int32_t a = e / n, b = e - a * n;
        double v = 0.0;
        if (a < b) {
            v = D[(int64_t)(ord[a + 1] - 1) * ld + (ord[b + 1] - 1)];
            if (!splits_finite(v)) V.ctl->nonfinite = 1;
        }
        V.gd[e] = v;
        V.mask[e] = 0;
    }
}
FNN_HD void splits_init(int tid, int nt, const SplitsView& V, const SplitsSwitches& sw) {
    if (tid != 0) return;
    SplitsCtl z{};
    z.leave = -1; z.enter_pos = -1;
    z.dep = sw.dep;
    z.max_steps = sw.steps >= 1 ? sw.steps : 40 * V.n + 1000;
    *V.ctl = z;
}

// Chepoi & Fichet: x[i][j] = (dd(i,j) + dd(i+1,j+1) - dd(i,j+1) - dd(i+1,j)) / 2, positions modulo n (k_unconstrained)
FNN_HD double splits_dd(const SplitsView& V, int32_t a, int32_t b) {
    if (a == b) return 0.0;
    return a < b ? V.gd[a * V.n + b] : V.gd[b * V.n + a];
}
FNN_HD void splits_closed_form(int tid, int nt, const SplitsView& V) {
    const int32_t n = V.n, tot = n * n;
    for (int32_t e = tid; e < tot; e += nt) {
        const int32_t i = e / n, j = e - i * n;
        double v = 0.0;
        if (i < j) {
            const int32_t i1 = i + 1, j1 = (j + 1) % n;
            v = (splits_dd(V, i, j) + splits_dd(V, i1, j1) - splits_dd(V, i, j1) - splits_dd(V, i1, j)) / 2.0;
        }
        V.gx[e] = v;
    }
}
FNN_HD SplitsRec splits_most_negative(int tid, int nt, const SplitsView& V) {
    SplitsRec best{0.0, -1, -1};
    const int32_t n = V.n, tot = n * n;
    for (int32_t e = tid; e < tot; e += nt) {
        const int32_t i = e / n, j = e - i * n;
        if (i >= j) continue;
        const SplitsRec c{-V.gx[e], e, e};
        if (c.v > 0.0 && splits_better(c, best)) best = c;
    }
    return best;
}
// the minimum of the per-wave records (every fold phase starts with it)
FNN_HD SplitsRec splits_fold(const SplitsView& V, int nt) {
    SplitsRec best = V.wred[0];
    for (int w = 1; w < (nt + 63) / 64; w++)
        if (splits_better(V.wred[w], best)) best = V.wred[w];
    return best;
}
FNN_HD void splits_fold_neg(int tid, int nt, const SplitsView& V) {
    if (tid == 0) V.ctl->neg = splits_fold(V, nt).k >= 0 ? 1 : 0;
}

// 2-D inclusive prefix sum: along the rows (src -> dst, one thread per row), then down the columns in place
FNN_HD void splits_prefix_rows(int tid, int nt, int32_t n, const double* src, double* dst) {
    for (int32_t r = tid; r < n; r += nt) {
        double s = 0.0;
        for (int32_t c = 0; c < n; c++) { s += src[r * n + c]; dst[r * n + c] = s; }
    }
}
FNN_HD void splits_prefix_cols(int tid, int nt, int32_t n, double* g) {
    for (int32_t c = tid; c < n; c += nt) {
        double s = 0.0;
        for (int32_t r = 0; r < n; r++) { s += g[r * n + c]; g[r * n + c] = s; }
    }
}
// y = A x - d from P = prefix of x (k_ab), 0 on and below the diagonal
FNN_HD void splits_ab_minus_d(int tid, int nt, const SplitsView& V) {
    const int32_t n = V.n, tot = n * n;
    const double* P = V.gp;
    for (int32_t e = tid; e < tot; e += nt) {
        const int32_t a = e / n, b = e - a * n;
        double v = 0.0;
        if (a < b) {
            const double first = splits_p(P, n, a - 1, b - 1) - splits_p(P, n, a - 1, a - 1);
            const double second = (splits_p(P, n, b - 1, n - 1) - splits_p(P, n, a - 1, n - 1)) - (splits_p(P, n, b - 1, b - 1) - splits_p(P, n, a - 1, b - 1));
            v = (first + second) - V.gd[e];
        }
        V.gy[e] = v;
    }
}
// RS of the prefix Q held in gy (k_scan1): the addends, then their prefix by one lane
FNN_HD void splits_rs_stage(int tid, int nt, const SplitsView& V) {
    const int32_t n = V.n;
    const double* Q = V.gy;
    for (int32_t i = tid; i < n; i += nt)
        V.rs[i] = (splits_p(Q, n, i, n - 1) - splits_p(Q, n, i - 1, n - 1)) + (splits_p(Q, n, n - 1, i) - splits_p(Q, n, n - 1, i - 1));
}
FNN_HD void splits_rs_scan(int tid, int nt, const SplitsView& V) {
    if (tid != 0) return;
    double s = 0.0;
    for (int32_t i = 0; i < V.n; i++) { s += V.rs[i]; V.rs[i] = s; }
}
// (A^T y)[i][j], i < j, from Q and RS (k_atx)
FNN_HD double splits_atx(const SplitsView& V, int32_t i, int32_t j) {
    return (V.rs[j] - V.rs[i]) - 2.0 * (V.gy[j * V.n + j] - V.gy[i * V.n + j]);
}
FNN_HD void splits_c_store(int tid, int nt, const SplitsView& V) {
    const int32_t n = V.n, tot = n * n;
    for (int32_t e = tid; e < tot; e += nt) {
        const int32_t i = e / n, j = e - i * n;
        V.gc[e] = i < j ? splits_atx(V, i, j) : 0.0;
    }
}
FNN_HD SplitsRec splits_c_max(int tid, int nt, const SplitsView& V) {
    SplitsRec best{0.0, -1, -1};
    const int32_t n = V.n, tot = n * n;
    for (int32_t e = tid; e < tot; e += nt) {
        const int32_t i = e / n, j = e - i * n;
        if (i >= j) continue;
        const double a = V.gc[e] < 0.0 ? -V.gc[e] : V.gc[e];
        const SplitsRec c{a, e, e};
        if (a > 0.0 && splits_better(c, best)) best = c;
    }
    return best;
}
FNN_HD void splits_fold_cmax(int tid, int nt, const SplitsView& V) {
    if (tid != 0) return;
    const SplitsRec b = splits_fold(V, nt);
    V.ctl->cmax = b.k >= 0 ? b.v : 0.0;
}
FNN_HD double splits_scale(const SplitsView& V) { return V.ctl->cmax > 0.0 ? V.ctl->cmax : 1.0; }

// from below starts at x = 0
FNN_HD void splits_lh_begin(int tid, int nt, const SplitsView& V) {
    const int32_t tot = V.n * V.n;
    for (int32_t e = tid; e < tot; e += nt) V.gx[e] = 0.0;
    if (tid == 0) V.ctl->route = FNN_SW_ROUTE_FROM_BELOW;
}
// the entering split: the largest multiplier w = -(A^T (A x - d)) above 1e-12 max|c| outside F that is not set aside, ties
// to the lowest live index
FNN_HD SplitsRec splits_pick(int tid, int nt, const SplitsView& V) {
    SplitsRec best{0.0, -1, -1};
    const int32_t n = V.n, tot = n * n;
    const double thr = 1e-12 * splits_scale(V);
    for (int32_t e = tid; e < tot; e += nt) {
        const int32_t i = e / n, j = e - i * n;
        if (i >= j || V.mask[e]) continue;
        const SplitsRec c{-splits_atx(V, i, j), splits_live_index(n, i, j), e};
        if (c.v > thr && splits_better(c, best)) best = c;
    }
    return best;
}
FNN_HD void splits_give_up(const SplitsView& V, int32_t why) {
    V.ctl->giveup = why;
    V.ctl->action = SPLITS_ACT_GIVEUP;
}
FNN_HD void splits_fold_pick(int tid, int nt, const SplitsView& V) {
    if (tid != 0) return;
    SplitsCtl& K = *V.ctl;
    const SplitsRec b = splits_fold(V, nt);
    if (b.k < 0) {  // the splits set aside get one more look against the current factor before this may be the optimum
        K.action = (K.n_aside > 0 && !K.rechecked) ? SPLITS_ACT_RECHECK : SPLITS_ACT_DONE;
        return;
    }
    if (++K.steps > K.max_steps) { splits_give_up(V, FNN_SW_GIVEUP_STEPS); return; }
    if (K.f >= V.cap) { splits_give_up(V, FNN_SW_GIVEUP_CAPACITY); return; }
    V.Fi[K.f] = b.e;
    V.xF[K.f] = 0.0;
    V.cF[K.f] = V.gc[b.e];
    K.ftot = K.f + 1;
    K.enter_pos = K.f;
    K.action = SPLITS_ACT_APPEND;
}
// the splits set aside may be looked at again (aside == 0: nothing to do)
FNN_HD void splits_release(int tid, int nt, const SplitsView& V, int32_t rechecked) {
    const int32_t tot = V.n * V.n;
    for (int32_t e = tid; e < tot; e += nt)
        if (V.mask[e] == 2) V.mask[e] = 0;
    if (tid == 0) {
        V.ctl->n_aside = 0; V.ctl->rechecked = rechecked;
        if (rechecked) V.ctl->rechecks++; else V.ctl->releases++;
    }
}

// ---- append row r of W for the split at position r of F (positions below r are in the factor)
FNN_HD void splits_append_h(int tid, int nt, const SplitsView& V, int32_t r) {
    const int32_t n = V.n, k = V.Fi[r], ki = k / n, kj = k - ki * n;
    for (int32_t j = tid; j < r; j += nt) {
        const int32_t a = V.Fi[j] / n, b = V.Fi[j] - a * n;
        V.hv[j] = splits_h_entry(n, a, b, ki, kj);
    }
}
// l = W h, row `row`: this lane's share of the dot product (the executor adds the 64 shares in a fixed tree)
FNN_HD double splits_append_l_share(const SplitsView& V, int32_t row, int32_t lane) {
    double s = 0.0;
    const double* w = V.W + (int64_t)row * V.cap;
    for (int32_t j = lane; j <= row; j += 64) s += w[j] * V.hv[j];
    return s;
}
// l^T W per column; the last thread adds l.l, l.z and looks up H_kk
FNN_HD void splits_append_r(int tid, int nt, const SplitsView& V, int32_t r) {
    for (int32_t j = tid; j < r; j += nt) {
        double s = 0.0;
        for (int32_t i = j; i < r; i++) s += V.lv[i] * V.W[(int64_t)i * V.cap + j];
        V.rv[j] = s;
    }
    if (tid == nt - 1) {
        double ll = 0.0, lz = 0.0;
        for (int32_t i = 0; i < r; i++) { ll += V.lv[i] * V.lv[i]; lz += V.lv[i] * V.zF[i]; }
        const int32_t n = V.n, k = V.Fi[r], ki = k / n, kj = k - ki * n;
        V.ctl->ll = ll; V.ctl->lz = lz;
        V.ctl->hkk = splits_h_entry(n, ki, kj, ki, kj);
    }
}
// delta^2 = H_kk - l.l safely positive: the row [-(l^T W) / delta, 1 / delta] and z_r; else the split is set aside and
// leaves F (the positions behind it move down)
FNN_HD void splits_append_row(int tid, int nt, const SplitsView& V, int32_t r, int32_t ftot, int32_t fresh) {
    const double hkk = V.ctl->hkk, d2 = hkk - V.ctl->ll;
    if (d2 > V.ctl->dep * hkk) {
        const double dl = std::sqrt(d2);
        double* w = V.W + (int64_t)r * V.cap;
        for (int32_t j = tid; j < r; j += nt) w[j] = -V.rv[j] / dl;
        if (tid == 0) {
            SplitsCtl& K = *V.ctl;
            w[r] = 1.0 / dl;
            V.zF[r] = (V.cF[r] - K.lz) / dl;
            V.mask[V.Fi[r]] = 1;
            K.f = r + 1;
            if (fresh) K.entered++;
            if (r + 1 > K.peak) K.peak = r + 1;
        }
    } else if (tid == 0) {
        SplitsCtl& K = *V.ctl;
        const int32_t k = V.Fi[r];
        V.mask[k] = 2;
        V.gx[k] = 0.0;
        K.n_aside++;
        if (fresh) K.aside_fresh++;
        else { K.departed++; K.aside_rebuild++; }
        if (K.enter_pos == r) K.enter_pos = -1;
        else if (K.enter_pos > r) K.enter_pos--;
        for (int32_t j = r + 1; j < ftot; j++) { V.Fi[j - 1] = V.Fi[j]; V.xF[j - 1] = V.xF[j]; V.cF[j - 1] = V.cF[j]; }
        K.ftot = ftot - 1;
    }
}

// ---- the sub-problem on F: s = W^T z
FNN_HD void splits_solve(int tid, int nt, const SplitsView& V, int32_t f) {
    for (int32_t j = tid; j < f; j += nt) {
        double s = 0.0;
        for (int32_t i = j; i < f; i++) s += V.W[(int64_t)i * V.cap + j] * V.zF[i];
        V.sF[j] = s;
    }
}
// Lawson-Hanson ratio: the smallest x_i / (x_i - s_i) over the s_i that are not positive (as the largest negated ratio)
FNN_HD SplitsRec splits_ratio_min(int tid, int nt, const SplitsView& V, int32_t f) {
    SplitsRec best{0.0, -1, -1};
    for (int32_t j = tid; j < f; j += nt) {
        if (V.sF[j] > 0.0) continue;
        double ratio = V.xF[j] > 0.0 ? V.xF[j] / (V.xF[j] - V.sF[j]) : 0.0;
        if (!(ratio >= 0.0)) ratio = 0.0;  // (NaN)
        const SplitsRec c{-ratio, j, j};
        if (splits_better(c, best)) best = c;
    }
    return best;
}
FNN_HD void splits_fold_ratio(int tid, int nt, const SplitsView& V) {
    if (tid != 0) return;
    SplitsCtl& K = *V.ctl;
    const SplitsRec b = splits_fold(V, nt);
    K.leave = b.k;
    K.alpha = b.k >= 0 ? -b.v : 1.0;
    K.action = SPLITS_ACT_APPEND;
    if (b.k >= 0 && ++K.steps > K.max_steps) splits_give_up(V, FNN_SW_GIVEUP_STEPS);
}
// every s > 0: it is the new x
FNN_HD void splits_accept(int tid, int nt, const SplitsView& V, int32_t f) {
    for (int32_t j = tid; j < f; j += nt) {
        V.xF[j] = V.sF[j];
        V.gx[V.Fi[j]] = V.sF[j];
    }
    if (tid == 0) { V.ctl->outer++; V.ctl->enter_pos = -1; }
}
// x += alpha (s - x); what reaches zero leaves
FNN_HD void splits_ratio_step(int tid, int nt, const SplitsView& V, int32_t f, double alpha, int32_t leave) {
    for (int32_t j = tid; j < f; j += nt) {
        double xn = V.xF[j] + alpha * (V.sF[j] - V.xF[j]);
        if (j == leave || !(xn > 0.0)) xn = 0.0;
        V.xF[j] = xn;
    }
}
// F without the splits that left, in order (one lane); the factor stays valid up to the first departed position.  A split
// that leaves in the step in which it entered is set aside.
FNN_HD void splits_compact(int tid, int nt, const SplitsView& V, int32_t f) {
    if (tid != 0) return;
    SplitsCtl& K = *V.ctl;
    int32_t q = 0, pmin = -1, ep = -1;
    for (int32_t j = 0; j < f; j++) {
        if (V.xF[j] > 0.0) {
            if (j == K.enter_pos) ep = q;
            V.Fi[q] = V.Fi[j]; V.xF[q] = V.xF[j]; V.cF[q] = V.cF[j];
            q++;
            continue;
        }
        const int32_t k = V.Fi[j];
        V.gx[k] = 0.0;
        if (j == K.enter_pos) { V.mask[k] = 2; K.n_aside++; K.aside_enter++; }
        else V.mask[k] = 0;
        K.departed++;
        if (pmin < 0) pmin = j;
    }
    K.enter_pos = ep;
    K.f = pmin < 0 ? f : pmin;
    K.ftot = q;
}

// ---- certificate: the largest Kuhn-Tucker violation of the weights in gx, g = A^T (A x - d) in Q / RS (k_kkt)
FNN_HD SplitsRec splits_kkt(int tid, int nt, const SplitsView& V) {
    SplitsRec best{0.0, -1, -1};
    const int32_t n = V.n, tot = n * n;
    const double scale = splits_scale(V);
    for (int32_t e = tid; e < tot; e += nt) {
        const int32_t i = e / n, j = e - i * n;
        if (i >= j) continue;
        const double xv = V.gx[e], g = splits_atx(V, i, j);
        double v = xv > 0.0 ? (g < 0.0 ? -g : g) / scale : -g / scale;
        if (-xv > v) v = -xv;
        if (xv != xv || g != g) v = INFINITY;
        const SplitsRec c{v, e, e};
        if (v > 0.0 && splits_better(c, best)) best = c;
    }
    return best;
}
FNN_HD void splits_fold_kkt(int tid, int nt, const SplitsView& V) {
    if (tid != 0) return;
    const SplitsRec b = splits_fold(V, nt);
    V.ctl->kkt = b.k >= 0 ? b.v : 0.0;
    V.ctl->certified = V.ctl->kkt <= 1e-9 ? 1 : 0;
    if (!V.ctl->certified) V.ctl->giveup = FNN_SW_GIVEUP_NUMERIC;
}
// weights in live index order (only a certified problem writes them), and the meta record
FNN_HD void splits_output(int tid, int nt, const SplitsView& V, double* out, SplitsMeta* meta) {
    const SplitsCtl& K = *V.ctl;
    const int32_t n = V.n, tot = n * n;
    if (K.certified && !K.nonfinite && !K.giveup)
        for (int32_t e = tid; e < tot; e += nt) {
            const int32_t i = e / n, j = e - i * n;
            if (i < j) out[splits_live_index(n, i, j)] = V.gx[e];
        }
    if (tid == 0) {
        SplitsMeta m{};
        m.kkt = K.kkt; m.nonfinite = K.nonfinite; m.giveup = K.giveup; m.route = K.route; m.certified = K.certified;
        m.outer = K.outer; m.entered = K.entered; m.departed = K.departed; m.n_aside = K.n_aside; m.peak = K.peak;
        m.aside_fresh = K.aside_fresh; m.aside_rebuild = K.aside_rebuild; m.aside_enter = K.aside_enter;
        m.rechecks = K.rechecks; m.releases = K.releases; m.steps = K.steps;
        *meta = m;
    }
}

// ------------------------------------------------------------------------------------------------ the sequence
// ex.all(f): f(tid, nt) for every thread, then the barrier.  ex.best(V, f): every thread's record f(tid, nt), reduced to
// one record per wave in V.wred, then the barrier.  ex.rows(nrows, share, store): for every row, the 64 lanes' shares
// share(row, lane) added in a fixed tree and handed to store(row, sum), then the barrier.  ex.get(p): the control word *p
// for every thread, and a barrier behind the read, so that the next phase may write the word.
template <class Exec>
FNN_HD void splits_operators(Exec& ex, const SplitsView& V) {  // gx -> Q = prefix of (A x - d) in gy, RS
    const int32_t n = V.n;
    ex.all([&](int tid, int nt) { splits_prefix_rows(tid, nt, n, V.gx, V.gp); });
    ex.all([&](int tid, int nt) { splits_prefix_cols(tid, nt, n, V.gp); });
    ex.all([&](int tid, int nt) { splits_ab_minus_d(tid, nt, V); });
    ex.all([&](int tid, int nt) { splits_prefix_rows(tid, nt, n, V.gy, V.gy); });
    ex.all([&](int tid, int nt) { splits_prefix_cols(tid, nt, n, V.gy); });
    ex.all([&](int tid, int nt) { splits_rs_stage(tid, nt, V); });
    ex.all([&](int tid, int nt) { splits_rs_scan(tid, nt, V); });
}
template <class Exec>
FNN_HD void splits_append_pending(Exec& ex, const SplitsView& V, int32_t fresh) {  // positions f ... ftot - 1 of F enter the factor
    for (;;) {
        const int32_t r = ex.get(&V.ctl->f), ftot = ex.get(&V.ctl->ftot);
        if (r >= ftot) break;
        ex.all([&](int tid, int nt) { splits_append_h(tid, nt, V, r); });
        ex.rows(r, [&](int32_t row, int32_t lane) { return splits_append_l_share(V, row, lane); }, [&](int32_t row, double s) { V.lv[row] = s; });
        ex.all([&](int tid, int nt) { splits_append_r(tid, nt, V, r); });
        ex.all([&](int tid, int nt) { splits_append_row(tid, nt, V, r, ftot, fresh); });
    }
}

template <class Exec>
FNN_HD void small_splits_problem(Exec& ex, const SplitsView& V, const SplitsSwitches& sw, const double* D, int64_t ld, const int32_t* ord, double* out,
                                 SplitsMeta* meta) {
    const int32_t n = V.n;
    ex.all([&](int tid, int nt) { splits_init(tid, nt, V, sw); });
    ex.all([&](int tid, int nt) { splits_reorder(tid, nt, V, D, ld, ord); });
    if (!ex.get(&V.ctl->nonfinite)) {
        ex.all([&](int tid, int nt) { splits_closed_form(tid, nt, V); });
        ex.best(V, [&](int tid, int nt) { return splits_most_negative(tid, nt, V); });
        ex.all([&](int tid, int nt) { splits_fold_neg(tid, nt, V); });
        // c = A^T d and its largest magnitude, the scale of every threshold
        ex.all([&](int tid, int nt) { splits_prefix_rows(tid, nt, n, V.gd, V.gy); });
        ex.all([&](int tid, int nt) { splits_prefix_cols(tid, nt, n, V.gy); });
        ex.all([&](int tid, int nt) { splits_rs_stage(tid, nt, V); });
        ex.all([&](int tid, int nt) { splits_rs_scan(tid, nt, V); });
        ex.all([&](int tid, int nt) { splits_c_store(tid, nt, V); });
        ex.best(V, [&](int tid, int nt) { return splits_c_max(tid, nt, V); });
        ex.all([&](int tid, int nt) { splits_fold_cmax(tid, nt, V); });
        bool gave_up = false;
        if (ex.get(&V.ctl->neg)) {
            ex.all([&](int tid, int nt) { splits_lh_begin(tid, nt, V); });
            bool fresh_w = false;
            for (;;) {
                if (!fresh_w) splits_operators(ex, V);
                fresh_w = true;
                ex.best(V, [&](int tid, int nt) { return splits_pick(tid, nt, V); });
                ex.all([&](int tid, int nt) { splits_fold_pick(tid, nt, V); });
                const int32_t action = ex.get(&V.ctl->action);
                if (action == SPLITS_ACT_DONE) break;
                if (action == SPLITS_ACT_GIVEUP) { gave_up = true; break; }
                if (action == SPLITS_ACT_RECHECK) {
                    ex.all([&](int tid, int nt) { splits_release(tid, nt, V, 1); });
                    continue;
                }
                const int32_t f0 = ex.get(&V.ctl->f);
                splits_append_pending(ex, V, 1);
                if (ex.get(&V.ctl->f) == f0) continue;  // numerically dependent on the factor: set aside, the next largest
                for (;;) {
                    const int32_t f = ex.get(&V.ctl->f);
                    ex.all([&](int tid, int nt) { splits_solve(tid, nt, V, f); });
                    ex.best(V, [&](int tid, int nt) { return splits_ratio_min(tid, nt, V, f); });
                    ex.all([&](int tid, int nt) { splits_fold_ratio(tid, nt, V); });
                    if (ex.get(&V.ctl->action) == SPLITS_ACT_GIVEUP) { gave_up = true; break; }
                    const int32_t leave = ex.get(&V.ctl->leave);
                    if (leave < 0) {
                        // progress (the entering split stayed): the splits set aside may be looked at again
                        const bool progress = ex.get(&V.ctl->enter_pos) >= 0 && ex.get(&V.ctl->n_aside) > 0;
                        ex.all([&](int tid, int nt) { splits_accept(tid, nt, V, f); });
                        if (progress) ex.all([&](int tid, int nt) { splits_release(tid, nt, V, 0); });
                        break;
                    }
                    const double alpha = ex.get(&V.ctl->alpha);
                    ex.all([&](int tid, int nt) { splits_ratio_step(tid, nt, V, f, alpha, leave); });
                    ex.all([&](int tid, int nt) { splits_compact(tid, nt, V, f); });
                    splits_append_pending(ex, V, 0);
                }
                if (gave_up) break;
                fresh_w = false;
            }
        }
        if (!gave_up) {
            splits_operators(ex, V);
            ex.best(V, [&](int tid, int nt) { return splits_kkt(tid, nt, V); });
            ex.all([&](int tid, int nt) { splits_fold_kkt(tid, nt, V); });
        }
    }
    ex.all([&](int tid, int nt) { splits_output(tid, nt, V, out, meta); });
}
// ... with the defaults (an executor that knows no switches)
template <class Exec>
FNN_HD void small_splits_problem(Exec& ex, const SplitsView& V, const double* D, int64_t ld, const int32_t* ord, double* out, SplitsMeta* meta) {
    small_splits_problem(ex, V, SplitsSwitches{SPLITS_DEP_REL, 0, 0}, D, ld, ord, out, meta);
}

// ------------------------------------------------------------------------------------------------ host side
// Which calls take the kernel.  FNN_SW_BATCH_ROUTE=kernel sends any batch >= 1 of n <= SPLITS_MAX_N to it (tests, and
// tools/splits_batch_perf.py, reach it below the default threshold that way); FNN_SW_BATCH_ROUTE=loop keeps every call on the
// one-problem solver.
inline bool small_splits_route(int32_t n, int64_t batch) {
    const char* e = std::getenv("FNN_SW_BATCH_ROUTE");
    if (e && !std::strcmp(e, "kernel")) return n <= SPLITS_MAX_N && batch >= 1;
    if (e && !std::strcmp(e, "loop")) return false;
    return n <= SPLITS_MAX_N && batch >= small_splits_min_batch(n);
}
inline int32_t small_splits_cap(int32_t n) {
    int32_t cap = small_splits_capacity(n);
    if (const char* e = std::getenv("FNN_SW_BATCH_CAP")) { const int v = std::atoi(e); if (v >= 1 && v < cap) cap = v; }
    return cap;
}
// FNN_SW_BATCH_DEP=<x in (0, 1)> and FNN_SW_BATCH_STEPS=<steps >= 1>, for tests: with a large threshold or a small limit
// honest inputs reach the set-aside, recheck and give-up paths that they never reach otherwise.
inline SplitsSwitches small_splits_switches() {
    SplitsSwitches sw{SPLITS_DEP_REL, 0, 0};
    if (const char* e = std::getenv("FNN_SW_BATCH_DEP")) { const double v = std::atof(e); if (v > 0.0 && v < 1.0) sw.dep = v; }
    if (const char* e = std::getenv("FNN_SW_BATCH_STEPS")) { const long long v = std::atoll(e); if (v >= 1 && v <= 0x7fffffff) sw.steps = (int32_t)v; }
    return sw;
}

// the per-problem record of a problem that the kernel solved (m: its meta record, w: its N weights)
inline fnn_sw_stats small_splits_stats(const SplitsMeta& m, const double* w, int64_t N, int32_t cap) {
    fnn_sw_stats s{};
    const bool below = m.route == FNN_SW_ROUTE_FROM_BELOW;
    for (int64_t k = 0; k < N; k++) s.nsplits += w[k] > 0.000001 ? 1 : 0;
    s.route = m.route; s.certified = 1; s.kkt_violation = m.kkt;
    s.outer_iterations = m.outer; s.entered = m.entered; s.departed = m.departed; s.n_set_aside = m.n_aside;
    s.free_set_peak = m.peak; s.capacity = below ? cap : 0;
    s.final_threshold_rel = below ? 1e-12 : 0.0;
    s.reserved[0] = below ? 1 : 0;
    s.reserved[2] = m.steps;  // what the step limit counts: entering splits and ratio steps
    s.reserved2[0] = m.aside_fresh; s.reserved2[1] = m.aside_rebuild; s.reserved2[2] = m.aside_enter;
    s.reserved2[3] = (int64_t)m.rechecks | ((int64_t)m.releases << 32);
    return s;
}

// ---- steps that the same-size and the ragged call share, one definition each (those of every batch call: fnn_small.h)
// o[1] ... o[n] is a permutation of 1..n (`seen`: scratch)
inline bool splits_ordering_ok(const int32_t* o, int32_t n, std::vector<char>& seen) {
    seen.assign((size_t)n + 1, 0);
    for (int32_t i = 1; i <= n; i++) {
        if (o[i] < 1 || o[i] > n || seen[(size_t)o[i]]) return false;
        seen[(size_t)o[i]] = 1;
    }
    return true;
}

// The outputs of a weight call.  The call fills these and commits as its last step: a failing call returns before that
// and leaves the caller's arrays untouched.
struct WeightStage {
    std::vector<double> wts;
    std::vector<fnn_sw_stats> sws;
    WeightStage(int64_t batch, size_t weights) : wts(weights), sws((size_t)batch) {}
    void commit(double* weights_out, fnn_sw_stats* stats_out) const {
        std::memcpy(weights_out, wts.data(), sizeof(double) * wts.size());
        if (stats_out) std::memcpy(stats_out, sws.data(), sizeof(fnn_sw_stats) * sws.size());
    }
};

// One problem's result from the kernel (m: its record, w: its N weights, cap: the capacity it ran with).  Taken: the
// weights are in wts, the per-problem record in sw, and the problem is counted under its route.
enum SplitsTaken { SPLITS_NONFINITE, SPLITS_TO_SINGLE, SPLITS_TAKEN };
inline SplitsTaken small_splits_take(const SplitsMeta& m, const double* w, int64_t N, int32_t cap, double* wts, fnn_sw_stats& sw, fnn_sw_batch_stats& st) {
    if (m.nonfinite) return SPLITS_NONFINITE;
    if (m.giveup || !m.certified) return SPLITS_TO_SINGLE;
    std::memcpy(wts, w, sizeof(double) * (size_t)N);
    sw = small_splits_stats(m, w, N, cap);
    if (m.route == FNN_SW_ROUTE_FROM_BELOW) st.n_kernel++; else st.n_closed_form++;
    return SPLITS_TAKEN;
}

// What the kernel did not take or gave up on goes one by one through the one-problem solver, on a dense host copy.
struct SplitsSingle {
    std::vector<double> one, span;
    bool inexact = false;  // FNN_EINEXACT from a problem does not end the call: result() reports it after the commit
    // problem b: the n x n matrix at src with row stride ld (on_device: in device memory), to w and sw
    template <class B>
    int32_t run(B& be, const std::string& W, int64_t b, const double* src, bool on_device, int32_t n, int64_t ld, const int32_t* ordering,
                int32_t device, double* w, fnn_sw_stats* sw, fnn_sw_batch_stats& st) {
        if (on_device) {
            span.resize((size_t)((int64_t)(n - 1) * ld + n));
            if (be.d2h(span.data(), src, sizeof(double) * span.size()) != FNN_OK) return fail(FNN_EHIP, W + "download failed (" + be.err() + ")");
            src = span.data();
        }
        one.resize((size_t)n * (size_t)n);
        pack_rows(one.data(), n, src, ld, n);
        int32_t rc = be.single(one.data(), n, ordering, device, w, sw);
        if (rc == FNN_EINEXACT) { inexact = true; rc = FNN_OK; }
        if (rc != FNN_OK) { g_last_error = W + "problem " + std::to_string(b) + ": " + g_last_error; return rc; }
        st.n_fallback++;
        return FNN_OK;
    }
    int32_t result(const std::string& W) const {
        if (inexact) return fail(FNN_EINEXACT, W + "at least one problem of the one-problem solver returned weights that fail its Kuhn-Tucker check (stats_out[b].certified)");
        return FNN_OK;
    }
};

// fnn_split_weights_batch[_device]_f64 over a backend B (HIP: fnn_splits_batch.hip; CPU driver:
// tests/emu/fnn_splits_batch_emu.cpp): open / alloc / h2d / d2h / err as small_batch's, and
//   run_splits(dD, n, ld, stride, d_ord, cnt, cap, threads, lds_bytes, d_work, pitch, d_out, d_meta, &t_kernel_s)
//                (a backend that honours the test switches reads small_splits_switches() here, once per launch)
//   single(D_host, n, ordering, device, weights, &sw_stats)      the one-problem solver on a dense host matrix
template <class B>
int32_t small_splits_batch(B& be, const char* who, const double* D, bool on_device, int32_t n, int64_t ld, int64_t stride, int64_t batch,
                           const int32_t* orderings, int32_t device, double* weights_out, fnn_sw_stats* stats_out, fnn_sw_batch_stats* stats) {
    const double t0 = now_s();
    const std::string W = std::string(who) + ": ";
    fnn_sw_batch_stats st{};
    st.max_n = SPLITS_MAX_N;
    if (batch < 0) return fail(FNN_EINVAL, W + "negative batch");
    if (batch == 0) { if (stats) *stats = st; return FNN_OK; }
    if (n < 2) return fail(FNN_EINVAL, W + "needs n >= 2");
    if (!D || !orderings || !weights_out) return fail(FNN_EINVAL, W + "NULL argument");
    if (ld < n || stride < (int64_t)n * ld) return fail(FNN_EINVAL, W + "needs ld >= n and stride >= n * ld");
    {
        std::vector<char> seen;
        for (int64_t b = 0; b < batch; b++)
            if (!splits_ordering_ok(orderings + b * (n + 1), n, seen))
                return fail(FNN_EINVAL, W + "problem " + std::to_string(b) + ": ordering is not a permutation of 1..n");
    }
    st.n_problems = batch;
    const int64_t N = (int64_t)n * (n - 1) / 2;
    WeightStage res(batch, (size_t)batch * (size_t)N);
    std::vector<int64_t> todo;  // problems for the one-problem solver
    int32_t rc = be.open(device);
    if (rc != FNN_OK) return fail(rc, W + be.err());
    const bool kernel_route = small_splits_route(n, batch);
    if (!kernel_route) {
        for (int64_t b = 0; b < batch; b++) todo.push_back(b);
    } else {
        const int32_t cap = small_splits_cap(n);
        const SplitsLayout L = small_splits_layout(n, cap);
        const int64_t pitch = small_splits_work(n, cap).pitch;
        st.capacity = cap;
        st.lds_bytes = L.bytes;
        st.block_threads = small_block_threads(n);
        if (const int32_t v = batch_threads_switch()) st.block_threads = v;
        const int64_t chunk = batch_chunk(batch, 8 * pitch, true);
        st.workspace_bytes = 8 * pitch * chunk;
        double* d_work = (double*)be.alloc(sizeof(double) * (size_t)pitch * (size_t)chunk);
        double* d_out = (double*)be.alloc(sizeof(double) * (size_t)N * (size_t)chunk);
        int32_t* d_ord = (int32_t*)be.alloc(sizeof(int32_t) * (size_t)(n + 1) * (size_t)chunk);
        SplitsMeta* d_meta = (SplitsMeta*)be.alloc(sizeof(SplitsMeta) * (size_t)chunk);
        double* d_D = on_device ? nullptr : (double*)be.alloc(sizeof(double) * (size_t)n * (size_t)n * (size_t)chunk);
        if (!d_work || !d_out || !d_ord || !d_meta || (!on_device && !d_D)) return fail(FNN_ENOMEM, W + "device allocation failed");
        std::unique_ptr<double[]> pack(on_device ? nullptr : new double[(size_t)n * (size_t)n * (size_t)chunk]);
        std::vector<SplitsMeta> meta((size_t)chunk);
        std::vector<double> outs((size_t)N * (size_t)chunk);
        for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
            const int64_t cnt = batch - b0 < chunk ? batch - b0 : chunk;
            st.chunks++;
            const double tu = now_s();
            const double* src = D + b0 * stride;
            int64_t kld = ld, kstride = stride;
            if (!on_device) {
                for (int64_t b = 0; b < cnt; b++) pack_rows(&pack[(size_t)(b * n * n)], n, src + b * stride, ld, n);
                if (be.h2d(d_D, pack.get(), sizeof(double) * (size_t)(cnt * n * n)) != FNN_OK) return fail(FNN_EHIP, W + "upload failed (" + be.err() + ")");
                src = d_D; kld = n; kstride = (int64_t)n * n;
            }
            if (be.h2d(d_ord, orderings + b0 * (n + 1), sizeof(int32_t) * (size_t)(cnt * (n + 1))) != FNN_OK)
                return fail(FNN_EHIP, W + "upload failed (" + be.err() + ")");
            st.t_upload_s += now_s() - tu;
            double tk = 0.0;
            if (be.run_splits(src, n, kld, kstride, d_ord, cnt, cap, st.block_threads, L.bytes, d_work, pitch, d_out, d_meta, &tk) != FNN_OK)
                return fail(FNN_EHIP, W + "kernel failed (" + be.err() + ")");
            st.t_kernel_s += tk;
            if (be.d2h(meta.data(), d_meta, sizeof(SplitsMeta) * (size_t)cnt) != FNN_OK ||
                be.d2h(outs.data(), d_out, sizeof(double) * (size_t)(cnt * N)) != FNN_OK)
                return fail(FNN_EHIP, W + "download failed (" + be.err() + ")");
            for (int64_t b = 0; b < cnt; b++) {
                const SplitsTaken t = small_splits_take(meta[(size_t)b], &outs[(size_t)(b * N)], N, cap, &res.wts[(size_t)((b0 + b) * N)],
                                                        res.sws[(size_t)(b0 + b)], st);
                if (t == SPLITS_NONFINITE) return fail_nonfinite(W, b0 + b);
                if (t == SPLITS_TO_SINGLE) todo.push_back(b0 + b);
            }
        }
    }
    SplitsSingle single;
    for (int64_t b : todo) {
        rc = single.run(be, W, b, D + b * stride, on_device, n, ld, orderings + b * (n + 1), device, &res.wts[(size_t)(b * N)], &res.sws[(size_t)b], st);
        if (rc != FNN_OK) return rc;
    }
    res.commit(weights_out, stats_out);
    st.t_total_s = now_s() - t0;
    if (stats) *stats = st;
    return single.result(W);
}

// ------------------------------------------------------------------------------------------------ ragged batches
// fnn_split_weights_ragged[_device]_f64 over a backend B (HIP: fnn_splits_batch.hip; CPU driver:
// tests/emu/fnn_ragged_emu.cpp): open / alloc / h2d / d2h / err / single as above, and
//   run_splits_ragged(base, d_desc, classes, ncls, d_ord, d_work, d_out, d_meta, &t_kernel_s)     one launch per class
// Layout as small_ragged's (fnn_small.h); `orderings` and weights_out are concatenated in the caller's order.  The kernel
// takes the problems of 2 <= n <= SPLITS_MAX_N when there are at least small_splits_min_batch(largest such n) of them
// (FNN_SW_BATCH_ROUTE overrides as for the same-size call); everything else, and what gives up in the kernel, goes
// through the one-problem solver.
template <class B>
int32_t small_splits_ragged(B& be, const char* who, const double* D, bool on_device, const int64_t* offsets, const int32_t* ns, const int64_t* lds,
                            int64_t batch, const int32_t* orderings, int32_t device, double* weights_out, fnn_sw_stats* stats_out,
                            fnn_sw_batch_stats* stats) {
    const double t0 = now_s();
    const std::string W = std::string(who) + ": ";
    fnn_sw_batch_stats st{};
    st.max_n = SPLITS_MAX_N;
    if (batch < 0) return fail(FNN_EINVAL, W + "negative batch");
    if (batch == 0) { if (stats) *stats = st; return FNN_OK; }
    if (!D || !offsets || !ns || !orderings || !weights_out) return fail(FNN_EINVAL, W + "NULL argument");
    auto ld_of = [&](int64_t b) { return lds ? lds[b] : (int64_t)ns[b]; };
    std::vector<int64_t> oo((size_t)batch + 1, 0), wo((size_t)batch + 1, 0);  // where problem b's ordering and weights start
    std::vector<int64_t> kern, todo;  // kernel range in the caller's order; problems for the one-problem solver
    int32_t kmax = 0;
    {
        std::vector<char> seen;
        for (int64_t b = 0; b < batch; b++) {
            const int32_t n = ns[b];
            const std::string P = W + "problem " + std::to_string(b) + ": ";
            if (n < 2) return fail(FNN_EINVAL, P + "needs n >= 2");
            if (ld_of(b) < n) return fail(FNN_EINVAL, P + "needs ld >= n");
            if (!splits_ordering_ok(orderings + oo[(size_t)b], n, seen)) return fail(FNN_EINVAL, P + "ordering is not a permutation of 1..n");
            oo[(size_t)b + 1] = oo[(size_t)b] + n + 1;
            wo[(size_t)b + 1] = wo[(size_t)b] + (int64_t)n * (n - 1) / 2;
            if (n <= SPLITS_MAX_N) { kern.push_back(b); kmax = std::max(kmax, n); }
            else todo.push_back(b);
        }
    }
    st.n_problems = batch;
    WeightStage res(batch, (size_t)wo[(size_t)batch]);
    int32_t rc = be.open(device);
    if (rc != FNN_OK) return fail(rc, W + be.err());
    int64_t bad = -1;  // the lowest caller's index whose distances the kernel found non-finite
    if (kern.empty() || !small_splits_route(kmax, (int64_t)kern.size())) {
        todo.insert(todo.end(), kern.begin(), kern.end());
    } else {
        auto cap_of = [&](int64_t b) { return small_splits_cap(ns[b]); };
        auto pitch_of = [&](int64_t b) { return small_splits_work(ns[b], cap_of(b)).pitch; };
        auto img_of = [&](int64_t b) { return round_up((int64_t)ns[b] * ns[b], 2); };  // every problem 16-byte aligned in the image
        const std::vector<int64_t> cut = ragged_chunks(kern, [&](int64_t b) { return 8 * pitch_of(b); });
        int64_t mcnt = 0, mwork = 0, mout = 0, mord = 0, mimg = 0;  // the largest chunk
        for (size_t c = 0; c + 1 < cut.size(); c++) {
            int64_t work = 0, out = 0, ord = 0, img = 0;
            for (int64_t k = cut[c]; k < cut[c + 1]; k++) {
                const int64_t b = kern[(size_t)k];
                work += pitch_of(b); out += wo[(size_t)b + 1] - wo[(size_t)b]; ord += ns[b] + 1; img += img_of(b);
            }
            mcnt = std::max(mcnt, cut[c + 1] - cut[c]); mwork = std::max(mwork, work); mout = std::max(mout, out);
            mord = std::max(mord, ord); mimg = std::max(mimg, img);
        }
        st.workspace_bytes = 8 * mwork;
        double* d_work = (double*)be.alloc(sizeof(double) * (size_t)mwork);
        double* d_out = (double*)be.alloc(sizeof(double) * (size_t)mout);
        int32_t* d_ord = (int32_t*)be.alloc(sizeof(int32_t) * (size_t)mord);
        SplitsMeta* d_meta = (SplitsMeta*)be.alloc(sizeof(SplitsMeta) * (size_t)mcnt);
        RaggedDesc* d_desc = (RaggedDesc*)be.alloc(sizeof(RaggedDesc) * (size_t)mcnt);
        double* d_D = on_device ? nullptr : (double*)be.alloc(sizeof(double) * (size_t)mimg);
        if (!d_work || !d_out || !d_ord || !d_meta || !d_desc || (!on_device && !d_D)) return fail(FNN_ENOMEM, W + "device allocation failed");
        std::unique_ptr<double[]> pack(on_device ? nullptr : new double[(size_t)mimg]);
        std::vector<int32_t> ords((size_t)mord);
        std::vector<SplitsMeta> meta((size_t)mcnt);
        std::vector<double> outs((size_t)mout);
        std::vector<RaggedDesc> slot, sorted;  // the chunk's descriptors in the caller's order / in launch order
        std::vector<RaggedClass> classes;
        const int32_t threads_switch = batch_threads_switch();
        for (size_t c = 0; c + 1 < cut.size() && bad < 0; c++) {
            const int64_t cnt = cut[c + 1] - cut[c];
            slot.clear();
            int64_t work = 0, out = 0, ord = 0, img = 0;
            const double tu = now_s();
            for (int64_t k = 0; k < cnt; k++) {
                const int64_t b = kern[(size_t)(cut[c] + k)];
                const int32_t n = ns[b];
                RaggedDesc d{};
                d.id = b; d.n = n; d.cap = cap_of(b);
                d.meta = k; d.ord = ord; d.out = out; d.work = work;
                std::memcpy(&ords[(size_t)ord], orderings + oo[(size_t)b], sizeof(int32_t) * (size_t)(n + 1));
                if (on_device) {
                    d.src = offsets[b]; d.ld = ld_of(b);
                } else {
                    pack_rows(&pack[(size_t)img], n, D + offsets[b], ld_of(b), n);
                    d.src = img; d.ld = n;
                    img += img_of(b);
                }
                work += pitch_of(b); out += wo[(size_t)b + 1] - wo[(size_t)b]; ord += n + 1;
                slot.push_back(d);
            }
            sorted = slot;
            ragged_classes(sorted, threads_switch, [](const RaggedDesc& d) { return small_splits_layout(d.n, d.cap).bytes; }, classes);
            if ((int64_t)classes.size() > RAGGED_MAX_CLASSES) return fail(FNN_ESTATE, W + "more size classes than launches allowed");
            if ((!on_device && be.h2d(d_D, pack.get(), sizeof(double) * (size_t)img) != FNN_OK) ||
                be.h2d(d_ord, ords.data(), sizeof(int32_t) * (size_t)ord) != FNN_OK ||
                be.h2d(d_desc, sorted.data(), sizeof(RaggedDesc) * (size_t)cnt) != FNN_OK)
                return fail(FNN_EHIP, W + "upload failed (" + be.err() + ")");
            st.t_upload_s += now_s() - tu;
            double tk = 0.0;
            if (be.run_splits_ragged(on_device ? D : d_D, d_desc, classes.data(), (int32_t)classes.size(), d_ord, d_work, d_out, d_meta, &tk) != FNN_OK)
                return fail(FNN_EHIP, W + "kernel failed (" + be.err() + ")");
            st.t_kernel_s += tk;
            st.chunks += (int32_t)classes.size();
            if (classes[0].lds_bytes > st.lds_bytes) {
                st.lds_bytes = classes[0].lds_bytes; st.block_threads = classes[0].threads; st.capacity = sorted[0].cap;
            }
            if (be.d2h(meta.data(), d_meta, sizeof(SplitsMeta) * (size_t)cnt) != FNN_OK ||
                be.d2h(outs.data(), d_out, sizeof(double) * (size_t)out) != FNN_OK)
                return fail(FNN_EHIP, W + "download failed (" + be.err() + ")");
            for (const RaggedDesc& d : slot) {
                const SplitsTaken t = small_splits_take(meta[(size_t)d.meta], &outs[(size_t)d.out], wo[(size_t)d.id + 1] - wo[(size_t)d.id], d.cap,
                                                        &res.wts[(size_t)wo[(size_t)d.id]], res.sws[(size_t)d.id], st);
                if (t == SPLITS_NONFINITE) { bad = d.id; break; }
                if (t == SPLITS_TO_SINGLE) todo.push_back(d.id);
            }
        }
    }
    // what the kernel did not take or gave up on: one by one through the one-problem solver, on a dense host copy, in the
    // caller's order (after a non-finite problem only those in front of it: fnn_last_error() names the lowest failure)
    std::sort(todo.begin(), todo.end());
    SplitsSingle single;
    for (int64_t b : todo) {
        if (bad >= 0 && b > bad) break;
        rc = single.run(be, W, b, D + offsets[b], on_device, ns[b], ld_of(b), orderings + oo[(size_t)b], device, &res.wts[(size_t)wo[(size_t)b]],
                        &res.sws[(size_t)b], st);
        if (rc != FNN_OK) return rc;
    }
    if (bad >= 0) return fail_nonfinite(W, bad);
    res.commit(weights_out, stats_out);
    st.t_total_s = now_s() - t0;
    if (stats) *stats = st;
    return single.result(W);
}

}  // namespace fnn
#endif

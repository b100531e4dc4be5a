// fnn_splits_batch_emu.cpp -- TEST INFRASTRUCTURE: CPU driver of the batched circular split weights (one workgroup per
// problem; fastneighbornet_amd/csrc/fnn_small_splits.h).
//
// Runs the per-thread phase bodies for tid = 0 ... nthreads-1, phase by phase (a barrier of the kernel is the end of such a
// loop), through the product's own sequence (small_splits_problem) under the product's own host logic
// (small_splits_batch<B>): argument checks, packing, chunking, collection.  "Device memory" is the heap.  Each problem's
// LDS image is a heap block of exactly the size the kernel declares and its workspace slice a heap block of exactly
// small_splits_work(n, cap).pitch doubles, both filled with 0xFF bytes first: under AddressSanitizer an index past either
// is an error, and a word read before it is written is a NaN or -1 that the checks of the weights notice.
//
// Build: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off (tests/splits_batch_common.py).  Same signatures as
// include/fastnn.h with the prefix emu_.  There is no one-problem solver behind the driver: a problem that the kernel's
// method gives up on (and any n above the limit) fails the call with FNN_ECAPACITY; emu_split_weights_batch_giveups says
// which problems of the last call gave up, and why.
#include "fnn_small_emu.h"

namespace {

using namespace fnn;

thread_local std::vector<int32_t> g_giveups;  // FNN_SW_GIVEUP_* per problem of the last call that reached the kernel
thread_local std::vector<int32_t> g_counts;   // ... and its six safety-net counts (the host keeps them for solved problems only)

struct EmuSplitsBackend : EmuHeapBackend {
    int64_t done = 0;  // problems of earlier chunks
    int32_t run_splits(const double* D, int32_t n, int64_t ld, int64_t stride, const int32_t* ord, int64_t cnt, int32_t cap, int32_t threads,
                       int32_t lds_bytes, double* work, int64_t pitch, double* out, SplitsMeta* meta, double* t_kernel_s) {
        const double t0 = now_s();
        const SplitsSwitches sw = small_splits_switches();
        const int64_t N = (int64_t)n * (n - 1) / 2;
        for (int64_t b = 0; b < cnt; b++) {
            if (!emu_splits_problem(threads, lds_bytes, pitch, n, cap, sw, D + b * stride, ld, ord + b * (n + 1), out + b * N, meta + b)) {
                last = "out of memory";
                return FNN_ENOMEM;
            }
            g_giveups[(size_t)(done + b)] = meta[b].giveup;
            const int32_t cnt6[6] = {meta[b].aside_fresh, meta[b].aside_rebuild, meta[b].aside_enter, meta[b].rechecks, meta[b].releases, meta[b].departed};
            std::memcpy(&g_counts[(size_t)(done + b) * 6], cnt6, sizeof(cnt6));
        }
        (void)work;
        done += cnt;
        *t_kernel_s = now_s() - t0;
        return FNN_OK;
    }
    int32_t single(const double*, int32_t n, const int32_t*, int32_t, double*, fnn_sw_stats*) {
        return fail(FNN_ECAPACITY, "the kernel's method gave up or n = " + std::to_string(n) + " is above its limit, and the CPU driver has no one-problem solver");
    }
};

int32_t entry(const char* who, const double* D, bool on_device, int32_t n, int64_t ld, int64_t stride, int64_t batch, const int32_t* orderings,
              int32_t device, double* weights_out, fnn_sw_stats* stats_out, fnn_sw_batch_stats* stats) {
    try {
        g_giveups.assign(batch > 0 ? (size_t)batch : 0, 0);
        g_counts.assign(batch > 0 ? (size_t)batch * 6 : 0, 0);
        EmuSplitsBackend be;
        return small_splits_batch(be, who, D, on_device, n, ld, stride, batch, orderings, device, weights_out, stats_out, stats);
    } catch (const std::exception& e) {
        return fail(FNN_ESTATE, std::string("exception: ") + e.what());
    }
}

}  // namespace

extern "C" {

const char* emu_last_error(void) { return fnn::g_last_error.c_str(); }
int32_t emu_split_weights_batch_max_n(void) { return fnn::SPLITS_MAX_N; }
int64_t emu_split_weights_batch_min_batch(int32_t n) { return fnn::small_splits_min_batch(n); }

int32_t emu_split_weights_batch_f64(const double* D, int32_t n, int64_t ld, int64_t stride, int64_t batch, const int32_t* orderings, int32_t device,
                                    double* weights_out, fnn_sw_stats* stats_out, fnn_sw_batch_stats* stats) {
    return entry("emu_split_weights_batch_f64", D, false, n, ld, stride, batch, orderings, device, weights_out, stats_out, stats);
}

// (the "device" pointer is host memory here: the kernel's reorder reads it in place through ld and stride)
int32_t emu_split_weights_batch_device_f64(const double* D, int32_t n, int64_t ld, int64_t stride, int64_t batch, const int32_t* orderings,
                                           int32_t device, double* weights_out, fnn_sw_stats* stats_out, fnn_sw_batch_stats* stats) {
    return entry("emu_split_weights_batch_device_f64", D, true, n, ld, stride, batch, orderings, device, weights_out, stats_out, stats);
}

// FNN_SW_GIVEUP_* of the first `cnt` problems of this thread's last call (0: solved); returns how many problems it had
int64_t emu_split_weights_batch_giveups(int32_t* out, int64_t cnt) {
    for (int64_t b = 0; b < cnt && b < (int64_t)g_giveups.size(); b++) out[b] = g_giveups[(size_t)b];
    return (int64_t)g_giveups.size();
}

// per problem of this thread's last call, given up or not: {set aside on a fresh append, on a rebuild, in the entering step,
// rechecks, releases, departed}; returns how many problems it had
int64_t emu_split_weights_batch_counts(int32_t* out, int64_t cnt) {
    for (int64_t b = 0; b < cnt && b < (int64_t)g_giveups.size(); b++) std::memcpy(out + b * 6, &g_counts[(size_t)b * 6], sizeof(int32_t) * 6);
    return (int64_t)g_giveups.size();
}

// ---- phase-level entries: the phase bodies on a crafted free set, for the paths that no whole problem reaches
// (tests/test_splits_phases.py through tests/emu/fnn_splits_phase_main.cpp).  The view is carved from heap blocks of
// exactly the kernel's sizes, filled with 0xFF bytes, as in run_splits.
namespace {
struct PhaseView {
    EmuBlock lds, slice;
    SplitsView V;
    PhaseView(int32_t n, double dep, int32_t max_steps)
        : lds((size_t)small_splits_layout(n, small_splits_capacity(n)).bytes),
          slice(sizeof(double) * (size_t)small_splits_work(n, small_splits_capacity(n)).pitch) {
        if (!lds.p || !slice.p) std::abort();
        V = small_splits_view(lds.bytes(), slice.doubles(), n, small_splits_capacity(n));
        splits_init(0, 1, V, SplitsSwitches{dep, max_steps, 0});
    }
};
}  // namespace

// One pass of the solver's inner loop behind splits_solve: splits_ratio_min, splits_fold_ratio and, when a member leaves,
// splits_ratio_step and splits_compact, on members 0 ... f - 1 (grid index Fi, weight xF, sub-problem solution sF, cF).
// ctl in: {enter_pos, departed, n_aside, steps, max_steps}; ctl out: {leave, action, f, ftot, enter_pos, departed,
// n_aside, aside_enter, steps}.  gx and mask are the n x n grids.  Returns 0, or -1 for sizes outside the view.
int32_t emu_splits_ratio_pass(int32_t n, int32_t threads, int32_t f, const int32_t* ctl_in, int32_t* ctl_out, double* alpha_out, int32_t* Fi, double* xF,
                              const double* sF, double* cF, double* gx, uint8_t* mask) {
    if (n < 2 || n > fnn::SPLITS_MAX_N || f < 1 || f > fnn::small_splits_capacity(n) || threads < 1 || threads > 1024) return -1;
    PhaseView P(n, fnn::SPLITS_DEP_REL, ctl_in[4]);
    const SplitsView& V = P.V;
    SplitsCtl& K = *V.ctl;
    K.enter_pos = ctl_in[0]; K.departed = ctl_in[1]; K.n_aside = ctl_in[2]; K.steps = ctl_in[3];
    K.f = f; K.ftot = f;
    const size_t tot = (size_t)n * (size_t)n;
    std::memcpy(V.Fi, Fi, sizeof(int32_t) * (size_t)f);
    std::memcpy(V.xF, xF, sizeof(double) * (size_t)f);
    std::memcpy(V.sF, sF, sizeof(double) * (size_t)f);
    std::memcpy(V.cF, cF, sizeof(double) * (size_t)f);
    std::memcpy(V.gx, gx, sizeof(double) * tot);
    std::memcpy(V.mask, mask, tot);
    CpuSplitsExec ex{threads};
    ex.best(V, [&](int tid, int nt) { return splits_ratio_min(tid, nt, V, f); });
    ex.all([&](int tid, int nt) { splits_fold_ratio(tid, nt, V); });
    const int32_t leave = ex.get(&K.leave);
    if (ex.get(&K.action) != SPLITS_ACT_GIVEUP && leave >= 0) {
        const double alpha = ex.get(&K.alpha);
        ex.all([&](int tid, int nt) { splits_ratio_step(tid, nt, V, f, alpha, leave); });
        ex.all([&](int tid, int nt) { splits_compact(tid, nt, V, f); });
    }
    const int32_t out[9] = {K.leave, K.action, K.f, K.ftot, K.enter_pos, K.departed, K.n_aside, K.aside_enter, K.steps};
    std::memcpy(ctl_out, out, sizeof(out));
    *alpha_out = K.alpha;
    std::memcpy(Fi, V.Fi, sizeof(int32_t) * (size_t)f);
    std::memcpy(xF, V.xF, sizeof(double) * (size_t)f);
    std::memcpy(cF, V.cF, sizeof(double) * (size_t)f);
    std::memcpy(gx, V.gx, sizeof(double) * tot);
    std::memcpy(mask, V.mask, tot);
    return 0;
}

// splits_append_row for position r of ftot members, positions below r in the factor, with the quantities the three phases
// in front of it leave: rv = l^T W (r entries), ll = l.l, lz = l.z, hkk = H_kk.  ctl in: {enter_pos, departed, n_aside,
// entered, peak}; ctl out: {f, ftot, enter_pos, departed, n_aside, entered, peak, aside_fresh, aside_rebuild}.  w_row
// (r + 1 entries) and *z_r are written when the split enters the factor, and left alone when it is set aside.
int32_t emu_splits_append_row(int32_t n, int32_t threads, int32_t r, int32_t ftot, int32_t fresh, double dep, double hkk, double ll, double lz,
                              const double* rv, const int32_t* ctl_in, int32_t* ctl_out, int32_t* Fi, double* xF, double* cF, double* gx, uint8_t* mask,
                              double* w_row, double* z_r) {
    if (n < 2 || n > fnn::SPLITS_MAX_N || r < 0 || r >= ftot || ftot > fnn::small_splits_capacity(n) || threads < 1 || threads > 1024) return -1;
    PhaseView P(n, dep, 0);
    const SplitsView& V = P.V;
    SplitsCtl& K = *V.ctl;
    K.enter_pos = ctl_in[0]; K.departed = ctl_in[1]; K.n_aside = ctl_in[2]; K.entered = ctl_in[3]; K.peak = ctl_in[4];
    K.f = r; K.ftot = ftot; K.hkk = hkk; K.ll = ll; K.lz = lz;
    const size_t tot = (size_t)n * (size_t)n;
    std::memcpy(V.Fi, Fi, sizeof(int32_t) * (size_t)ftot);
    std::memcpy(V.xF, xF, sizeof(double) * (size_t)ftot);
    std::memcpy(V.cF, cF, sizeof(double) * (size_t)ftot);
    if (r > 0) std::memcpy(V.rv, rv, sizeof(double) * (size_t)r);  // (r == 0: rv may be NULL)
    std::memcpy(V.gx, gx, sizeof(double) * tot);
    std::memcpy(V.mask, mask, tot);
    double* w = V.W + (int64_t)r * V.cap;
    std::memcpy(w, w_row, sizeof(double) * (size_t)(r + 1));
    V.zF[r] = *z_r;
    CpuSplitsExec ex{threads};
    ex.all([&](int tid, int nt) { splits_append_row(tid, nt, V, r, ftot, fresh); });
    const int32_t out[9] = {K.f, K.ftot, K.enter_pos, K.departed, K.n_aside, K.entered, K.peak, K.aside_fresh, K.aside_rebuild};
    std::memcpy(ctl_out, out, sizeof(out));
    std::memcpy(Fi, V.Fi, sizeof(int32_t) * (size_t)ftot);
    std::memcpy(xF, V.xF, sizeof(double) * (size_t)ftot);
    std::memcpy(cF, V.cF, sizeof(double) * (size_t)ftot);
    std::memcpy(gx, V.gx, sizeof(double) * tot);
    std::memcpy(mask, V.mask, tot);
    std::memcpy(w_row, w, sizeof(double) * (size_t)(r + 1));
    *z_r = V.zF[r];
    return 0;
}

}  // extern "C"

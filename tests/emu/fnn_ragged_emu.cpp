// fnn_ragged_emu.cpp -- TEST INFRASTRUCTURE: CPU driver of the ragged batch calls (problems of different sizes in one call;
// DESIGN.md section 13).
//
// Runs the per-thread phase bodies of fastneighbornet_amd/csrc/fnn_small.h and fnn_small_splits.h for tid = 0 ... nthreads-1,
// phase by phase (a barrier of the kernel is the end of such a loop), under the product's own host logic
// (small_ragged<B>, small_splits_ragged<B>): argument checks, chunking, size classes, descriptors, collection.  A "launch"
// walks the class's descriptors as the kernel's workgroups do.  "Device memory" is the heap.  Each problem's LDS image is a
// heap block of exactly the size its OWN layout needs (never more than its class reserves: that is checked), and a split
// problem's workspace slice and weights are heap blocks of exactly their size, all filled with 0xFF bytes first: under
// AddressSanitizer an index past a layout is an error, and a word read before it is written is a NaN or -1 that the
// comparison with the oracle notices.
//
// Build: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off (tests/ragged_common.py).  Same signatures as include/fastnn.h
// with the prefix emu_.  There is no same-size entry, one-problem engine or one-problem solver behind the driver: an order
// problem above the LDS limit fails the call with FNN_EINVAL, a split problem that the kernel's method gives up on (and any
// n above its limit) with FNN_ECAPACITY; emu_split_weights_ragged_giveups says which problems of the last call gave up.
#include "fnn_small_emu.h"

namespace {

using namespace fnn;

thread_local std::vector<int32_t> g_giveups;  // FNN_SW_GIVEUP_* per problem (caller's index) of the last call that reached the kernel

struct EmuRaggedBackend : EmuHeapBackend {
    int32_t validate_ragged(const double* base, const RaggedDesc* desc, int64_t cnt, int64_t* bad) {
        *bad = -1;
        for (int64_t k = 0; k < cnt; k++)  // (any order: the kernel takes the minimum index)
            for (int t = 0; t < 256; t++)
                if (small_validate_thread(t, 256, base + desc[k].src, desc[k].n, desc[k].ld) && (*bad < 0 || desc[k].id < *bad)) *bad = desc[k].id;
        return FNN_OK;
    }
    int32_t run_ragged(const double* base, const RaggedDesc* desc, const RaggedClass* cls, int32_t ncls, int32_t* meta, Agg3Rec* log, Event* ev,
                       double* t_kernel_s) {
        const double t0 = now_s();
        for (int32_t c = 0; c < ncls; c++)
            for (int64_t k = 0; k < cls[c].count; k++) {
                const RaggedDesc d = desc[cls[c].first + k];
                const int32_t bytes = small_layout(d.n).bytes, threads = cls[c].threads;
                if (bytes > cls[c].lds_bytes) { last = "a class reserves less LDS than one of its problems needs"; return FNN_ESTATE; }
                EmuBlock lds((size_t)bytes);
                if (!lds.p) { last = "out of memory"; return FNN_ENOMEM; }
                const SmallView V = small_view(lds.bytes(), d.n);
                for (int t = 0; t < threads; t++) small_load(t, threads, V, base + d.src, d.ld, d.vec);
                CpuExec ex{threads};
                small_problem(ex, V, ev ? ev + d.ev : nullptr, meta + d.meta, log + d.log);
            }
        *t_kernel_s = now_s() - t0;
        return FNN_OK;
    }
    int32_t large(const std::string& W, const double*, bool, int32_t n, const int64_t*, const int64_t*, int64_t, const fnn_opts&, bool, int32_t*,
                  fnn_event*, int32_t*, fnn_batch_stats*, int64_t*) {
        return fail(FNN_EINVAL, W + "the CPU driver has no same-size entry for n = " + std::to_string(n) + " above the LDS limit");
    }
    int32_t run_splits_ragged(const double* base, const RaggedDesc* desc, const RaggedClass* cls, int32_t ncls, const int32_t* ord, double* work,
                              double* out, SplitsMeta* meta, double* t_kernel_s) {
        const double t0 = now_s();
        const SplitsSwitches sw = small_splits_switches();
        for (int32_t c = 0; c < ncls; c++)
            for (int64_t k = 0; k < cls[c].count; k++) {
                const RaggedDesc d = desc[cls[c].first + k];
                const int32_t bytes = small_splits_layout(d.n, d.cap).bytes, threads = cls[c].threads;
                if (bytes > cls[c].lds_bytes) { last = "a class reserves less LDS than one of its problems needs"; return FNN_ESTATE; }
                if (!emu_splits_problem(threads, bytes, small_splits_work(d.n, d.cap).pitch, d.n, d.cap, sw, base + d.src, d.ld, ord + d.ord, out + d.out,
                                        meta + d.meta)) {
                    last = "out of memory";
                    return FNN_ENOMEM;
                }
                if ((size_t)d.id < g_giveups.size()) g_giveups[(size_t)d.id] = meta[d.meta].giveup;
            }
        (void)work;
        *t_kernel_s = now_s() - t0;
        return FNN_OK;
    }
    int32_t single(const double*, int32_t n, const int32_t*, int32_t, double*, fnn_sw_stats*) {
        return fail(FNN_ECAPACITY, "the kernel's method gave up or n = " + std::to_string(n) + " is above its limit, and the CPU driver has no one-problem solver");
    }
};

int32_t orders_entry(const char* who, const double* D, bool on_device, const int64_t* offsets, const int32_t* n, const int64_t* ld, int64_t batch,
                     const fnn_opts* opts, int32_t* orders_out, fnn_event* events_out, int32_t* nevents_out, fnn_batch_stats* stats) {
    try {
        EmuRaggedBackend be;
        return small_ragged(be, who, D, on_device, offsets, n, ld, batch, opts, orders_out, events_out, nevents_out, stats);
    } catch (const std::exception& e) {
        return fail(FNN_ESTATE, std::string("exception: ") + e.what());
    }
}

int32_t weights_entry(const char* who, const double* D, bool on_device, const int64_t* offsets, const int32_t* n, const int64_t* ld, int64_t batch,
                      const int32_t* orderings, int32_t device, double* weights_out, fnn_sw_stats* stats_out, fnn_sw_batch_stats* stats) {
    try {
        g_giveups.assign(batch > 0 ? (size_t)batch : 0, 0);
        EmuRaggedBackend be;
        return small_splits_ragged(be, who, D, on_device, offsets, n, ld, batch, orderings, device, weights_out, stats_out, stats);
    } catch (const std::exception& e) {
        return fail(FNN_ESTATE, std::string("exception: ") + e.what());
    }
}

}  // namespace

extern "C" {

const char* emu_last_error(void) { return fnn::g_last_error.c_str(); }
int32_t emu_batch_lds_max_n(void) { return fnn::SMALL_LDS_MAX_N; }
int32_t emu_split_weights_batch_max_n(void) { return fnn::SPLITS_MAX_N; }
int64_t emu_split_weights_batch_min_batch(int32_t n) { return fnn::small_splits_min_batch(n); }

int32_t emu_canonical_order_ragged_f64(const double* D, const int64_t* offsets, const int32_t* n, const int64_t* ld, int64_t batch, const fnn_opts* opts,
                                       int32_t* orders_out, fnn_event* events_out, int32_t* nevents_out, fnn_batch_stats* stats) {
    return orders_entry("emu_canonical_order_ragged_f64", D, false, offsets, n, ld, batch, opts, orders_out, events_out, nevents_out, stats);
}

// (the "device" pointer is host memory here: the matrices are read in place, through offsets and ld)
int32_t emu_canonical_order_ragged_device_f64(const double* D, const int64_t* offsets, const int32_t* n, const int64_t* ld, int64_t batch,
                                              const fnn_opts* opts, int32_t* orders_out, fnn_event* events_out, int32_t* nevents_out,
                                              fnn_batch_stats* stats) {
    return orders_entry("emu_canonical_order_ragged_device_f64", D, true, offsets, n, ld, batch, opts, orders_out, events_out, nevents_out, stats);
}

int32_t emu_split_weights_ragged_f64(const double* D, const int64_t* offsets, const int32_t* n, const int64_t* ld, int64_t batch, const int32_t* orderings,
                                     int32_t device, double* weights_out, fnn_sw_stats* stats_out, fnn_sw_batch_stats* stats) {
    return weights_entry("emu_split_weights_ragged_f64", D, false, offsets, n, ld, batch, orderings, device, weights_out, stats_out, stats);
}

int32_t emu_split_weights_ragged_device_f64(const double* D, const int64_t* offsets, const int32_t* n, const int64_t* ld, int64_t batch,
                                            const int32_t* orderings, int32_t device, double* weights_out, fnn_sw_stats* stats_out,
                                            fnn_sw_batch_stats* stats) {
    return weights_entry("emu_split_weights_ragged_device_f64", D, true, offsets, n, ld, batch, orderings, device, weights_out, stats_out, stats);
}

// FNN_SW_GIVEUP_* of the first `cnt` problems of this thread's last weight call (0: solved); returns how many problems it had
int64_t emu_split_weights_ragged_giveups(int32_t* out, int64_t cnt) {
    for (int64_t b = 0; b < cnt && b < (int64_t)g_giveups.size(); b++) out[b] = g_giveups[(size_t)b];
    return (int64_t)g_giveups.size();
}

}  // extern "C"

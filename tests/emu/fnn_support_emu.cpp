// fnn_support_emu.cpp -- TEST INFRASTRUCTURE: CPU driver of the split-support path.
//
// Runs the per-thread steps of fastneighbornet_amd/csrc/fnn_support.h for every thread of every workgroup of every launch
// of the kernel route, under the same host logic as the product (support_call<B>): argument checks, chunking, hash
// repeats, the carry across chunks, the host route.  A barrier of a kernel is the end of a loop over the threads; a ballot
// is the loop over a wave's lanes; the integer atomics are the plain operations (one thread runs at a time).  "Device
// memory" is the heap: every buffer has exactly the size the host logic asks for and is filled with 0xFF bytes first
// (fnn_small_emu.h), the LDS image of a workgroup is a block of exactly sup_lds_bytes: under AddressSanitizer an index past
// a layout is an error.  emu_support_set_reverse(1) runs the workgroups of every launch from the last to the first: the
// table must not depend on the order in which workgroups run.
//
// Build: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off (tests/support_common.py).  Same signatures as include/fastnn.h
// with the prefix emu_.
#include "../../fastneighbornet_amd/csrc/fnn_support.h"
#include "fnn_small_emu.h"

namespace {

using namespace fnn;

bool g_reverse = false;

struct EmuSupBackend : EmuHeapBackend {
    void release(void* p) {
        for (size_t q = 0; q < bufs.size(); q++)
            if (bufs[q] == p) { bufs.erase(bufs.begin() + (long)q); break; }
        std::free(p);
    }
    int32_t fill(void* p, int byte, size_t bytes) { std::memset(p, byte, bytes); return FNN_OK; }

    template <class F>
    static void grid(int64_t blocks, F block) {
        for (int64_t q = 0; q < blocks; q++) block(g_reverse ? blocks - 1 - q : q);
    }
    template <class F>
    static void flat(int64_t items, F thread) {
        grid((items + SUP_THREADS - 1) / SUP_THREADS, [&](int64_t blk) {
            for (int t = 0; t < SUP_THREADS; t++) thread((uint32_t)(blk * SUP_THREADS + t));
        });
    }
    bool emit_block(const SupArgs& a, int64_t bl) {
        EmuBlock lds((size_t)sup_lds_bytes(a.n, a.words));
        if (!lds.p) return false;
        const SupLds L = sup_lds_view(lds.bytes(), a.n, a.words);
        for (int t = 0; t < SUP_THREADS; t++) sup_emit_load(a, L, bl, t, SUP_THREADS);
        for (int t = 0; t < SUP_THREADS; t++) sup_emit_prefix(a, L, t);
        uint32_t base = a.recbase[bl];
        for (int64_t k0 = 0; k0 < a.K; k0 += SUP_THREADS) {
            bool f[SUP_THREADS];
            for (int v = 0; v < SUP_WAVES; v++) {
                uint64_t m = 0;
                for (int lane = 0; lane < 64; lane++) {
                    const int64_t k = k0 + 64 * v + lane;
                    f[64 * v + lane] = k < a.K && sup_counts(a, bl, k);
                    if (f[64 * v + lane]) m |= 1ull << lane;
                }
                L.wmask[v] = m;
            }
            uint32_t total = 0;
            for (int t = 0; t < SUP_THREADS; t++) {
                const uint32_t place = sup_emit_place(L.wmask, t, &total);
                if (f[t]) sup_emit_record(a, L.P, bl, k0 + t, base + place);
            }
            base += total;
        }
        return true;
    }
    int32_t run(int kernel, const SupArgs& a, int64_t items, double* t_kernel_s) {
        const double t0 = now_s();
        bool ok = true;
        switch (kernel) {
            case SUP_K_COUNT:
                grid(items, [&](int64_t bl) { for (int t = 0; t < SUP_THREADS; t++) sup_count_thread(a, bl, t, SUP_THREADS); });
                break;
            case SUP_K_EMIT: grid(items, [&](int64_t bl) { ok = emit_block(a, bl) && ok; }); break;
            case SUP_K_VERIFY: flat(items, [&](uint32_t g) { sup_verify_thread(a, g); }); break;
            case SUP_K_SCAN_SUMS:
                grid(items, [&](int64_t blk) { for (int t = 0; t < SUP_THREADS; t++) sup_scan_sums_thread(a, blk, t); });
                break;
            case SUP_K_SCAN_APPLY:
                grid(items, [&](int64_t blk) {
                    uint32_t part[SUP_THREADS];
                    for (int t = 0; t < SUP_THREADS; t++) part[t] = sup_scan_own(a, blk, t);
                    for (int t = 0; t < SUP_THREADS; t++) sup_scan_apply_thread(a, blk, t, part);
                });
                break;
            case SUP_K_ROWS: flat(items, [&](uint32_t g) { sup_rows_thread(a, g); }); break;
            case SUP_K_SCATTER: flat(items, [&](uint32_t g) { sup_scatter_thread(a, g); }); break;
            case SUP_K_RANK: flat(items, [&](uint32_t g) { sup_rank_thread(a, g); }); break;
            case SUP_K_SUM: flat(items, [&](uint32_t g) { sup_sum_thread(a, g); }); break;
            default: last = "no such kernel"; return FNN_EHIP;
        }
        if (!ok) { last = "out of memory"; return FNN_EHIP; }
        *t_kernel_s = now_s() - t0;
        return FNN_OK;
    }
};

}  // namespace

extern "C" {

const char* emu_last_error(void) { return fnn::g_last_error.c_str(); }
void emu_support_set_reverse(int32_t on) { g_reverse = on != 0; }
int32_t emu_split_support_max_n(void) { return fnn::SUP_MAX_N; }
int64_t emu_split_support_min_work(void) { return fnn::SUP_MIN_WORK; }

int32_t emu_split_support_f64(int32_t n, int64_t batch, const int32_t* orderings, const double* weights, double threshold, int64_t lead, int32_t device,
                              uint64_t* keys_out, int64_t* first_b_out, int64_t* first_k_out, int64_t* counts_out, double* weight_sum_out,
                              int64_t capacity, int64_t* count_out, fnn_support_stats* stats) {
    try {
        EmuSupBackend be;
        return fnn::support_call(be, "emu_split_support_f64", n, batch, orderings, weights, false, threshold, lead, device, keys_out, first_b_out,
                                 first_k_out, counts_out, weight_sum_out, capacity, count_out, stats);
    } catch (const std::exception& e) {
        return fnn::fail(FNN_ESTATE, std::string("exception: ") + e.what());
    }
}

// (the "device" pointer is host memory here: the weights are read in place)
int32_t emu_split_support_device_f64(int32_t n, int64_t batch, const int32_t* orderings, const double* d_weights, double threshold, int64_t lead,
                                     int32_t device, uint64_t* keys_out, int64_t* first_b_out, int64_t* first_k_out, int64_t* counts_out,
                                     double* weight_sum_out, int64_t capacity, int64_t* count_out, fnn_support_stats* stats) {
    try {
        EmuSupBackend be;
        return fnn::support_call(be, "emu_split_support_device_f64", n, batch, orderings, d_weights, true, threshold, lead, device, keys_out,
                                 first_b_out, first_k_out, counts_out, weight_sum_out, capacity, count_out, stats);
    } catch (const std::exception& e) {
        return fnn::fail(FNN_ESTATE, std::string("exception: ") + e.what());
    }
}

int32_t emu_split_keys(int32_t n, const int32_t* ordering, const int64_t* k, int64_t count, uint64_t* keys_out) {
    try {
        return fnn::sup_split_keys("emu_split_keys", n, ordering, k, count, keys_out);
    } catch (const std::exception& e) {
        return fnn::fail(FNN_ESTATE, std::string("exception: ") + e.what());
    }
}

}  // extern "C"

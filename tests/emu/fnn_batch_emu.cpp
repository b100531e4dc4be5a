// fnn_batch_emu.cpp -- TEST INFRASTRUCTURE: CPU driver of the batched small-problem path.
//
// Runs the per-thread phase bodies of fastneighbornet_amd/csrc/fnn_small.h for tid = 0 ... nthreads-1, phase by phase
// (a barrier of the kernel is the end of such a loop), under the same host logic as the product (small_batch<B>):
// argument checks, chunking, validation, expansion.  "Device memory" is the heap, and each problem's LDS image is a heap
// block of exactly the size the kernel declares, filled with 0xFF bytes first (fnn_small_emu.h): under AddressSanitizer an
// index past the layout is an error, and a word read before it is written is a NaN or -1 that the comparison with the
// oracle notices.
//
// Build: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off (tests/test_batch_emu.py).  Same signatures as include/fastnn.h
// with the prefix emu_.
#include "fnn_small_emu.h"

namespace {

using namespace fnn;

struct EmuBatchBackend : EmuHeapBackend {
    int32_t validate(const double* D, int32_t n, int64_t ld, int64_t stride, int64_t cnt, int64_t* bad) {
        *bad = -1;
        for (int64_t b = cnt; b-- > 0;)  // (any order: the kernel takes the minimum index)
            for (int t = 0; t < 256; t++)
                if (small_validate_thread(t, 256, D + b * stride, n, ld)) *bad = b;
        return FNN_OK;
    }
    int32_t run(const double* D, int32_t n, int64_t ld, int64_t stride, int64_t cnt, int32_t threads, int32_t lds_bytes,
                int32_t* meta, Agg3Rec* log, Event* ev, double* t_kernel_s) {
        const int32_t vec = (ld == n && stride % 2 == 0 && reinterpret_cast<uintptr_t>(D) % 16 == 0) ? 1 : 0;
        const double t0 = now_s();
        for (int64_t b = 0; b < cnt; b++) {
            EmuBlock lds((size_t)lds_bytes);
            if (!lds.p) { last = "out of memory"; return FNN_ENOMEM; }
            const SmallView V = small_view(lds.bytes(), n);
            for (int t = 0; t < threads; t++) small_load(t, threads, V, D + b * stride, ld, vec);
            CpuExec ex{threads};
            small_problem(ex, V, ev ? ev + b * n : nullptr, meta + b * SMALL_META_INTS, log + b * n);
        }
        *t_kernel_s = now_s() - t0;
        return FNN_OK;
    }
    int32_t fallback(const std::string& W, const double*, bool, int32_t, int64_t, int64_t, int64_t, const fnn_opts&, int32_t*,
                     fnn_event*, int32_t*, fnn_batch_stats&) {
        return fail(FNN_EINVAL, W + "the CPU driver has no one-problem engine for n above the LDS limit");
    }
};

}  // namespace

extern "C" {

const char* emu_last_error(void) { return fnn::g_last_error.c_str(); }
int32_t emu_batch_lds_max_n(void) { return fnn::SMALL_LDS_MAX_N; }

int32_t emu_canonical_order_batch_f64(const double* D, int32_t n, int64_t ld, int64_t stride, int64_t batch, const fnn_opts* opts,
                                      int32_t* orders_out, fnn_event* events_out, int32_t* nevents_out, fnn_batch_stats* stats) {
    try {
        EmuBatchBackend be;
        return fnn::small_batch(be, "emu_canonical_order_batch_f64", D, false, n, ld, stride, batch, opts, orders_out, events_out, nevents_out, stats);
    } catch (const std::exception& e) {
        return fnn::fail(FNN_ESTATE, std::string("exception: ") + e.what());
    }
}

// (the "device" pointer is host memory here: the matrices are read in place, through ld and stride)
int32_t emu_canonical_order_batch_device_f64(const double* D, int32_t n, int64_t ld, int64_t stride, int64_t batch, const fnn_opts* opts,
                                             int32_t* orders_out, fnn_event* events_out, int32_t* nevents_out, fnn_batch_stats* stats) {
    try {
        EmuBatchBackend be;
        return fnn::small_batch(be, "emu_canonical_order_batch_device_f64", D, true, n, ld, stride, batch, opts, orders_out, events_out, nevents_out, stats);
    } catch (const std::exception& e) {
        return fnn::fail(FNN_ESTATE, std::string("exception: ") + e.what());
    }
}

}  // extern "C"

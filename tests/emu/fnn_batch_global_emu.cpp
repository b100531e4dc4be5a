// fnn_batch_global_emu.cpp -- TEST INFRASTRUCTURE: CPU driver of the batched path above the LDS limit (the matrix in a
// working copy in global memory, everything else in LDS).
//
// Runs the per-thread phase bodies of fastneighbornet_amd/csrc/fnn_small_global.h (and those of fnn_small.h that the
// route reuses) for tid = 0 ... nthreads-1, phase by phase (a barrier of the kernel is the end of such a loop), under the
// same host logic as the product (small_global_batch<B>): argument checks, packing, chunking, validation, expansion.
// "Device memory" is the heap.  Each problem's LDS image is a heap block of exactly the size the kernel declares, filled
// with 0xFF bytes first, and each working matrix is a heap block of exactly small_global_pitch(n) doubles, filled likewise
// (the chunk's image is copied into it and, on the host entry, back): under AddressSanitizer an index past either is an
// error, and a word read before it is written is a NaN or -1 that the comparison with the oracle notices.
//
// Build: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off (tests/batch_global_common.py).  Same signatures as
// include/fastnn.h with the prefix emu_.  Calls that the product would not send down this route fail with FNN_EINVAL: the
// driver has neither the LDS kernel nor the one-problem engine.
#include "../../fastneighbornet_amd/csrc/fnn_small_global.h"
#include "fnn_small_emu.h"

namespace {

using namespace fnn;

struct CpuGlobalExec {
    int nt;
    template <class F>
    void all(F f) {
        for (int t = 0; t < nt; t++) f(t, nt);
    }
    void scan_global(const GlobalView& V, int32_t m, int32_t c) {
        for (int w = 0; w < (nt + 63) / 64; w++) {
            SmallCand b{0.0, -1, -1};
            for (int t = w * 64; t < nt && t < (w + 1) * 64; t++) {
                const SmallCand o = global_scan_thread(t, nt, V, m, c);
                if (small_before(o, b)) b = o;
            }
            V.wred[w] = b;
        }
    }
};

struct EmuGlobalBackend : EmuHeapBackend {
    int32_t validate(const double* D, int32_t n, int64_t ld, int64_t stride, int64_t cnt, int64_t* bad) {
        *bad = -1;
        for (int64_t b = cnt; b-- > 0;)  // (any order: the kernel takes the minimum index)
            for (int t = 0; t < 256; t++)
                if (small_validate_thread(t, 256, D + b * stride, n, ld)) *bad = b;
        return FNN_OK;
    }
    int32_t run_global(const double* src, int64_t ld, int64_t stride, double* work, int64_t cnt, int32_t n, int32_t threads, int32_t lds_bytes,
                       int32_t* meta, Agg3Rec* log, Event* ev, double* t_kernel_s) {
        const size_t pitch = (size_t)small_global_pitch(n);
        const double t0 = now_s();
        for (int64_t b = 0; b < cnt; b++) {
            EmuBlock lds((size_t)lds_bytes), copy(sizeof(double) * pitch);  // copy: this problem's working copy, on its own
            if (!lds.p || !copy.p) { last = "out of memory"; return FNN_ENOMEM; }
            double* mat = copy.doubles();
            const GlobalView V = small_global_view(lds.bytes(), mat, n);
            if (src != work) {
                for (int t = 0; t < threads; t++) global_copy(t, threads, V, src + b * stride, ld);
            } else {  // in place in the upload buffer: the rows (never the padding) are what the kernel finds there
                for (int32_t r = 0; r < n; r++) std::memcpy(mat + (size_t)r * V.ldm, work + (size_t)b * pitch + (size_t)r * V.ldm, sizeof(double) * (size_t)n);
            }
            CpuGlobalExec ex{threads};
            global_problem(ex, V, ev ? ev + b * n : nullptr, meta + b * SMALL_META_INTS, log + b * n);
        }
        *t_kernel_s = now_s() - t0;
        return FNN_OK;
    }
};

int32_t entry(const char* who, const double* D, bool on_device, int32_t n, int64_t ld, int64_t stride, int64_t batch, const fnn_opts* opts,
              int32_t* orders_out, fnn_event* events_out, int32_t* nevents_out, fnn_batch_stats* stats) {
    try {
        if (!small_global_route(n, batch))
            return fail(FNN_EINVAL, std::string(who) + ": not a call for the global-memory route (the CPU driver has no other)");
        EmuGlobalBackend be;
        return small_global_batch(be, who, D, on_device, n, ld, stride, batch, opts, orders_out, events_out, nevents_out, stats);
    } catch (const std::exception& e) {
        return fail(FNN_ESTATE, std::string("exception: ") + e.what());
    }
}

}  // namespace

extern "C" {

const char* emu_last_error(void) { return fnn::g_last_error.c_str(); }
int32_t emu_batch_lds_max_n(void) { return fnn::SMALL_LDS_MAX_N; }
int32_t emu_batch_global_max_n(void) { return fnn::SMALL_GLOBAL_MAX_N; }
int64_t emu_batch_global_min_batch(int32_t n) { return fnn::small_global_min_batch(n); }

int32_t emu_canonical_order_batch_f64(const double* D, int32_t n, int64_t ld, int64_t stride, int64_t batch, const fnn_opts* opts,
                                      int32_t* orders_out, fnn_event* events_out, int32_t* nevents_out, fnn_batch_stats* stats) {
    return entry("emu_canonical_order_batch_f64", D, false, n, ld, stride, batch, opts, orders_out, events_out, nevents_out, stats);
}

// (the "device" pointer is host memory here: each matrix is copied from it, through ld and stride, into a working copy)
int32_t emu_canonical_order_batch_device_f64(const double* D, int32_t n, int64_t ld, int64_t stride, int64_t batch, const fnn_opts* opts,
                                             int32_t* orders_out, fnn_event* events_out, int32_t* nevents_out, fnn_batch_stats* stats) {
    return entry("emu_canonical_order_batch_device_f64", D, true, n, ld, stride, batch, opts, orders_out, events_out, nevents_out, stats);
}

}  // extern "C"

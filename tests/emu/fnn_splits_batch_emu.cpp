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
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../fastneighbornet_amd/csrc/fnn_small_splits.h"

namespace {

using namespace fnn;

thread_local std::vector<int32_t> g_giveups;  // FNN_SW_GIVEUP_* per problem of the last call that reached the kernel

struct CpuSplitsExec {
    int nt;
    template <class F>
    void all(F f) {
        for (int t = 0; t < nt; t++) f(t, nt);
    }
    template <class F>
    void best(const SplitsView& V, F f) {
        for (int w = 0; w < (nt + 63) / 64; w++) {
            SplitsRec b{0.0, -1, -1};
            for (int t = w * 64; t < nt && t < (w + 1) * 64; t++) {
                const SplitsRec o = f(t, nt);
                if (splits_better(o, b)) b = o;
            }
            V.wred[w] = b;
        }
    }
    template <class P, class S>
    void rows(int32_t nrows, P share, S store) {
        for (int32_t row = 0; row < nrows; row++) {
            double p[64];
            for (int l = 0; l < 64; l++) p[l] = share(row, l);
            for (int off = 32; off > 0; off >>= 1)  // the tree of the kernel's shuffles, as lane 0 sees it
                for (int l = 0; l < off; l++) p[l] += p[l + off];
            store(row, p[0]);
        }
    }
    template <class T>
    T get(const T* p) { return *p; }
};

struct EmuSplitsBackend {
    std::vector<void*> bufs;
    std::string last;
    int64_t done = 0;  // problems of earlier chunks
    ~EmuSplitsBackend() { for (void* p : bufs) std::free(p); }
    const std::string& err() const { return last; }
    int32_t open(int32_t) { return FNN_OK; }
    void* alloc(size_t bytes) {
        void* p = std::malloc(bytes ? bytes : 1);
        if (p) { std::memset(p, 0xFF, bytes); bufs.push_back(p); }
        return p;
    }
    int32_t h2d(void* dst, const void* src, size_t bytes) { std::memcpy(dst, src, bytes); return FNN_OK; }
    int32_t d2h(void* dst, const void* src, size_t bytes) { std::memcpy(dst, src, bytes); return FNN_OK; }
    int32_t run_splits(const double* D, int32_t n, int64_t ld, int64_t stride, const int32_t* ord, int64_t cnt, int32_t cap, int32_t threads,
                       int32_t lds_bytes, double* work, int64_t pitch, double* out, SplitsMeta* meta, double* t_kernel_s) {
        const double t0 = now_s();
        const int64_t N = (int64_t)n * (n - 1) / 2;
        for (int64_t b = 0; b < cnt; b++) {
            unsigned char* lds = (unsigned char*)std::malloc((size_t)lds_bytes);
            double* slice = (double*)std::malloc(sizeof(double) * (size_t)pitch);  // this problem's slice, on its own
            double* w = (double*)std::malloc(sizeof(double) * (size_t)N);
            if (!lds || !slice || !w) { std::free(lds); std::free(slice); std::free(w); last = "out of memory"; return FNN_ENOMEM; }
            std::memset(lds, 0xFF, (size_t)lds_bytes);
            std::memset(slice, 0xFF, sizeof(double) * (size_t)pitch);
            std::memset(w, 0xFF, sizeof(double) * (size_t)N);
            const SplitsView V = small_splits_view(lds, slice, n, cap);
            CpuSplitsExec ex{threads};
            small_splits_problem(ex, V, D + b * stride, ld, ord + b * (n + 1), w, meta + b);
            std::memcpy(out + b * N, w, sizeof(double) * (size_t)N);
            g_giveups[(size_t)(done + b)] = meta[b].giveup;
            std::free(w);
            std::free(slice);
            std::free(lds);
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

}  // extern "C"

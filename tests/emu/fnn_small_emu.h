// fnn_small_emu.h -- TEST INFRASTRUCTURE: what the CPU drivers of the batch calls share (fnn_batch_emu.cpp,
// fnn_batch_global_emu.cpp, fnn_splits_batch_emu.cpp, fnn_ragged_emu.cpp).
//
// "Device memory" is the heap, and every block is filled with 0xFF bytes first: a word read before it is written is a NaN
// or -1 that the comparison with the oracle notices.  What one workgroup owns (its LDS image, its working copy or
// workspace slice, its weights) is an EmuBlock of exactly the size the kernel declares: under AddressSanitizer an index
// past the layout is an error.  The executors run a phase for tid = 0 ... nt - 1; a barrier of the kernel is the end of
// such a loop.
#ifndef FNN_SMALL_EMU_H
#define FNN_SMALL_EMU_H

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../fastneighbornet_amd/csrc/fnn_small_splits.h"

namespace fnn {

// open / alloc / h2d / d2h / err of a backend (small_batch<B> and the others)
struct EmuHeapBackend {
    std::vector<void*> bufs;
    std::string last;
    ~EmuHeapBackend() { for (void* p : bufs) std::free(p); }
    const std::string& err() const { return last; }
    int32_t open(int32_t) { return FNN_OK; }
    void* alloc(size_t bytes) {
        void* p = std::malloc(bytes ? bytes : 1);
        if (p) { std::memset(p, 0xFF, bytes); bufs.push_back(p); }
        return p;
    }
    int32_t h2d(void* dst, const void* src, size_t bytes) { std::memcpy(dst, src, bytes); return FNN_OK; }
    int32_t d2h(void* dst, const void* src, size_t bytes) { std::memcpy(dst, src, bytes); return FNN_OK; }
};

// a heap block of exactly `bytes` bytes, 0xFF-filled, freed on scope exit; p == nullptr: out of memory
struct EmuBlock {
    void* p;
    explicit EmuBlock(size_t bytes) : p(std::malloc(bytes)) { if (p) std::memset(p, 0xFF, bytes); }
    ~EmuBlock() { std::free(p); }
    EmuBlock(const EmuBlock&) = delete;
    EmuBlock& operator=(const EmuBlock&) = delete;
    unsigned char* bytes() const { return (unsigned char*)p; }
    double* doubles() const { return (double*)p; }
};

struct CpuExec {
    int nt;
    template <class F>
    void all(F f) {
        for (int t = 0; t < nt; t++) f(t, nt);
    }
    void scan(const SmallView& V, int32_t m, int32_t c) {
        for (int w = 0; w < (nt + 63) / 64; w++) {
            SmallCand b{0.0, -1, -1};
            for (int t = w * 64; t < nt && t < (w + 1) * 64; t++) {
                const SmallCand o = small_scan_thread(t, nt, V, m, c);
                if (small_before(o, b)) b = o;
            }
            V.wred[w] = b;
        }
    }
};

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

// One split-weight problem as one workgroup runs it: LDS image, workspace slice and weights are blocks of their own, and
// the weights are copied to `out` afterwards.  false: out of memory.
inline bool emu_splits_problem(int32_t threads, int32_t lds_bytes, int64_t pitch, int32_t n, int32_t cap, const SplitsSwitches& sw, const double* D,
                               int64_t ld, const int32_t* ord, double* out, SplitsMeta* meta) {
    const int64_t N = (int64_t)n * (n - 1) / 2;
    EmuBlock lds((size_t)lds_bytes), slice(sizeof(double) * (size_t)pitch), w(sizeof(double) * (size_t)N);
    if (!lds.p || !slice.p || !w.p) return false;
    const SplitsView V = small_splits_view(lds.bytes(), slice.doubles(), n, cap);
    CpuSplitsExec ex{threads};
    small_splits_problem(ex, V, sw, D, ld, ord, w.doubles(), meta);
    std::memcpy(out, w.p, sizeof(double) * (size_t)N);
    return true;
}

}  // namespace fnn
#endif

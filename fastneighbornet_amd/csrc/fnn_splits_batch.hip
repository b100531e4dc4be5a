// fnn_splits_batch.hip -- circular split weights of many small problems in one call: k_small_splits solves one whole
// non-negative least-squares problem per workgroup (the phase bodies, their sequence and the host side of the call are
// fnn_small_splits.h); k_small_splits_ragged is the same for problems of different sizes, one
// descriptor per workgroup.
//
// The kernel is a thin wrapper: it carves the dynamic LDS and the problem's workspace slice into the view and hands the
// phases to small_splits_problem() with an executor whose barrier is __syncthreads().  No cross-workgroup communication,
// no floating-point atomics, vector stores and plain C++ only.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "fnn_ragged_hip.h"
#include "fnn_small_splits.h"

namespace fnn {

// Waves of the workgroup hand grid entries and rows of the factor to each other through GLOBAL memory: a phase's stores
// must have left the storing wave before the barrier lets another wave load them.  The compiler lowers __syncthreads()'s
// workgroup-scope release to s_waitcnt lgkmcnt(0) alone, so the wait for the vector stores is written out, as in
// GpuGlobalExec (fnn_batch.hip; DESIGN.md section 11 "Memory ordering").
struct GpuSplitsExec {
    __device__ __forceinline__ void barrier() {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    template <class F>
    __device__ __forceinline__ void all(F f) {
        f((int)threadIdx.x, (int)blockDim.x);
        barrier();
    }
    template <class F>
    __device__ __forceinline__ void best(const SplitsView& V, F f) {
        SplitsRec b = f((int)threadIdx.x, (int)blockDim.x);
        for (int off = 32; off > 0; off >>= 1) {
            SplitsRec o;
            o.v = __shfl_down(b.v, off);
            o.k = __shfl_down(b.k, off);
            o.e = __shfl_down(b.e, off);
            if (splits_better(o, b)) b = o;
        }
        if ((threadIdx.x & 63) == 0) V.wred[threadIdx.x >> 6] = b;
        barrier();
    }
    template <class P, class S>
    __device__ __forceinline__ void rows(int32_t nrows, P share, S store) {
        const int32_t lane = threadIdx.x & 63;
        for (int32_t row = threadIdx.x >> 6; row < nrows; row += blockDim.x >> 6) {
            double p = share(row, lane);
            for (int off = 32; off > 0; off >>= 1) p += __shfl_down(p, off);
            if (lane == 0) store(row, p);
        }
        barrier();
    }
    template <class T>
    __device__ __forceinline__ T get(const T* p) {
        const T v = *static_cast<const volatile T*>(p);
        __syncthreads();
        return v;
    }
};

// grid: one workgroup per problem of the chunk; dynamic LDS: small_splits_layout(n, cap).bytes.  `work` (neither const nor
// __restrict__: the workgroup stores to it and loads what it stored) holds the problems' slices, `pitch` doubles apart.
__global__ __launch_bounds__(1024) void k_small_splits(const double* __restrict__ D, int32_t n, int64_t ld, int64_t stride,
                                                       const int32_t* __restrict__ ord, int32_t cap, SplitsSwitches sw, double* work, int64_t pitch,
                                                       double* __restrict__ out, SplitsMeta* __restrict__ meta) {
    extern __shared__ __attribute__((aligned(16))) unsigned char splits_lds[];
    const int64_t b = blockIdx.x;
    const SplitsView V = small_splits_view(splits_lds, work + b * pitch, n, cap);
    GpuSplitsExec ex;
    small_splits_problem(ex, V, sw, D + b * stride, ld, ord + b * (n + 1), out + b * ((int64_t)n * (n - 1) / 2), meta + b);
}

// Ragged batches: one workgroup per DESCRIPTOR.  grid: the problems of one size class, desc already
// advanced to the class's first descriptor; dynamic LDS: small_splits_layout of the class's largest member, of which the
// problem uses its own small_splits_layout(n, cap).bytes.  The descriptor is the same for every thread of the workgroup.
__global__ __launch_bounds__(1024) void k_small_splits_ragged(const double* __restrict__ D, const RaggedDesc* __restrict__ desc,
                                                              const int32_t* __restrict__ ord, SplitsSwitches sw, double* work,
                                                              double* __restrict__ out, SplitsMeta* __restrict__ meta) {
    extern __shared__ __attribute__((aligned(16))) unsigned char splits_lds[];
    const RaggedDesc d = desc[blockIdx.x];
    const SplitsView V = small_splits_view(splits_lds, work + d.work, d.n, d.cap);
    GpuSplitsExec ex;
    small_splits_problem(ex, V, sw, D + d.src, d.ld, ord + d.ord, out + d.out, meta + d.meta);
}

struct SplitsHipBackend : HipBatchBase {
    RaggedLauncher ragged{RAGGED_SPLITS_STREAMS};

    int32_t run_splits(const double* dD, int32_t n, int64_t ld, int64_t stride, const int32_t* d_ord, int64_t cnt, int32_t cap, int32_t threads,
                       int32_t lds_bytes, double* d_work, int64_t pitch, double* d_out, SplitsMeta* d_meta, double* t_kernel_s) {
        const SplitsSwitches sw = small_splits_switches();
        return timed_launch(reinterpret_cast<const void*>(&k_small_splits), "k_small_splits", lds_bytes, [&] {
            hipLaunchKernelGGL(k_small_splits, dim3((unsigned)cnt), dim3((unsigned)threads), (size_t)lds_bytes, stream, dD, n, ld, stride, d_ord, cap, sw,
                               d_work, pitch, d_out, d_meta);
        }, t_kernel_s);
    }
    int32_t run_splits_ragged(const double* base, const RaggedDesc* d_desc, const RaggedClass* cls, int32_t ncls, const int32_t* d_ord, double* d_work,
                              double* d_out, SplitsMeta* d_meta, double* t_kernel_s) {
        int32_t lds_max = 0;
        for (int32_t c = 0; c < ncls; c++) lds_max = cls[c].lds_bytes > lds_max ? cls[c].lds_bytes : lds_max;
        if (!ok(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_small_splits_ragged), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max),
                "hipFuncSetAttribute"))
            return FNN_EHIP;
        const SplitsSwitches sw = small_splits_switches();
        const char* what = "";
        const hipError_t e = ragged.run(stream, e0, e1, ncls, [&](int32_t c, hipStream_t s) {
            hipLaunchKernelGGL(k_small_splits_ragged, dim3((unsigned)cls[c].count), dim3((unsigned)cls[c].threads), (size_t)cls[c].lds_bytes, s, base,
                               d_desc + cls[c].first, d_ord, sw, d_work, d_out, d_meta);
        }, t_kernel_s, &what);
        return ok(e, (std::string("k_small_splits_ragged: ") + what).c_str()) ? FNN_OK : FNN_EHIP;
    }
    int32_t single(const double* D, int32_t n, const int32_t* ordering, int32_t device, double* weights, fnn_sw_stats* sw) {
        return fnn_split_weights_f64(D, n, n, ordering, device, weights, sw);
    }
};

}  // namespace fnn

extern "C" {

int32_t fnn_split_weights_batch_max_n(void) { return fnn::SPLITS_MAX_N; }
int64_t fnn_split_weights_batch_min_batch(int32_t n) { return fnn::small_splits_min_batch(n); }

int32_t fnn_split_weights_batch_f64(const double* D, int32_t n, int64_t ld, int64_t stride, int64_t batch, const int32_t* orderings, int32_t device,
                                    double* weights_out, fnn_sw_stats* stats_out, fnn_sw_batch_stats* stats) {
    FNN_BATCH_TRY(
        fnn::SplitsHipBackend be;
        return fnn::small_splits_batch(be, "fnn_split_weights_batch_f64", D, false, n, ld, stride, batch, orderings, device, weights_out, stats_out, stats);
    )
}

int32_t fnn_split_weights_batch_device_f64(const double* d_D, int32_t n, int64_t ld, int64_t stride, int64_t batch, const int32_t* orderings,
                                           int32_t device, double* weights_out, fnn_sw_stats* stats_out, fnn_sw_batch_stats* stats) {
    FNN_BATCH_TRY(
        fnn::SplitsHipBackend be;
        return fnn::small_splits_batch(be, "fnn_split_weights_batch_device_f64", d_D, true, n, ld, stride, batch, orderings, device, weights_out, stats_out, stats);
    )
}

int32_t fnn_split_weights_ragged_f64(const double* D, const int64_t* offsets, const int32_t* n, const int64_t* ld, int64_t batch, const int32_t* orderings,
                                     int32_t device, double* weights_out, fnn_sw_stats* stats_out, fnn_sw_batch_stats* stats) {
    FNN_BATCH_TRY(
        fnn::SplitsHipBackend be;
        return fnn::small_splits_ragged(be, "fnn_split_weights_ragged_f64", D, false, offsets, n, ld, batch, orderings, device, weights_out, stats_out, stats);
    )
}

int32_t fnn_split_weights_ragged_device_f64(const double* d_D, const int64_t* offsets, const int32_t* n, const int64_t* ld, int64_t batch,
                                            const int32_t* orderings, int32_t device, double* weights_out, fnn_sw_stats* stats_out,
                                            fnn_sw_batch_stats* stats) {
    FNN_BATCH_TRY(
        fnn::SplitsHipBackend be;
        return fnn::small_splits_ragged(be, "fnn_split_weights_ragged_device_f64", d_D, true, offsets, n, ld, batch, orderings, device, weights_out, stats_out, stats);
    )
}

}  // extern "C"

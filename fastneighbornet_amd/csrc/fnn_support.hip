// fnn_support.hip -- split support on the device: the kernels of the sequence in fnn_support.h and
// the HIP backend of fnn_split_support[_device]_f64.  Every kernel is a loop frame around the per-thread steps of
// fnn_support.h; integer atomics (compare-and-swap, min, add) and plain C++ only - no float atomics, no spin, no inline
// assembly.  256 threads per workgroup everywhere.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "fnn_support.h"
#include "fnn_ragged_hip.h"

namespace fnn {

// one workgroup per problem of the chunk
__global__ __launch_bounds__(SUP_THREADS) void k_sup_count(const SupArgs a) {
    sup_count_thread(a, (int64_t)blockIdx.x, (int)threadIdx.x, SUP_THREADS);
}

// one workgroup per problem: ordering and prefix sets in LDS, then the indices k in tiles of 256, in order
__global__ __launch_bounds__(SUP_THREADS) void k_sup_emit(const SupArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sup_lds[];
    const SupLds L = sup_lds_view(sup_lds, a.n, a.words);
    const int t = (int)threadIdx.x;
    const int64_t bl = (int64_t)blockIdx.x;
    sup_emit_load(a, L, bl, t, SUP_THREADS);
    __syncthreads();
    sup_emit_prefix(a, L, t);
    __syncthreads();
    uint32_t base = a.recbase[bl];
    for (int64_t k0 = 0; k0 < a.K; k0 += SUP_THREADS) {
        const int64_t k = k0 + t;
        const bool f = k < a.K && sup_counts(a, bl, k);
        const uint64_t m = __ballot(f);
        if ((t & 63) == 0) L.wmask[t >> 6] = m;
        __syncthreads();
        uint32_t total;
        const uint32_t place = sup_emit_place(L.wmask, t, &total);
        if (f) sup_emit_record(a, L.P, bl, k, base + place);
        base += total;
        __syncthreads();  // (the next tile's ballots overwrite wmask)
    }
}

__global__ __launch_bounds__(SUP_THREADS) void k_sup_verify(const SupArgs a) { sup_verify_thread(a, blockIdx.x * SUP_THREADS + threadIdx.x); }
__global__ __launch_bounds__(SUP_THREADS) void k_sup_rows(const SupArgs a) { sup_rows_thread(a, blockIdx.x * SUP_THREADS + threadIdx.x); }
__global__ __launch_bounds__(SUP_THREADS) void k_sup_scatter(const SupArgs a) { sup_scatter_thread(a, blockIdx.x * SUP_THREADS + threadIdx.x); }
__global__ __launch_bounds__(SUP_THREADS) void k_sup_rank(const SupArgs a) { sup_rank_thread(a, blockIdx.x * SUP_THREADS + threadIdx.x); }
__global__ __launch_bounds__(SUP_THREADS) void k_sup_sum(const SupArgs a) { sup_sum_thread(a, blockIdx.x * SUP_THREADS + threadIdx.x); }

// one workgroup per tile of SUP_SCAN_TILE words
__global__ __launch_bounds__(SUP_THREADS) void k_sup_scan_sums(const SupArgs a) {
    sup_scan_sums_thread(a, (int64_t)blockIdx.x, (int)threadIdx.x);
}
__global__ __launch_bounds__(SUP_THREADS) void k_sup_scan_apply(const SupArgs a) {
    __shared__ uint32_t part[SUP_THREADS];
    const int t = (int)threadIdx.x;
    part[t] = sup_scan_own(a, (int64_t)blockIdx.x, t);
    __syncthreads();
    sup_scan_apply_thread(a, (int64_t)blockIdx.x, t, part);
}

struct SupHipBackend : HipBatchBase {
    void release(void* p) {
        bufs.erase(std::remove(bufs.begin(), bufs.end(), p), bufs.end());
        (void)hipFree(p);
    }
    int32_t fill(void* p, int byte, size_t bytes) {
        if (!bytes) return FNN_OK;
        return ok(hipMemsetAsync(p, byte, bytes, stream), "hipMemset") && ok(hipStreamSynchronize(stream), "fill") ? FNN_OK : FNN_EHIP;
    }
    template <class K>
    int32_t launch(K kernel, const char* name, int64_t blocks, int32_t lds_bytes, const SupArgs& a, double* t_kernel_s) {
        if (blocks <= 0) { *t_kernel_s = 0.0; return FNN_OK; }
        if (blocks >= ((int64_t)1 << 31)) { last = "too many workgroups for one launch"; return FNN_EHIP; }
        return timed_launch(reinterpret_cast<const void*>(kernel), name, lds_bytes, [&] {
            hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(SUP_THREADS), (size_t)lds_bytes, stream, a);
        }, t_kernel_s);
    }
    int32_t run(int kernel, const SupArgs& a, int64_t items, double* t_kernel_s) {
        const int64_t flat = (items + SUP_THREADS - 1) / SUP_THREADS;
        switch (kernel) {
            case SUP_K_COUNT: return launch(&k_sup_count, "k_sup_count", items, 0, a, t_kernel_s);
            case SUP_K_EMIT: return launch(&k_sup_emit, "k_sup_emit", items, sup_lds_bytes(a.n, a.words), a, t_kernel_s);
            case SUP_K_VERIFY: return launch(&k_sup_verify, "k_sup_verify", flat, 0, a, t_kernel_s);
            case SUP_K_SCAN_SUMS: return launch(&k_sup_scan_sums, "k_sup_scan_sums", items, 0, a, t_kernel_s);
            case SUP_K_SCAN_APPLY: return launch(&k_sup_scan_apply, "k_sup_scan_apply", items, 0, a, t_kernel_s);
            case SUP_K_ROWS: return launch(&k_sup_rows, "k_sup_rows", flat, 0, a, t_kernel_s);
            case SUP_K_SCATTER: return launch(&k_sup_scatter, "k_sup_scatter", flat, 0, a, t_kernel_s);
            case SUP_K_RANK: return launch(&k_sup_rank, "k_sup_rank", flat, 0, a, t_kernel_s);
            case SUP_K_SUM: return launch(&k_sup_sum, "k_sup_sum", flat, 0, a, t_kernel_s);
        }
        last = "no such kernel";
        return FNN_EHIP;
    }
};

}  // namespace fnn

extern "C" {

int32_t fnn_split_support_max_n(void) { return fnn::SUP_MAX_N; }
int64_t fnn_split_support_min_work(void) { return fnn::SUP_MIN_WORK; }

int32_t fnn_split_support_f64(int32_t n, int64_t batch, const int32_t* orderings, const double* weights, double threshold, int64_t lead, int32_t device,
                              uint64_t* keys_out, int64_t* first_b_out, int64_t* first_k_out, int64_t* counts_out, double* weight_sum_out,
                              int64_t capacity, int64_t* count_out, fnn_support_stats* stats) {
    FNN_BATCH_TRY(
        fnn::SupHipBackend be;
        return fnn::support_call(be, "fnn_split_support_f64", n, batch, orderings, weights, false, threshold, lead, device, keys_out, first_b_out,
                                 first_k_out, counts_out, weight_sum_out, capacity, count_out, stats);
    )
}

int32_t fnn_split_support_device_f64(int32_t n, int64_t batch, const int32_t* orderings, const double* d_weights, double threshold, int64_t lead,
                                     int32_t device, uint64_t* keys_out, int64_t* first_b_out, int64_t* first_k_out, int64_t* counts_out,
                                     double* weight_sum_out, int64_t capacity, int64_t* count_out, fnn_support_stats* stats) {
    FNN_BATCH_TRY(
        fnn::SupHipBackend be;
        return fnn::support_call(be, "fnn_split_support_device_f64", n, batch, orderings, d_weights, true, threshold, lead, device, keys_out,
                                 first_b_out, first_k_out, counts_out, weight_sum_out, capacity, count_out, stats);
    )
}

int32_t fnn_split_keys(int32_t n, const int32_t* ordering, const int64_t* k, int64_t count, uint64_t* keys_out) {
    FNN_BATCH_TRY(return fnn::sup_split_keys("fnn_split_keys", n, ordering, k, count, keys_out);)
}

}  // extern "C"

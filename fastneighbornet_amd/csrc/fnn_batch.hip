// fnn_batch.hip -- many small problems in one call: k_small runs one whole Canonical Neighbor-Net problem per workgroup
// out of LDS (the phase bodies and the host side of the call are fnn_small.h); k_small_global does
// the same above the LDS limit with the matrix in a working copy in global memory (fnn_small_global.h); k_small_ragged is
// k_small for problems of different sizes, one descriptor per workgroup.
//
// Each kernel is a thin wrapper: it carves the dynamic LDS into the view, loads the matrix and hands the phases to
// small_problem() / global_problem() with an executor whose barrier is __syncthreads().  No cross-workgroup communication,
// no atomics on the event path, vector stores and plain C++ only.
#include <hip/hip_runtime.h>

#include <climits>
#include <string>
#include <vector>

#include "fnn_ragged_hip.h"
#include "fnn_small_global.h"

namespace fnn {

struct GpuExec {
    template <class F>
    __device__ __forceinline__ void all(F f) {
        f((int)threadIdx.x, (int)blockDim.x);
        __syncthreads();
    }
    // the scan's minimum under the total order (Q, i, j): DPP-free wave reduction by shuffles, one record per wave in LDS
    __device__ __forceinline__ void scan(const SmallView& V, int32_t m, int32_t c) {
        SmallCand b = small_scan_thread((int)threadIdx.x, (int)blockDim.x, V, m, c);
        for (int off = 32; off > 0; off >>= 1) {
            SmallCand o;
            o.q = __shfl_down(b.q, off);
            o.i = __shfl_down(b.i, off);
            o.j = __shfl_down(b.j, off);
            if (small_before(o, b)) b = o;
        }
        if ((threadIdx.x & 63) == 0) V.wred[threadIdx.x >> 6] = b;
        __syncthreads();
    }
};

// grid: one workgroup per problem of the chunk; dynamic LDS: small_layout(n).bytes
__global__ __launch_bounds__(1024) void k_small(const double* __restrict__ D, int32_t n, int64_t ld, int64_t stride, int32_t vec,
                                                int32_t* __restrict__ meta, Agg3Rec* __restrict__ log, Event* __restrict__ ev) {
    extern __shared__ __attribute__((aligned(16))) unsigned char small_lds[];
    const SmallView V = small_view(small_lds, n);
    const int64_t b = blockIdx.x;
    small_load((int)threadIdx.x, (int)blockDim.x, V, D + b * stride, ld, vec);  // (the first phase's barrier covers the load)
    GpuExec ex;
    small_problem(ex, V, ev ? ev + b * n : nullptr, meta + b * SMALL_META_INTS, log + b * n);
}

// Ragged batches: one workgroup per DESCRIPTOR.  grid: the problems of one size class, desc already
// advanced to the class's first descriptor; dynamic LDS: small_layout(the class's largest n).bytes, of which the problem
// uses small_layout(its own n).bytes.  The descriptor is the same for every thread of the workgroup.
__global__ __launch_bounds__(1024) void k_small_ragged(const double* __restrict__ D, const RaggedDesc* __restrict__ desc,
                                                       int32_t* __restrict__ meta, Agg3Rec* __restrict__ log, Event* __restrict__ ev) {
    extern __shared__ __attribute__((aligned(16))) unsigned char small_lds[];
    const RaggedDesc d = desc[blockIdx.x];
    const SmallView V = small_view(small_lds, d.n);
    small_load((int)threadIdx.x, (int)blockDim.x, V, D + d.src, d.ld, d.vec);  // (the first phase's barrier covers the load)
    GpuExec ex;
    small_problem(ex, V, ev ? ev + d.ev : nullptr, meta + d.meta, log + d.log);
}

// the lowest caller's index of a problem whose matrix fails the check, through atomicMin on one word
__global__ __launch_bounds__(256) void k_small_validate_ragged(const double* __restrict__ D, const RaggedDesc* __restrict__ desc,
                                                               unsigned long long* first_bad) {
    const RaggedDesc d = desc[blockIdx.x];
    if (small_validate_thread((int)threadIdx.x, (int)blockDim.x, D + d.src, d.n, d.ld)) atomicMin(first_bad, (unsigned long long)d.id);
}

// Waves of the workgroup hand matrix entries to each other through GLOBAL memory: a phase's stores must have left the
// storing wave before the barrier lets another wave load them.  __syncthreads() is a workgroup-scope release, the barrier
// and a workgroup-scope acquire; for a workgroup on one CU the compiler lowers that release to s_waitcnt lgkmcnt(0) alone
// (the CU's memory pipeline keeps its waves' accesses in order), so the wait for the vector stores is written out: every
// wave drains its own stores, then joins the barrier.  It costs nothing in a phase that stored nothing to global memory.
// (DESIGN.md section 11 records what the kept ISA shows in front of each s_barrier.)
struct GpuGlobalExec {
    template <class F>
    __device__ __forceinline__ void all(F f) {
        f((int)threadIdx.x, (int)blockDim.x);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    __device__ __forceinline__ void scan_global(const GlobalView& V, int32_t m, int32_t c) {
        SmallCand b = global_scan_thread((int)threadIdx.x, (int)blockDim.x, V, m, c);
        for (int off = 32; off > 0; off >>= 1) {
            SmallCand o;
            o.q = __shfl_down(b.q, off);
            o.i = __shfl_down(b.i, off);
            o.j = __shfl_down(b.j, off);
            if (small_before(o, b)) b = o;
        }
        if ((threadIdx.x & 63) == 0) V.wred[threadIdx.x >> 6] = b;
        __syncthreads();
    }
};

// grid: one workgroup per problem of the chunk; dynamic LDS: small_global_layout(n).bytes.  `work` (neither const nor
// __restrict__: the workgroup stores to it and loads what it stored) holds the working copies, small_global_pitch(n)
// doubles apart; src == work: the matrices are there already (host entry), otherwise each is copied in first.
__global__ __launch_bounds__(1024) void k_small_global(const double* src, int32_t n, int64_t ld, int64_t stride, double* work,
                                                       int32_t* __restrict__ meta, Agg3Rec* __restrict__ log, Event* __restrict__ ev) {
    extern __shared__ __attribute__((aligned(16))) unsigned char small_lds[];
    const int64_t b = blockIdx.x;
    const GlobalView V = small_global_view(small_lds, work + b * small_global_pitch(n), n);
    if (src != work) global_copy((int)threadIdx.x, (int)blockDim.x, V, src + b * stride, ld);  // (the first phase's barrier covers the copy)
    GpuGlobalExec ex;
    global_problem(ex, V, ev ? ev + b * n : nullptr, meta + b * SMALL_META_INTS, log + b * n);
}

// the lowest index of a problem whose matrix fails the check, through atomicMin on one word
__global__ __launch_bounds__(256) void k_small_validate(const double* __restrict__ D, int32_t n, int64_t ld, int64_t stride, int32_t* first_bad) {
    const int64_t b = blockIdx.x;
    if (small_validate_thread((int)threadIdx.x, (int)blockDim.x, D + b * stride, n, ld)) atomicMin(first_bad, (int32_t)blockIdx.x);
}

struct SmallHipBackend : HipBatchBase {
    int32_t* d_bad = nullptr;
    unsigned long long* d_bad64 = nullptr;
    RaggedLauncher ragged{RAGGED_ORDER_STREAMS};

    int32_t validate(const double* dD, int32_t n, int64_t ld, int64_t stride, int64_t cnt, int64_t* bad) {
        if (!d_bad && !(d_bad = (int32_t*)alloc(sizeof(int32_t)))) return FNN_EHIP;
        int32_t h = INT_MAX;
        if (h2d(d_bad, &h, sizeof(h)) != FNN_OK) return FNN_EHIP;
        hipLaunchKernelGGL(k_small_validate, dim3((unsigned)cnt), dim3(256), 0, stream, dD, n, ld, stride, d_bad);
        if (!ok(hipGetLastError(), "k_small_validate")) return FNN_EHIP;
        if (d2h(&h, d_bad, sizeof(h)) != FNN_OK) return FNN_EHIP;
        *bad = h == INT_MAX ? -1 : h;
        return FNN_OK;
    }
    int32_t run(const double* dD, int32_t n, int64_t ld, int64_t stride, int64_t cnt, int32_t threads, int32_t lds_bytes,
                int32_t* d_meta, Agg3Rec* d_log, Event* d_ev, double* t_kernel_s) {
        const int32_t vec = (ld == n && stride % 2 == 0 && reinterpret_cast<uintptr_t>(dD) % 16 == 0) ? 1 : 0;
        return timed_launch(reinterpret_cast<const void*>(&k_small), "k_small", lds_bytes, [&] {
            hipLaunchKernelGGL(k_small, dim3((unsigned)cnt), dim3((unsigned)threads), (size_t)lds_bytes, stream, dD, n, ld, stride, vec, d_meta, d_log, d_ev);
        }, t_kernel_s);
    }
    int32_t run_global(const double* src, int64_t ld, int64_t stride, double* work, int64_t cnt, int32_t n, int32_t threads, int32_t lds_bytes,
                       int32_t* d_meta, Agg3Rec* d_log, Event* d_ev, double* t_kernel_s) {
        return timed_launch(reinterpret_cast<const void*>(&k_small_global), "k_small_global", lds_bytes, [&] {
            hipLaunchKernelGGL(k_small_global, dim3((unsigned)cnt), dim3((unsigned)threads), (size_t)lds_bytes, stream, src, n, ld, stride, work, d_meta, d_log, d_ev);
        }, t_kernel_s);
    }
    // ---- ragged batches (small_ragged<B>, fnn_small.h)
    int32_t validate_ragged(const double* base, const RaggedDesc* d_desc, int64_t cnt, int64_t* bad) {
        if (!d_bad64 && !(d_bad64 = (unsigned long long*)alloc(sizeof(unsigned long long)))) return FNN_EHIP;
        unsigned long long h = ~0ull;
        if (h2d(d_bad64, &h, sizeof(h)) != FNN_OK) return FNN_EHIP;
        hipLaunchKernelGGL(k_small_validate_ragged, dim3((unsigned)cnt), dim3(256), 0, stream, base, d_desc, d_bad64);
        if (!ok(hipGetLastError(), "k_small_validate_ragged")) return FNN_EHIP;
        if (d2h(&h, d_bad64, sizeof(h)) != FNN_OK) return FNN_EHIP;
        *bad = h == ~0ull ? -1 : (int64_t)h;
        return FNN_OK;
    }
    int32_t run_ragged(const double* base, const RaggedDesc* d_desc, const RaggedClass* cls, int32_t ncls, int32_t* d_meta, Agg3Rec* d_log,
                       Event* d_ev, double* t_kernel_s) {
        int32_t lds_max = 0;
        for (int32_t c = 0; c < ncls; c++) lds_max = cls[c].lds_bytes > lds_max ? cls[c].lds_bytes : lds_max;
        // more than 64 KiB of dynamic LDS has to be asked for
        if (!ok(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_small_ragged), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max),
                "hipFuncSetAttribute"))
            return FNN_EHIP;
        const char* what = "";
        const hipError_t e = ragged.run(stream, e0, e1, ncls, [&](int32_t c, hipStream_t s) {
            hipLaunchKernelGGL(k_small_ragged, dim3((unsigned)cls[c].count), dim3((unsigned)cls[c].threads), (size_t)cls[c].lds_bytes, s, base,
                               d_desc + cls[c].first, d_meta, d_log, d_ev);
        }, t_kernel_s, &what);
        return ok(e, (std::string("k_small_ragged: ") + what).c_str()) ? FNN_OK : FNN_EHIP;
    }
    // cnt problems of ONE size n above the LDS limit, anywhere in host or device memory: gathered into a dense device
    // array of the call's own, checked there, and handed to the same-size device entry 2 GiB at a time
    int32_t large(const std::string& W, const double* D, bool on_device, int32_t n, const int64_t* offs, const int64_t* lds, int64_t cnt,
                  const fnn_opts& opts, bool run, int32_t* orders, fnn_event* events, int32_t* nev, fnn_batch_stats* gs, int64_t* bad) {
        *bad = -1;
        if (!run && !opts.validate) return FNN_OK;
        const int64_t nn = (int64_t)n * n;
        int64_t part = SMALL_CHUNK_BYTES / (8 * nn);
        if (part < 1) part = 1;
        if (part > cnt) part = cnt;
        double* buf = nullptr;
        if (!ok(hipMalloc(&buf, sizeof(double) * (size_t)nn * (size_t)part), "hipMalloc")) return fail(FNN_ENOMEM, W + "device allocation failed");
        int32_t rc = FNN_OK;
        fnn_opts o2 = opts;
        o2.validate = 0;
        for (int64_t k0 = 0; k0 < cnt && rc == FNN_OK && *bad < 0; k0 += part) {
            const int64_t c = cnt - k0 < part ? cnt - k0 : part;
            const double tu = now_s();
            bool up = true;
            for (int64_t k = 0; k < c && up; k++)
                up = ok(hipMemcpy2DAsync(buf + k * nn, sizeof(double) * (size_t)n, D + offs[k0 + k], sizeof(double) * (size_t)lds[k0 + k],
                                         sizeof(double) * (size_t)n, (size_t)n, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream),
                        "hipMemcpy2D");
            if (!up || !ok(hipStreamSynchronize(stream), "gather")) { rc = fail(FNN_EHIP, W + "upload failed (" + last + ")"); break; }
            gs->t_upload_s += now_s() - tu;
            if (opts.validate) {
                int64_t b = -1;
                if (validate(buf, n, n, nn, c, &b) != FNN_OK) { rc = fail(FNN_EHIP, W + "validate failed (" + last + ")"); break; }
                if (b >= 0) { *bad = k0 + b; break; }
            }
            if (!run) continue;
            fnn_batch_stats s{};
            rc = fnn_canonical_order_batch_device_f64(buf, n, n, nn, c, &o2, orders + k0 * (n + 1), events ? events + k0 * n : nullptr, nev + k0, &s);
            if (rc != FNN_OK) { g_last_error = W + "the " + std::to_string(n) + "-taxon problems: " + g_last_error; break; }
            gs->n_global += s.n_global; gs->n_fallback += s.n_fallback; gs->n_lds += s.n_lds; gs->n_events += s.n_events;
            gs->chunks += s.chunks; gs->t_upload_s += s.t_upload_s; gs->t_kernel_s += s.t_kernel_s;
        }
        (void)hipFree(buf);
        return rc;
    }
    // n above the LDS limit: the one-problem engine, one handle for the whole call
    int32_t fallback(const std::string& W, const double* D, bool on_device, int32_t n, int64_t ld, int64_t stride, int64_t batch,
                     const fnn_opts& opts, int32_t* orders, fnn_event* events, int32_t* nev, fnn_batch_stats& st) {
        fnn_opts o = opts;
        if (events) o.record_events = 1;
        fnn_handle* h = nullptr;
        int32_t rc = fnn_create(n, &o, &h);
        if (rc != FNN_OK) return rc;
        for (int64_t b = 0; b < batch && rc == FNN_OK; b++) {
            fnn_stats fs;
            rc = on_device ? fnn_set_matrix_device(h, D + b * stride, ld) : fnn_set_rows(h, 0, n, D + b * stride, ld);
            if (rc == FNN_OK) rc = fnn_run(h, orders + b * (n + 1), &fs);
            if (rc != FNN_OK) { g_last_error = W + "problem " + std::to_string(b) + ": " + g_last_error; break; }
            nev[b] = (int32_t)fs.n_events;
            st.n_events += fs.n_events;
            if (events) {
                std::memset(events + b * n, 0, sizeof(fnn_event) * (size_t)n);
                const int64_t got = fnn_get_events(h, events + b * n, n);
                if (got < 0 || got != fs.n_events) {
                    rc = got < 0 ? (int32_t)got : FNN_ESTATE;
                    g_last_error = W + "problem " + std::to_string(b) + ": the engine returned " + std::to_string(got) + " events for a run of " +
                                   std::to_string(fs.n_events);
                    break;
                }
            }
            st.n_fallback++;
        }
        const std::string keep = g_last_error;
        fnn_destroy(h);
        g_last_error = keep;
        return rc;
    }
};

}  // namespace fnn

extern "C" {

int32_t fnn_batch_lds_max_n(void) { return fnn::SMALL_LDS_MAX_N; }
int32_t fnn_batch_global_max_n(void) { return fnn::SMALL_GLOBAL_MAX_N; }
int64_t fnn_batch_global_min_batch(int32_t n) { return fnn::small_global_min_batch(n); }

int32_t fnn_canonical_order_batch_f64(const double* D, int32_t n, int64_t ld, int64_t stride, int64_t batch, const fnn_opts* opts,
                                      int32_t* orders_out, fnn_event* events_out, int32_t* nevents_out, fnn_batch_stats* stats) {
    FNN_BATCH_TRY(
        fnn::SmallHipBackend be;
        if (fnn::small_global_route(n, batch))
            return fnn::small_global_batch(be, "fnn_canonical_order_batch_f64", D, false, n, ld, stride, batch, opts, orders_out, events_out, nevents_out, stats);
        return fnn::small_batch(be, "fnn_canonical_order_batch_f64", D, false, n, ld, stride, batch, opts, orders_out, events_out, nevents_out, stats);
    )
}

int32_t fnn_canonical_order_batch_device_f64(const double* d_D, int32_t n, int64_t ld, int64_t stride, int64_t batch, const fnn_opts* opts,
                                             int32_t* orders_out, fnn_event* events_out, int32_t* nevents_out, fnn_batch_stats* stats) {
    FNN_BATCH_TRY(
        fnn::SmallHipBackend be;
        if (fnn::small_global_route(n, batch))
            return fnn::small_global_batch(be, "fnn_canonical_order_batch_device_f64", d_D, true, n, ld, stride, batch, opts, orders_out, events_out, nevents_out, stats);
        return fnn::small_batch(be, "fnn_canonical_order_batch_device_f64", d_D, true, n, ld, stride, batch, opts, orders_out, events_out, nevents_out, stats);
    )
}

int32_t fnn_canonical_order_ragged_f64(const double* D, const int64_t* offsets, const int32_t* n, const int64_t* ld, int64_t batch, const fnn_opts* opts,
                                       int32_t* orders_out, fnn_event* events_out, int32_t* nevents_out, fnn_batch_stats* stats) {
    FNN_BATCH_TRY(
        fnn::SmallHipBackend be;
        return fnn::small_ragged(be, "fnn_canonical_order_ragged_f64", D, false, offsets, n, ld, batch, opts, orders_out, events_out, nevents_out, stats);
    )
}

int32_t fnn_canonical_order_ragged_device_f64(const double* d_D, const int64_t* offsets, const int32_t* n, const int64_t* ld, int64_t batch,
                                              const fnn_opts* opts, int32_t* orders_out, fnn_event* events_out, int32_t* nevents_out,
                                              fnn_batch_stats* stats) {
    FNN_BATCH_TRY(
        fnn::SmallHipBackend be;
        return fnn::small_ragged(be, "fnn_canonical_order_ragged_device_f64", d_D, true, offsets, n, ld, batch, opts, orders_out, events_out, nevents_out, stats);
    )
}

}  // extern "C"

// fnn_ragged_hip.h -- what the two HIP backends of the batch calls (fnn_batch.hip, fnn_splits_batch.hip) share:
//   HipBatchBase    the call's device, stream, events and buffers, the transfers and the timed launch of one kernel;
//   RaggedLauncher  how the size classes of one ragged chunk reach the device;
//   FNN_BATCH_TRY   the exception barrier of the C entry points.
//
// RaggedLauncher: the classes are independent of each other, and the class of the largest problems holds one or two workgroups per CU for
// the longest time.  They are launched largest first, round-robin over the call's own stream and up to three side streams,
// so that the workgroups of the smaller classes can fill the CUs that the large ones leave idle instead of waiting behind
// them.  How many streams pay was measured per half: the split weights, whose classes run for tenths
// of a second, gain a quarter from a second stream and nothing from more; the orders, whose classes run for milliseconds,
// lose more to the creation of a stream than the overlap returns.  FNN_RAGGED_STREAMS=1..4 overrides either default.
#ifndef FNN_RAGGED_HIP_H
#define FNN_RAGGED_HIP_H

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>
#include <vector>

#include "fnn_engine.h"  // fnn::fail, the FNN_* codes

namespace fnn {

struct HipBatchBase {
    std::vector<void*> bufs;
    hipStream_t stream = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    std::string last;
    int prev_device = -1;  // the caller's current device, restored when the call ends

    ~HipBatchBase() {
        for (void* p : bufs) (void)hipFree(p);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (stream) (void)hipStreamDestroy(stream);
        if (prev_device >= 0) (void)hipSetDevice(prev_device);
    }
    const std::string& err() const { return last; }
    bool ok(hipError_t e, const char* what) {
        if (e == hipSuccess) return true;
        last = std::string(what) + ": " + hipGetErrorString(e);
        return false;
    }
    int32_t open(int32_t device) {
        int cnt = 0;
        if (!ok(hipGetDeviceCount(&cnt), "hipGetDeviceCount")) return FNN_EHIP;
        if (device < 0 || device >= cnt) { last = "no HIP device " + std::to_string(device) + " (there is no CPU fallback)"; return FNN_EHIP; }
        int cur = -1;
        // (remembered even when it is `device` already: the one-problem solver sets the device too, and restoring the
        // current device is harmless)
        if (hipGetDevice(&cur) == hipSuccess) prev_device = cur;
        if (!ok(hipSetDevice(device), "hipSetDevice") || !ok(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "hipStreamCreate") ||
            !ok(hipEventCreate(&e0), "hipEventCreate") || !ok(hipEventCreate(&e1), "hipEventCreate"))
            return FNN_EHIP;
        return FNN_OK;
    }
    void* alloc(size_t bytes) {
        void* p = nullptr;
        if (!ok(hipMalloc(&p, bytes ? bytes : 1), "hipMalloc")) return nullptr;
        bufs.push_back(p);
        return p;
    }
    int32_t h2d(void* dst, const void* src, size_t bytes) {
        return ok(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream), "hipMemcpy") && ok(hipStreamSynchronize(stream), "upload") ? FNN_OK : FNN_EHIP;
    }
    int32_t d2h(void* dst, const void* src, size_t bytes) {
        return ok(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream), "hipMemcpy") && ok(hipStreamSynchronize(stream), "download") ? FNN_OK : FNN_EHIP;
    }
    // One launch of `kernel` (`name` in the error text) with lds_bytes of dynamic LDS, waited for and timed: launch()
    // enqueues it on `stream`.  More than 64 KiB of dynamic LDS has to be asked for.
    template <class Launch>
    int32_t timed_launch(const void* kernel, const char* name, int32_t lds_bytes, Launch launch, double* t_kernel_s) {
        if (!ok(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes), "hipFuncSetAttribute")) return FNN_EHIP;
        if (!ok(hipEventRecord(e0, stream), "hipEventRecord")) return FNN_EHIP;
        launch();
        if (!ok(hipGetLastError(), (std::string(name) + " launch").c_str())) return FNN_EHIP;
        if (!ok(hipEventRecord(e1, stream), "hipEventRecord") || !ok(hipEventSynchronize(e1), name)) return FNN_EHIP;
        float ms = 0.f;
        if (!ok(hipEventElapsedTime(&ms, e0, e1), "hipEventElapsedTime")) return FNN_EHIP;
        *t_kernel_s = (double)ms * 1e-3;
        return FNN_OK;
    }
};

constexpr int RAGGED_ORDER_STREAMS = 1;
constexpr int RAGGED_SPLITS_STREAMS = 2;

struct RaggedLauncher {
    static constexpr int MAX_SIDE = 3;
    hipStream_t side[MAX_SIDE] = {nullptr, nullptr, nullptr};
    hipEvent_t done[MAX_SIDE] = {nullptr, nullptr, nullptr};
    int default_streams;
    explicit RaggedLauncher(int default_streams_) : default_streams(default_streams_) {}

    ~RaggedLauncher() {
        for (int i = 0; i < MAX_SIDE; i++) {
            if (done[i]) (void)hipEventDestroy(done[i]);
            if (side[i]) (void)hipStreamDestroy(side[i]);
        }
    }
    int streams() const {
        if (const char* e = std::getenv("FNN_RAGGED_STREAMS")) { const int v = std::atoi(e); if (v >= 1 && v <= MAX_SIDE + 1) return v; }
        return default_streams;
    }
    // launch(c, stream) enqueues class c.  Everything enqueued on `main` before the call is complete before any class
    // starts; when the call returns all classes are complete and *t_s is the time from the first start to the last end.
    // On failure *what names the step.
    template <class Launch>
    hipError_t run(hipStream_t main, hipEvent_t e0, hipEvent_t e1, int32_t ncls, Launch launch, double* t_s, const char** what) {
        hipError_t e;
        const int ns = ncls < streams() ? (ncls < 1 ? 1 : ncls) : streams();
        *what = "hipEventRecord";
        if ((e = hipEventRecord(e0, main)) != hipSuccess) return e;
        for (int i = 0; i + 1 < ns; i++) {
            *what = "hipStreamCreate";
            if (!side[i] && (e = hipStreamCreateWithFlags(&side[i], hipStreamNonBlocking)) != hipSuccess) return e;
            if (!done[i] && (e = hipEventCreateWithFlags(&done[i], hipEventDisableTiming)) != hipSuccess) return e;
            *what = "hipStreamWaitEvent";
            if ((e = hipStreamWaitEvent(side[i], e0, 0)) != hipSuccess) return e;
        }
        *what = "kernel launch";
        for (int32_t c = 0; c < ncls; c++) {
            launch(c, c % ns == 0 ? main : side[c % ns - 1]);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
        for (int i = 0; i + 1 < ns; i++) {
            *what = "hipEventRecord";
            if ((e = hipEventRecord(done[i], side[i])) != hipSuccess) return e;
            *what = "hipStreamWaitEvent";
            if ((e = hipStreamWaitEvent(main, done[i], 0)) != hipSuccess) return e;
        }
        *what = "hipEventRecord";
        if ((e = hipEventRecord(e1, main)) != hipSuccess) return e;
        *what = "kernel";
        if ((e = hipEventSynchronize(e1)) != hipSuccess) return e;
        float ms = 0.f;
        *what = "hipEventElapsedTime";
        if ((e = hipEventElapsedTime(&ms, e0, e1)) != hipSuccess) return e;
        *t_s = (double)ms * 1e-3;
        return hipSuccess;
    }
};

}  // namespace fnn

#define FNN_BATCH_TRY(body)                                                   \
    try {                                                                     \
        body                                                                  \
    } catch (const std::bad_alloc&) {                                         \
        return fnn::fail(FNN_ENOMEM, "out of host memory");                   \
    } catch (const std::exception& e) {                                       \
        return fnn::fail(FNN_ESTATE, std::string("exception: ") + e.what()); \
    }

#endif

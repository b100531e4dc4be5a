// fnn_ragged_hip.h -- how the size classes of one ragged chunk reach the device, shared by the two
// HIP backends (fnn_batch.hip, fnn_splits_batch.hip).
//
// The classes are independent of each other, and the class of the largest problems holds one or two workgroups per CU for
// the longest time.  They are launched largest first, round-robin over the call's own stream and up to three side streams,
// so that the workgroups of the smaller classes can fill the CUs that the large ones leave idle instead of waiting behind
// them.  How many streams pay was measured per half: the split weights, whose classes run for tenths
// of a second, gain a quarter from a second stream and nothing from more; the orders, whose classes run for milliseconds,
// lose more to the creation of a stream than the overlap returns.  FNN_RAGGED_STREAMS=1..4 overrides either default.
#ifndef FNN_RAGGED_HIP_H
#define FNN_RAGGED_HIP_H

#include <hip/hip_runtime.h>

#include <cstdlib>

namespace fnn {

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
#endif

// fnn_draw_emu.cpp -- TEST INFRASTRUCTURE: CPU driver of the bootstrap entries that draw their replicates on the device
// (DESIGN.md section 17).
//
// k_draw as loops: for every row of the grid the per-lane steps of fastneighbornet_amd/csrc/fnn_draw.h for tid = 0 ... 255,
// a barrier of the kernel being the end of such a loop; the wave reduction as a maximum over each wave's 64 lanes.  The
// row's LDS image is a heap block of exactly the bytes the launch declares, filled with 0xFF first; so is every "device"
// buffer (fnn_small_emu.h): under AddressSanitizer a counter or a plane byte past either is an error.  The distance kernels
// behind it are fnn_dist_model_emu.cpp's, under the product's host logic (dist_bootstrap_batch<B>).
//
// Build: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off (tests/draw_common.py).  Same signatures as include/fastnn.h
// with the prefix emu_ - the model entries of fnn_dist_model_emu.cpp among them -, and emu_bootstrap_draw_planes.
#include "fnn_dist_model_emu.cpp"  // EmuDistModelBackend; emu_last_error and the model entries, exported from here too

namespace {

struct EmuDrawBackend : EmuDistModelBackend {
    int32_t run_draw(const DrawArgs& a, int64_t rows, double* t_draw_s) {
        const double t0 = now_s();
        const int32_t lds_bytes = draw_lds_bytes(a.lpad);
        if (lds_bytes > DRAW_LDS_BYTES) { last = "too many sites for the draw kernel"; return FNN_EHIP; }
        for (int64_t row = 0; row < rows; row++) {
            EmuBlock lds((size_t)lds_bytes);
            if (!lds.p) { last = "out of memory"; return FNN_EHIP; }
            uint32_t* hist = (uint32_t*)lds.p;
            uint32_t most[DRAW_THREADS] = {};
            if (row < a.cnt) {
                for (int tid = 0; tid < DRAW_THREADS; tid++) draw_lane_zero(hist, a.lpad, tid, DRAW_THREADS);
                for (int tid = 0; tid < DRAW_THREADS; tid++) draw_lane_count(a, hist, row, tid, DRAW_THREADS);
                for (int tid = 0; tid < DRAW_THREADS; tid++) most[tid] = draw_lane_planes(a, hist, row, tid, DRAW_THREADS);
            } else
                for (int tid = 0; tid < DRAW_THREADS; tid++) draw_lane_planes(a, nullptr, row, tid, DRAW_THREADS);
            for (int tid = 0; tid < DRAW_THREADS; tid++) draw_lane_row_words(a, row, tid);
            for (int wave = 0; wave < DRAW_THREADS / 64; wave++) {
                uint32_t m = 0;
                for (int lane = 0; lane < 64; lane++) m = most[64 * wave + lane] > m ? most[64 * wave + lane] : m;
                if (m > *a.max_count) *a.max_count = m;
            }
        }
        *t_draw_s = now_s() - t0;
        return FNN_OK;
    }
};

}  // namespace

extern "C" {

int32_t emu_bootstrap_draw_max_sites(void) { return fnn::DRAW_MAX_SITES; }

int32_t emu_bootstrap_distances_batch_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, int64_t batch, uint64_t seed, int64_t lead,
                                          const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride, fnn_boot_stats* stats) {
    try {
        EmuDrawBackend be;
        return fnn::dist_bootstrap_batch(be, "emu_bootstrap_distances_batch_f64", seq, n, L, lds, batch, seed, lead, m, device, D_out, false, ld, stride, stats);
    } catch (const std::exception& e) {
        return fnn::fail(FNN_ESTATE, std::string("exception: ") + e.what());
    }
}

// (the "device" pointer is host memory here: the matrices are written in place, through ld and stride)
int32_t emu_bootstrap_distances_batch_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, int64_t batch, uint64_t seed, int64_t lead,
                                                 const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                 fnn_boot_stats* stats) {
    try {
        EmuDrawBackend be;
        return fnn::dist_bootstrap_batch(be, "emu_bootstrap_distances_batch_device_f64", seq, n, L, lds, batch, seed, lead, m, device, D_out, true, ld,
                                         stride, stats);
    } catch (const std::exception& e) {
        return fnn::fail(FNN_ESTATE, std::string("exception: ") + e.what());
    }
}

// The planes themselves: one launch of the draw over rows = round_up(batch, 64) rows, as the host logic sizes a chunk of `batch`
// problems that starts at problem `first` of the call.  planes_out: digits x rows x lpad bytes, lpad = round_up(L, 64);
// total_out: rows; max_count_out: one word.
int32_t emu_bootstrap_draw_planes(int64_t L, int64_t batch, int64_t first, int64_t lead, uint64_t seed, int32_t digits, int8_t* planes_out,
                                  int64_t* total_out, uint32_t* max_count_out) {
    try {
        using namespace fnn;
        if (L <= 0 || L > DRAW_MAX_SITES || batch <= 0 || digits < 1 || digits > DIST_MAX_DIGITS) return fail(FNN_EINVAL, "emu_bootstrap_draw_planes: bad argument");
        EmuDrawBackend be;
        const int64_t lpad = round_up(L, (int64_t)DIST_K), rows = round_up(batch, (int64_t)DIST_REPS);
        const size_t plane_bytes = (size_t)rows * (size_t)lpad;
        DrawArgs a{};
        a.planes = (int8_t*)be.alloc(plane_bytes * (size_t)digits);
        a.plane_stride = (int64_t)plane_bytes; a.lpad = lpad; a.L = L; a.digits = digits; a.cnt = batch; a.first = first; a.lead = lead; a.seed = seed;
        a.total = (int64_t*)be.alloc(sizeof(int64_t) * (size_t)rows);
        a.bad = (int32_t*)be.alloc(sizeof(int32_t) * (size_t)rows);
        a.sat = (int32_t*)be.alloc(sizeof(int32_t) * (size_t)rows);
        a.max_count = (uint32_t*)be.alloc(sizeof(uint32_t));
        if (!a.planes || !a.total || !a.bad || !a.sat || !a.max_count) return fail(FNN_ENOMEM, "emu_bootstrap_draw_planes: out of memory");
        *a.max_count = 0;
        double t = 0.0;
        if (be.run_draw(a, rows, &t) != FNN_OK) return fail(FNN_EHIP, be.err());
        for (int64_t r = 0; r < rows; r++)
            if (a.bad[r] != 0 || a.sat[r] != 0) return fail(FNN_ESTATE, "emu_bootstrap_draw_planes: a flag was not zeroed");
        std::memcpy(planes_out, a.planes, plane_bytes * (size_t)digits);
        std::memcpy(total_out, a.total, sizeof(int64_t) * (size_t)rows);
        *max_count_out = *a.max_count;
        return FNN_OK;
    } catch (const std::exception& e) {
        return fnn::fail(FNN_ESTATE, std::string("exception: ") + e.what());
    }
}

}  // extern "C"

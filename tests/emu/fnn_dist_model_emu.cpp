// fnn_dist_model_emu.cpp -- TEST INFRASTRUCTURE: CPU driver of the alignment-distance path with the corrected distances
// (DESIGN.md section 16).
//
// As fnn_dist_emu.cpp, for k_dist_model: the per-lane steps of fastneighbornet_amd/csrc/fnn_dist.h and fnn_dist_model.h for
// lane = 0 ... 63 of every wave of the kernel's grid - sized from dist_model_rt like the kernel's -, the tile product as
// loops from the stated lane maps, under the product's host logic (dist_batch_model<B>).  "Device memory" is the heap: every
// buffer has exactly the size the host logic asks for and is filled with 0xFF bytes first (fnn_small_emu.h).
//
// Build: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off (tests/dist_model_common.py).  Same signatures as
// include/fastnn.h with the prefix emu_, and emu_dist_log1p.
#include "../../fastneighbornet_amd/csrc/fnn_dist.h"
#include "fnn_small_emu.h"

namespace {

using namespace fnn;

// MODEL == FNN_DIST_P: k_dist itself
template <int MODEL, int P, bool MISSING, int RT>
void emu_wave(const DistArgs& a, const DistModel& dm, const DistTile& t, int64_t b0) {
    constexpr bool K2P = MODEL == FNN_DIST_K2P;
    DistAcc am[RT][P][64], av[RT][P][64], at[RT][P][64];
    std::memset(am, 0, sizeof(am));
    std::memset(av, 0, sizeof(av));
    std::memset(at, 0, sizeof(at));
    DistFrag fm[64], fv[64], ft[64], fb[64];
    std::memset(fv, 0xFF, sizeof(fv));
    std::memset(ft, 0xFF, sizeof(ft));
    for (int64_t s = 0; s < a.lpad; s += DIST_K) {
        for (int lane = 0; lane < 64; lane++) {
            if (K2P) dist_lane_a_ts<MISSING>(a, t, lane, s, fm[lane], fv[lane], ft[lane]);
            else dist_lane_a<MISSING>(a, t, lane, s, fm[lane], fv[lane]);
        }
        for (int rt = 0; rt < RT; rt++)
            for (int d = 0; d < P; d++) {
                for (int lane = 0; lane < 64; lane++) fb[lane] = dist_lane_b(a, b0, rt, d, lane, s);
                dist_tile_product(fm, fb, am[rt][d]);
                if (MISSING) dist_tile_product(fv, fb, av[rt][d]);
                if (K2P) dist_tile_product(ft, fb, at[rt][d]);
            }
    }
    for (int rt = 0; rt < RT; rt++)
        for (int lane = 0; lane < 64; lane++) {
            DistAcc m[P], v[P], x[P];
            for (int d = 0; d < P; d++) { m[d] = am[rt][d][lane]; v[d] = av[rt][d][lane]; x[d] = at[rt][d][lane]; }
            if constexpr (MODEL == FNN_DIST_P) dist_lane_store<P, MISSING>(a, t, b0 + DIST_TILE * rt, lane, m, v);
            else dist_lane_store_model<MODEL, P, MISSING>(a, dm, t, b0 + DIST_TILE * rt, lane, m, v, x);
        }
}

struct EmuDistModelBackend : EmuHeapBackend {
    template <int MODEL, int P, bool MISSING>
    void grid(const DistArgs& a, const DistModel& dm, int64_t tile_groups, int64_t cnt) {
        constexpr int RT = MODEL == FNN_DIST_P ? DIST_RT : dist_model_rt(MODEL, P, MISSING);
        const int64_t rep_groups = round_up(cnt, (int64_t)(DIST_TILE * RT)) / (DIST_TILE * RT);
        for (int64_t blk = 0; blk < tile_groups * rep_groups; blk++) {
            const int64_t rg = blk / tile_groups, tg = blk - rg * tile_groups;
            for (int wave = 0; wave < DIST_WAVES; wave++) emu_wave<MODEL, P, MISSING, RT>(a, dm, a.tiles[tg * DIST_WAVES + wave], rg * (DIST_TILE * RT));
        }
    }
    template <int MODEL>
    int32_t run_of(int32_t P, bool missing, const DistArgs& a, const DistModel& dm, int64_t tile_groups, int64_t cnt, double* t_kernel_s) {
        const double t0 = now_s();
        switch (P * 2 + (missing ? 1 : 0)) {
            case 2: grid<MODEL, 1, false>(a, dm, tile_groups, cnt); break;
            case 3: grid<MODEL, 1, true>(a, dm, tile_groups, cnt); break;
            case 4: grid<MODEL, 2, false>(a, dm, tile_groups, cnt); break;
            case 5: grid<MODEL, 2, true>(a, dm, tile_groups, cnt); break;
            case 6: grid<MODEL, 3, false>(a, dm, tile_groups, cnt); break;
            case 7: grid<MODEL, 3, true>(a, dm, tile_groups, cnt); break;
            default: last = "no kernel for " + std::to_string(P) + " digits"; return FNN_EHIP;
        }
        *t_kernel_s = now_s() - t0;
        return FNN_OK;
    }
    int32_t run(int32_t P, bool missing, const DistArgs& a, int64_t tile_groups, int64_t rep_groups, double* t_kernel_s) {
        return run_of<FNN_DIST_P>(P, missing, a, DistModel{}, tile_groups, a.cnt, t_kernel_s);
    }
    int32_t run_model(int32_t model, int32_t P, bool missing, const DistArgs& a, const DistModel& dm, int64_t tile_groups, int64_t cnt, double* t_kernel_s) {
        if (model == FNN_DIST_JC69) return run_of<FNN_DIST_JC69>(P, missing, a, dm, tile_groups, cnt, t_kernel_s);
        if (model == FNN_DIST_K2P) return run_of<FNN_DIST_K2P>(P, missing, a, dm, tile_groups, cnt, t_kernel_s);
        last = "no kernel for model " + std::to_string(model);
        return FNN_EHIP;
    }
};

}  // namespace

extern "C" {

const char* emu_last_error(void) { return fnn::g_last_error.c_str(); }

double emu_dist_log1p(double x) { return fnn::dist_log1p(x); }

int32_t emu_alignment_distances_model_batch_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch, int64_t ldc,
                                                const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                fnn_dist_model_stats* stats) {
    try {
        EmuDistModelBackend be;
        return fnn::dist_batch_model(be, "emu_alignment_distances_model_batch_f64", seq, n, L, lds, counts, batch, ldc, m, device, D_out, false, ld, stride,
                                     stats);
    } catch (const std::exception& e) {
        return fnn::fail(FNN_ESTATE, std::string("exception: ") + e.what());
    }
}

// (the "device" pointer is host memory here: the matrices are written in place, through ld and stride)
int32_t emu_alignment_distances_model_batch_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch,
                                                       int64_t ldc, const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                       fnn_dist_model_stats* stats) {
    try {
        EmuDistModelBackend be;
        return fnn::dist_batch_model(be, "emu_alignment_distances_model_batch_device_f64", seq, n, L, lds, counts, batch, ldc, m, device, D_out, true, ld,
                                     stride, stats);
    } catch (const std::exception& e) {
        return fnn::fail(FNN_ESTATE, std::string("exception: ") + e.what());
    }
}

}  // extern "C"

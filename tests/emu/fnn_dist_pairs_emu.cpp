// fnn_dist_pairs_emu.cpp -- TEST INFRASTRUCTURE: CPU driver of the alignment-distance path with the 4 x 4 tables of state
// pairs.
//
// As fnn_dist_model_emu.cpp, for k_dist_pairs: the per-lane steps of fastneighbornet_amd/csrc/fnn_dist_pairs.h and
// fnn_dist_model.h for lane = 0 ... 63 of every wave of the kernel's grid - sized from dist_pairs_rt like the kernel's -, the
// tile product as loops from the stated lane maps, under the product's host logic.  The other kernels behind it, k_draw
// among them, are fnn_draw_emu.cpp's.  "Device memory" is the heap: every buffer has exactly the size the host logic asks for
// and is filled with 0xFF bytes first (fnn_small_emu.h).
//
// Build: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off (tests/dist_pairs_common.py).  The model, bootstrap and table
// entries of include/fastnn.h with the prefix emup_ (fnn_draw_emu.cpp's emu_ entries know no table), and emup_dist_log.
#include "fnn_draw_emu.cpp"  // EmuDrawBackend

namespace {

template <int MODEL, int P, int RT>
void emu_wave_pairs(const DistArgs& a, const DistPairs& dp, const DistTile& t, int64_t b0) {
    DistAcc acc[RT][DIST_PAIR_CELLS][P][64];
    std::memset(acc, 0, sizeof(acc));
    DistFrag f[DIST_PAIR_CELLS][64];
    DistFrag fb[64];
    for (int64_t s = 0; s < a.lpad; s += DIST_K) {
        for (int lane = 0; lane < 64; lane++) {
            DistFrag fl[DIST_PAIR_CELLS];
            dist_lane_a_pairs(a, t, lane, s, fl);
            for (int c = 0; c < DIST_PAIR_CELLS; c++) f[c][lane] = fl[c];
        }
        for (int rt = 0; rt < RT; rt++)
            for (int d = 0; d < P; d++) {
                for (int lane = 0; lane < 64; lane++) fb[lane] = dist_lane_b(a, b0, rt, d, lane, s);
                for (int c = 0; c < DIST_PAIR_CELLS; c++) dist_tile_product(f[c], fb, acc[rt][c][d]);
            }
    }
    for (int rt = 0; rt < RT; rt++)
        for (int lane = 0; lane < 64; lane++) {
            DistAcc mine[DIST_PAIR_CELLS][P];
            for (int c = 0; c < DIST_PAIR_CELLS; c++)
                for (int d = 0; d < P; d++) mine[c][d] = acc[rt][c][d][lane];
            dist_lane_store_pairs<MODEL, P>(a, dp, t, b0 + DIST_TILE * rt, lane, mine);
        }
}

struct EmuDistPairsBackend : EmuDrawBackend {
    template <int MODEL, int P>
    void grid_pairs(const DistArgs& a, const DistPairs& dp, int64_t tile_groups, int64_t cnt) {
        constexpr int RT = dist_pairs_rt(P);
        const int64_t rep_groups = round_up(cnt, (int64_t)(DIST_TILE * RT)) / (DIST_TILE * RT);
        for (int64_t blk = 0; blk < tile_groups * rep_groups; blk++) {
            const int64_t rg = blk / tile_groups, tg = blk - rg * tile_groups;
            for (int wave = 0; wave < DIST_WAVES; wave++) emu_wave_pairs<MODEL, P, RT>(a, dp, a.tiles[tg * DIST_WAVES + wave], rg * (DIST_TILE * RT));
        }
    }
    template <int MODEL>
    int32_t run_pairs_of(int32_t P, const DistArgs& a, const DistPairs& dp, int64_t tile_groups, int64_t cnt, double* t_kernel_s) {
        const double t0 = now_s();
        switch (P) {
            case 1: grid_pairs<MODEL, 1>(a, dp, tile_groups, cnt); break;
            case 2: grid_pairs<MODEL, 2>(a, dp, tile_groups, cnt); break;
            case 3: grid_pairs<MODEL, 3>(a, dp, tile_groups, cnt); break;
            default: last = "no kernel for " + std::to_string(P) + " digits"; return FNN_EHIP;
        }
        *t_kernel_s = now_s() - t0;
        return FNN_OK;
    }
    int32_t run_pairs(int32_t model, int32_t P, const DistArgs& a, const DistPairs& dp, int64_t tile_groups, int64_t cnt, double* t_kernel_s) {
        switch (model) {
            case FNN_DIST_F81: return run_pairs_of<FNN_DIST_F81>(P, a, dp, tile_groups, cnt, t_kernel_s);
            case FNN_DIST_F84: return run_pairs_of<FNN_DIST_F84>(P, a, dp, tile_groups, cnt, t_kernel_s);
            case FNN_DIST_TN93: return run_pairs_of<FNN_DIST_TN93>(P, a, dp, tile_groups, cnt, t_kernel_s);
            case FNN_DIST_LOGDET: return run_pairs_of<FNN_DIST_LOGDET>(P, a, dp, tile_groups, cnt, t_kernel_s);
            case DIST_PAIR_COUNTS: return run_pairs_of<DIST_PAIR_COUNTS>(P, a, dp, tile_groups, cnt, t_kernel_s);
        }
        last = "no kernel for model " + std::to_string(model);
        return FNN_EHIP;
    }
};

template <class F>
int32_t emup_try(F&& f) {
    try {
        return f();
    } catch (const std::exception& e) {
        return fnn::fail(FNN_ESTATE, std::string("exception: ") + e.what());
    }
}

}  // namespace

extern "C" {

const char* emup_last_error(void) { return fnn::g_last_error.c_str(); }

double emup_dist_log(double x) { return fnn::dist_log(x); }

int32_t emup_alignment_distances_model_batch_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch, int64_t ldc,
                                                 const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                 fnn_dist_model_stats* stats) {
    return emup_try([&] {
        EmuDistPairsBackend be;
        return fnn::dist_batch_model(be, "emup_alignment_distances_model_batch_f64", seq, n, L, lds, counts, batch, ldc, m, device, D_out, false, ld, stride,
                                     stats);
    });
}

// (the "device" pointers are host memory here: the output is written in place, through ld and stride)
int32_t emup_alignment_distances_model_batch_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch,
                                                        int64_t ldc, const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                        fnn_dist_model_stats* stats) {
    return emup_try([&] {
        EmuDistPairsBackend be;
        return fnn::dist_batch_model(be, "emup_alignment_distances_model_batch_device_f64", seq, n, L, lds, counts, batch, ldc, m, device, D_out, true, ld,
                                     stride, stats);
    });
}

int32_t emup_alignment_pair_counts_batch_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch, int64_t ldc,
                                             int32_t device, int64_t* F_out, int64_t ld, int64_t stride, fnn_dist_model_stats* stats) {
    return emup_try([&] {
        EmuDistPairsBackend be;
        return fnn::dist_batch_pair_counts(be, "emup_alignment_pair_counts_batch_i64", seq, n, L, lds, counts, batch, ldc, device, F_out, false, ld, stride,
                                           stats);
    });
}

int32_t emup_alignment_pair_counts_batch_device_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch,
                                                    int64_t ldc, int32_t device, int64_t* F_out, int64_t ld, int64_t stride, fnn_dist_model_stats* stats) {
    return emup_try([&] {
        EmuDistPairsBackend be;
        return fnn::dist_batch_pair_counts(be, "emup_alignment_pair_counts_batch_device_i64", seq, n, L, lds, counts, batch, ldc, device, F_out, true, ld,
                                           stride, stats);
    });
}

int32_t emup_bootstrap_draw_max_sites(void) { return fnn::DRAW_MAX_SITES; }

int32_t emup_bootstrap_distances_batch_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, int64_t batch, uint64_t seed, int64_t lead,
                                           const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride, fnn_boot_stats* stats) {
    return emup_try([&] {
        EmuDistPairsBackend be;
        return fnn::dist_bootstrap_batch(be, "emup_bootstrap_distances_batch_f64", seq, n, L, lds, batch, seed, lead, m, device, D_out, false, ld, stride,
                                         stats);
    });
}

int32_t emup_bootstrap_distances_batch_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, int64_t batch, uint64_t seed, int64_t lead,
                                                  const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                  fnn_boot_stats* stats) {
    return emup_try([&] {
        EmuDistPairsBackend be;
        return fnn::dist_bootstrap_batch(be, "emup_bootstrap_distances_batch_device_f64", seq, n, L, lds, batch, seed, lead, m, device, D_out, true, ld,
                                         stride, stats);
    });
}

}  // extern "C"

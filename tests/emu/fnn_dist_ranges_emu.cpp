// fnn_dist_ranges_emu.cpp -- TEST INFRASTRUCTURE: CPU driver of the alignment distances over site ranges.
//
// As fnn_dist_pairs_emu.cpp, for k_dist_ranges and k_dist_ranges_pairs: the per-lane steps of
// fastneighbornet_amd/csrc/fnn_dist_ranges.h - the bounds of a lane's column, the B operand from them, the walk over the tile's
// span - and the A operands and epilogues of fnn_dist.h / fnn_dist_pairs.h for lane = 0 ... 63 of every wave of the kernels' grids,
// one pair tile against one window tile each, the tile product as loops from the stated lane maps, under the product's host logic
// (dist_batch_ranges<B>).  "Device memory" is the heap: every buffer - the bounds and the span table among them - has exactly
// the size the host logic asks for and is filled with 0xFF bytes first (fnn_small_emu.h); no plane exists.
//
// Build: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off (tests/dist_ranges_common.py).  The range entries of
// include/fastnn.h with the prefix emur_, and the counts entries they are compared with under the same prefix.
#include "fnn_dist_gamma_emu.cpp"  // EmuDistPairsBackend, emup_try

namespace {

template <int MODEL, bool MISSING>
void emu_wave_ranges(const DistArgs& a, const DistRanges& dr, const DistModel& dm, const DistTile& t, int64_t wt) {
    constexpr bool K2P = MODEL == FNN_DIST_K2P;
    const int64_t b0 = wt * DIST_TILE;
    DistAcc am[64], av[64], at[64];
    std::memset(am, 0, sizeof(am));
    std::memset(av, 0, sizeof(av));
    std::memset(at, 0, sizeof(at));
    const DistSpan sp = dr.spans[wt];
    DistRangeLane rl[64];
    for (int lane = 0; lane < 64; lane++) rl[lane] = dist_lane_range(dr, b0, lane);
    DistFrag fm[64], fv[64], ft[64], fb[64];
    std::memset(fv, 0xFF, sizeof(fv));
    std::memset(ft, 0xFF, sizeof(ft));
    for (int32_t s = sp.lo; s < sp.hi; s += DIST_K) {
        for (int lane = 0; lane < 64; lane++) {
            if (K2P) dist_lane_a_ts<MISSING>(a, t, lane, s, fm[lane], fv[lane], ft[lane]);
            else dist_lane_a<MISSING>(a, t, lane, s, fm[lane], fv[lane]);
            fb[lane] = dist_lane_b_range(rl[lane], lane, s);
        }
        dist_tile_product(fm, fb, am);
        if (MISSING) dist_tile_product(fv, fb, av);
        if (K2P) dist_tile_product(ft, fb, at);
    }
    for (int lane = 0; lane < 64; lane++) {
        const DistAcc m[1] = {am[lane]}, v[1] = {av[lane]}, x[1] = {at[lane]};
        if constexpr (MODEL == FNN_DIST_P) dist_lane_store<1, MISSING>(a, t, b0, lane, m, v);
        else dist_lane_store_model<MODEL, 1, MISSING>(a, dm, t, b0, lane, m, v, x);
    }
}

template <int MODEL>
void emu_wave_ranges_pairs(const DistArgs& a, const DistRanges& dr, const DistPairs& dp, const DistTile& t, int64_t wt) {
    const int64_t b0 = wt * DIST_TILE;
    DistAcc acc[DIST_PAIR_CELLS][64];
    std::memset(acc, 0, sizeof(acc));
    const DistSpan sp = dr.spans[wt];
    DistRangeLane rl[64];
    for (int lane = 0; lane < 64; lane++) rl[lane] = dist_lane_range(dr, b0, lane);
    DistFrag f[DIST_PAIR_CELLS][64], fb[64];
    for (int32_t s = sp.lo; s < sp.hi; s += DIST_K) {
        for (int lane = 0; lane < 64; lane++) {
            DistFrag fl[DIST_PAIR_CELLS];
            dist_lane_a_pairs(a, t, lane, s, fl);
            for (int c = 0; c < DIST_PAIR_CELLS; c++) f[c][lane] = fl[c];
            fb[lane] = dist_lane_b_range(rl[lane], lane, s);
        }
        for (int c = 0; c < DIST_PAIR_CELLS; c++) dist_tile_product(f[c], fb, acc[c]);
    }
    for (int lane = 0; lane < 64; lane++) {
        DistAcc mine[DIST_PAIR_CELLS][1];
        for (int c = 0; c < DIST_PAIR_CELLS; c++) mine[c][0] = acc[c][lane];
        dist_lane_store_pairs<MODEL, 1>(a, dp, t, b0, lane, mine);
    }
}

struct EmuDistRangesBackend : EmuDistPairsBackend {
    template <int MODEL, bool MISSING>
    void grid_ranges(const DistArgs& a, const DistRanges& dr, const DistModel& dm, int64_t tile_groups, int64_t cnt) {
        const int64_t win_tiles = round_up(cnt, (int64_t)DIST_TILE) / DIST_TILE;
        for (int64_t blk = 0; blk < tile_groups * win_tiles; blk++) {
            const int64_t wt = blk / tile_groups, tg = blk - wt * tile_groups;
            for (int wave = 0; wave < DIST_WAVES; wave++) emu_wave_ranges<MODEL, MISSING>(a, dr, dm, a.tiles[tg * DIST_WAVES + wave], wt);
        }
    }
    template <int MODEL>
    int32_t run_ranges_of(bool missing, const DistArgs& a, const DistRanges& dr, const DistModel& dm, int64_t tile_groups, int64_t cnt, double* t_kernel_s) {
        const double t0 = now_s();
        if (missing) grid_ranges<MODEL, true>(a, dr, dm, tile_groups, cnt);
        else grid_ranges<MODEL, false>(a, dr, dm, tile_groups, cnt);
        *t_kernel_s = now_s() - t0;
        return FNN_OK;
    }
    int32_t run_ranges(int32_t model, bool missing, const DistArgs& a, const DistRanges& dr, const DistModel& dm, int64_t tile_groups, int64_t cnt,
                       double* t_kernel_s) {
        if (model == FNN_DIST_P) return run_ranges_of<FNN_DIST_P>(missing, a, dr, dm, tile_groups, cnt, t_kernel_s);
        if (model == FNN_DIST_JC69) return run_ranges_of<FNN_DIST_JC69>(missing, a, dr, dm, tile_groups, cnt, t_kernel_s);
        if (model == FNN_DIST_K2P) return run_ranges_of<FNN_DIST_K2P>(missing, a, dr, dm, tile_groups, cnt, t_kernel_s);
        last = "no kernel for model " + std::to_string(model);
        return FNN_EHIP;
    }
    template <int MODEL>
    int32_t run_ranges_pairs_of(const DistArgs& a, const DistRanges& dr, const DistPairs& dp, int64_t tile_groups, int64_t cnt, double* t_kernel_s) {
        const double t0 = now_s();
        const int64_t win_tiles = round_up(cnt, (int64_t)DIST_TILE) / DIST_TILE;
        for (int64_t blk = 0; blk < tile_groups * win_tiles; blk++) {
            const int64_t wt = blk / tile_groups, tg = blk - wt * tile_groups;
            for (int wave = 0; wave < DIST_WAVES; wave++) emu_wave_ranges_pairs<MODEL>(a, dr, dp, a.tiles[tg * DIST_WAVES + wave], wt);
        }
        *t_kernel_s = now_s() - t0;
        return FNN_OK;
    }
    int32_t run_ranges_pairs(int32_t model, const DistArgs& a, const DistRanges& dr, const DistPairs& dp, int64_t tile_groups, int64_t cnt, double* t_kernel_s) {
        switch (model) {
            case FNN_DIST_F81: return run_ranges_pairs_of<FNN_DIST_F81>(a, dr, dp, tile_groups, cnt, t_kernel_s);
            case FNN_DIST_F84: return run_ranges_pairs_of<FNN_DIST_F84>(a, dr, dp, tile_groups, cnt, t_kernel_s);
            case FNN_DIST_TN93: return run_ranges_pairs_of<FNN_DIST_TN93>(a, dr, dp, tile_groups, cnt, t_kernel_s);
            case FNN_DIST_LOGDET: return run_ranges_pairs_of<FNN_DIST_LOGDET>(a, dr, dp, tile_groups, cnt, t_kernel_s);
            case DIST_PAIR_COUNTS: return run_ranges_pairs_of<DIST_PAIR_COUNTS>(a, dr, dp, tile_groups, cnt, t_kernel_s);
        }
        last = "no kernel for model " + std::to_string(model);
        return FNN_EHIP;
    }
};

}  // namespace

extern "C" {

const char* emur_last_error(void) { return fnn::g_last_error.c_str(); }

// (the "device" pointers are host memory here: the output is written in place, through ld and stride)
int32_t emur_alignment_distances_ranges_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts, const int64_t* ends, int64_t batch,
                                            const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride, fnn_range_stats* stats) {
    return emup_try([&] {
        EmuDistRangesBackend be;
        return fnn::dist_batch_ranges(be, "emur_alignment_distances_ranges_f64", seq, n, L, lds, starts, ends, batch, m, false, device, D_out, false, ld, stride,
                                      stats);
    });
}

int32_t emur_alignment_distances_ranges_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts, const int64_t* ends,
                                                   int64_t batch, const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                   fnn_range_stats* stats) {
    return emup_try([&] {
        EmuDistRangesBackend be;
        return fnn::dist_batch_ranges(be, "emur_alignment_distances_ranges_device_f64", seq, n, L, lds, starts, ends, batch, m, false, device, D_out, true, ld,
                                      stride, stats);
    });
}

int32_t emur_alignment_pair_counts_ranges_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts, const int64_t* ends, int64_t batch,
                                              int32_t device, int64_t* F_out, int64_t ld, int64_t stride, fnn_range_stats* stats) {
    return emup_try([&] {
        EmuDistRangesBackend be;
        return fnn::dist_batch_ranges(be, "emur_alignment_pair_counts_ranges_i64", seq, n, L, lds, starts, ends, batch, nullptr, true, device,
                                      reinterpret_cast<double*>(F_out), false, ld, stride, stats);
    });
}

int32_t emur_alignment_pair_counts_ranges_device_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts, const int64_t* ends,
                                                     int64_t batch, int32_t device, int64_t* F_out, int64_t ld, int64_t stride, fnn_range_stats* stats) {
    return emup_try([&] {
        EmuDistRangesBackend be;
        return fnn::dist_batch_ranges(be, "emur_alignment_pair_counts_ranges_device_i64", seq, n, L, lds, starts, ends, batch, nullptr, true, device,
                                      reinterpret_cast<double*>(F_out), true, ld, stride, stats);
    });
}

// the counts entries behind the same backend: what the range entries are compared with
int32_t emur_alignment_distances_model_batch_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch, int64_t ldc,
                                                 const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                 fnn_dist_model_stats* stats) {
    return emup_try([&] {
        EmuDistRangesBackend be;
        return fnn::dist_batch_model(be, "emur_alignment_distances_model_batch_f64", seq, n, L, lds, counts, batch, ldc, m, device, D_out, false, ld, stride,
                                     stats);
    });
}

int32_t emur_alignment_distances_model_batch_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch,
                                                        int64_t ldc, const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                        fnn_dist_model_stats* stats) {
    return emup_try([&] {
        EmuDistRangesBackend be;
        return fnn::dist_batch_model(be, "emur_alignment_distances_model_batch_device_f64", seq, n, L, lds, counts, batch, ldc, m, device, D_out, true, ld,
                                     stride, stats);
    });
}

int32_t emur_alignment_pair_counts_batch_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch, int64_t ldc,
                                             int32_t device, int64_t* F_out, int64_t ld, int64_t stride, fnn_dist_model_stats* stats) {
    return emup_try([&] {
        EmuDistRangesBackend be;
        return fnn::dist_batch_pair_counts(be, "emur_alignment_pair_counts_batch_i64", seq, n, L, lds, counts, batch, ldc, device, F_out, false, ld, stride,
                                           stats);
    });
}

int32_t emur_alignment_pair_counts_batch_device_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch,
                                                    int64_t ldc, int32_t device, int64_t* F_out, int64_t ld, int64_t stride, fnn_dist_model_stats* stats) {
    return emup_try([&] {
        EmuDistRangesBackend be;
        return fnn::dist_batch_pair_counts(be, "emur_alignment_pair_counts_batch_device_i64", seq, n, L, lds, counts, batch, ldc, device, F_out, true, ld,
                                           stride, stats);
    });
}

}  // extern "C"

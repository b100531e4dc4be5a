// fnn_bootscan_emu.cpp -- TEST INFRASTRUCTURE: CPU driver of the bootscan entries.
//
// As fnn_dist_ranges_emu.cpp, for k_draw_ranges, k_dist_scan and k_dist_scan_pairs: the per-lane steps of
// fastneighbornet_amd/csrc/fnn_scan.h - a row's window, its draws into a histogram over the window's span, the compact plane row,
// the B operand read at s - lo, the group's bound of the epilogue - and the A operands and epilogues of fnn_dist.h /
// fnn_dist_pairs.h for tid = 0 ... 255 of every row of the draw's grid and lane = 0 ... 63 of every wave of the distance kernels'
// grids, one pair tile against one column group each, under the product's host logic (dist_batch_scan<B>).  "Device memory" is the
// heap: every buffer - the window and group tables and the compact planes among them - has exactly the size the host logic asks
// for and is filled with 0xFF bytes first (fnn_small_emu.h); a row's LDS image is a block of exactly the bytes the launch declares.
//
// Build: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off (tests/bootscan_common.py).  The bootscan entries of include/fastnn.h
// with the prefix emus_, the counts and bootstrap entries they are compared with under the same prefix, and
// emus_bootscan_draw_planes.
#include "fnn_dist_ranges_emu.cpp"  // EmuDistRangesBackend, emup_try

namespace {

template <int MODEL, bool MISSING>
void emu_wave_scan(const DistArgs& a, const ScanArgs& sa, const DistModel& dm, const DistTile& t, int64_t cg) {
    constexpr bool K2P = MODEL == FNN_DIST_K2P;
    const ScanGroup g = sa.groups[cg];
    DistAcc am[DIST_RT][64], av[DIST_RT][64], at[DIST_RT][64];
    std::memset(am, 0, sizeof(am));
    std::memset(av, 0, sizeof(av));
    std::memset(at, 0, sizeof(at));
    const int8_t* rows[DIST_RT][64];
    for (int rt = 0; rt < DIST_RT; rt++)
        for (int lane = 0; lane < 64; lane++) rows[rt][lane] = scan_lane_row(sa, g, rt, lane);
    DistFrag fm[64], fv[64], ft[64], fb[64];
    std::memset(fv, 0xFF, sizeof(fv));
    std::memset(ft, 0xFF, sizeof(ft));
    for (int32_t s = g.lo; s < g.hi; s += DIST_K) {
        for (int lane = 0; lane < 64; lane++) {
            if (K2P) dist_lane_a_ts<MISSING>(a, t, lane, s, fm[lane], fv[lane], ft[lane]);
            else dist_lane_a<MISSING>(a, t, lane, s, fm[lane], fv[lane]);
        }
        for (int rt = 0; rt < DIST_RT; rt++) {
            if (DIST_TILE * rt >= g.rows) continue;
            for (int lane = 0; lane < 64; lane++) fb[lane] = scan_lane_b(rows[rt][lane], g, s);
            dist_tile_product(fm, fb, am[rt]);
            if (MISSING) dist_tile_product(fv, fb, av[rt]);
            if (K2P) dist_tile_product(ft, fb, at[rt]);
        }
    }
    const DistArgs al = scan_group_args(a, g);
    for (int rt = 0; rt < DIST_RT; rt++)
        for (int lane = 0; lane < 64; lane++) {
            const DistAcc m[1] = {am[rt][lane]}, v[1] = {av[rt][lane]}, x[1] = {at[rt][lane]};
            if constexpr (MODEL == FNN_DIST_P) dist_lane_store<1, MISSING>(al, t, (int64_t)g.row0 + DIST_TILE * rt, lane, m, v);
            else dist_lane_store_model<MODEL, 1, MISSING>(al, dm, t, (int64_t)g.row0 + DIST_TILE * rt, lane, m, v, x);
        }
}

template <int MODEL>
void emu_wave_scan_pairs(const DistArgs& a, const ScanArgs& sa, const DistPairs& dp, const DistTile& t, int64_t cg) {
    constexpr int RT = dist_pairs_rt(1);
    const ScanGroup g = sa.groups[cg];
    static thread_local DistAcc acc[RT][DIST_PAIR_CELLS][64];
    std::memset(acc, 0, sizeof(acc));
    const int8_t* rows[RT][64];
    for (int rt = 0; rt < RT; rt++)
        for (int lane = 0; lane < 64; lane++) rows[rt][lane] = scan_lane_row(sa, g, rt, lane);
    DistFrag f[DIST_PAIR_CELLS][64], fb[64];
    for (int32_t s = g.lo; s < g.hi; s += DIST_K) {
        for (int lane = 0; lane < 64; lane++) {
            DistFrag fl[DIST_PAIR_CELLS];
            dist_lane_a_pairs(a, t, lane, s, fl);
            for (int c = 0; c < DIST_PAIR_CELLS; c++) f[c][lane] = fl[c];
        }
        for (int rt = 0; rt < RT; rt++) {
            if (DIST_TILE * rt >= g.rows) continue;
            for (int lane = 0; lane < 64; lane++) fb[lane] = scan_lane_b(rows[rt][lane], g, s);
            for (int c = 0; c < DIST_PAIR_CELLS; c++) dist_tile_product(f[c], fb, acc[rt][c]);
        }
    }
    const DistArgs al = scan_group_args(a, g);
    for (int rt = 0; rt < RT; rt++)
        for (int lane = 0; lane < 64; lane++) {
            DistAcc mine[DIST_PAIR_CELLS][1];
            for (int c = 0; c < DIST_PAIR_CELLS; c++) mine[c][0] = acc[rt][c][lane];
            dist_lane_store_pairs<MODEL, 1>(al, dp, t, (int64_t)g.row0 + DIST_TILE * rt, lane, mine);
        }
}

struct EmuScanBackend : EmuDistRangesBackend {
    int32_t run_draw_ranges(const ScanArgs& a, int64_t rows, int32_t span, double* t_draw_s) {
        const double t0 = now_s();
        const int32_t lds_bytes = draw_lds_bytes(span);
        if (lds_bytes > DRAW_LDS_BYTES) { last = "too many sites for the draw kernel"; return FNN_EHIP; }
        for (int64_t row = 0; row < rows; row++) {
            EmuBlock lds((size_t)lds_bytes);
            if (!lds.p) { last = "out of memory"; return FNN_EHIP; }
            uint32_t* hist = (uint32_t*)lds.p;
            uint32_t most[DRAW_THREADS] = {};
            const ScanWindow w = scan_row_window(a, row);
            for (int tid = 0; tid < DRAW_THREADS; tid++) draw_lane_zero(hist, w.hi - w.lo, tid, DRAW_THREADS);
            for (int tid = 0; tid < DRAW_THREADS; tid++) scan_lane_count(a, w, hist, row, tid, DRAW_THREADS);
            for (int tid = 0; tid < DRAW_THREADS; tid++) most[tid] = scan_lane_plane(a, w, hist, row, tid, DRAW_THREADS);
            for (int tid = 0; tid < DRAW_THREADS; tid++) scan_lane_row_words(a, w, row, tid);
            for (int wave = 0; wave < DRAW_THREADS / 64; wave++) {
                uint32_t m = 0;
                for (int lane = 0; lane < 64; lane++) m = most[64 * wave + lane] > m ? most[64 * wave + lane] : m;
                if (m > *a.max_count) *a.max_count = m;
            }
        }
        *t_draw_s = now_s() - t0;
        return FNN_OK;
    }
    template <int MODEL>
    int32_t run_scan_of(bool missing, const DistArgs& a, const ScanArgs& sa, const DistModel& dm, int64_t tile_groups, int64_t groups, double* t_kernel_s) {
        const double t0 = now_s();
        for (int64_t blk = 0; blk < tile_groups * groups; blk++) {
            const int64_t cg = blk / tile_groups, tg = blk - cg * tile_groups;
            for (int wave = 0; wave < DIST_WAVES; wave++) {
                if (missing) emu_wave_scan<MODEL, true>(a, sa, dm, a.tiles[tg * DIST_WAVES + wave], cg);
                else emu_wave_scan<MODEL, false>(a, sa, dm, a.tiles[tg * DIST_WAVES + wave], cg);
            }
        }
        *t_kernel_s = now_s() - t0;
        return FNN_OK;
    }
    int32_t run_scan(int32_t model, bool missing, const DistArgs& a, const ScanArgs& sa, const DistModel& dm, int64_t tile_groups, int64_t groups,
                     double* t_kernel_s) {
        if (model == FNN_DIST_P) return run_scan_of<FNN_DIST_P>(missing, a, sa, dm, tile_groups, groups, t_kernel_s);
        if (model == FNN_DIST_JC69) return run_scan_of<FNN_DIST_JC69>(missing, a, sa, dm, tile_groups, groups, t_kernel_s);
        if (model == FNN_DIST_K2P) return run_scan_of<FNN_DIST_K2P>(missing, a, sa, dm, tile_groups, groups, t_kernel_s);
        last = "no kernel for model " + std::to_string(model);
        return FNN_EHIP;
    }
    template <int MODEL>
    int32_t run_scan_pairs_of(const DistArgs& a, const ScanArgs& sa, const DistPairs& dp, int64_t tile_groups, int64_t groups, double* t_kernel_s) {
        const double t0 = now_s();
        for (int64_t blk = 0; blk < tile_groups * groups; blk++) {
            const int64_t cg = blk / tile_groups, tg = blk - cg * tile_groups;
            for (int wave = 0; wave < DIST_WAVES; wave++) emu_wave_scan_pairs<MODEL>(a, sa, dp, a.tiles[tg * DIST_WAVES + wave], cg);
        }
        *t_kernel_s = now_s() - t0;
        return FNN_OK;
    }
    int32_t run_scan_pairs(int32_t model, const DistArgs& a, const ScanArgs& sa, const DistPairs& dp, int64_t tile_groups, int64_t groups, double* t_kernel_s) {
        switch (model) {
            case FNN_DIST_F81: return run_scan_pairs_of<FNN_DIST_F81>(a, sa, dp, tile_groups, groups, t_kernel_s);
            case FNN_DIST_F84: return run_scan_pairs_of<FNN_DIST_F84>(a, sa, dp, tile_groups, groups, t_kernel_s);
            case FNN_DIST_TN93: return run_scan_pairs_of<FNN_DIST_TN93>(a, sa, dp, tile_groups, groups, t_kernel_s);
            case FNN_DIST_LOGDET: return run_scan_pairs_of<FNN_DIST_LOGDET>(a, sa, dp, tile_groups, groups, t_kernel_s);
            case DIST_PAIR_COUNTS: return run_scan_pairs_of<DIST_PAIR_COUNTS>(a, sa, dp, tile_groups, groups, t_kernel_s);
        }
        last = "no kernel for model " + std::to_string(model);
        return FNN_EHIP;
    }
};

}  // namespace

extern "C" {

const char* emus_last_error(void) { return fnn::g_last_error.c_str(); }

int32_t emus_bootscan_counts(int64_t L, const int64_t* starts, const int64_t* ends, int64_t windows, int64_t replicates, int64_t lead, uint64_t seed,
                             int64_t first, int64_t count, uint16_t* counts_out) {
    return emup_try([&] { return fnn::dist_bootscan_counts("emus_bootscan_counts", L, starts, ends, windows, replicates, lead, seed, first, count, counts_out); });
}

// (the "device" pointers are host memory here: the output is written in place, through ld and stride)
int32_t emus_bootscan_distances_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts, const int64_t* ends, int64_t windows,
                                    int64_t replicates, uint64_t seed, int64_t lead, const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld,
                                    int64_t stride, fnn_scan_stats* stats) {
    return emup_try([&] {
        EmuScanBackend be;
        return fnn::dist_batch_scan(be, "emus_bootscan_distances_f64", seq, n, L, lds, starts, ends, windows, replicates, seed, lead, m, false, device, D_out,
                                    false, ld, stride, stats);
    });
}

int32_t emus_bootscan_distances_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts, const int64_t* ends, int64_t windows,
                                           int64_t replicates, uint64_t seed, int64_t lead, const fnn_dist_model* m, int32_t device, double* D_out,
                                           int64_t ld, int64_t stride, fnn_scan_stats* stats) {
    return emup_try([&] {
        EmuScanBackend be;
        return fnn::dist_batch_scan(be, "emus_bootscan_distances_device_f64", seq, n, L, lds, starts, ends, windows, replicates, seed, lead, m, false, device,
                                    D_out, true, ld, stride, stats);
    });
}

int32_t emus_bootscan_pair_counts_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts, const int64_t* ends, int64_t windows,
                                      int64_t replicates, uint64_t seed, int64_t lead, const fnn_dist_model* m, int32_t device, int64_t* F_out, int64_t ld,
                                      int64_t stride, fnn_scan_stats* stats) {
    return emup_try([&] {
        EmuScanBackend be;
        return fnn::dist_batch_scan(be, "emus_bootscan_pair_counts_i64", seq, n, L, lds, starts, ends, windows, replicates, seed, lead, m, true, device,
                                    reinterpret_cast<double*>(F_out), false, ld, stride, stats);
    });
}

int32_t emus_bootscan_pair_counts_device_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts, const int64_t* ends,
                                             int64_t windows, int64_t replicates, uint64_t seed, int64_t lead, const fnn_dist_model* m, int32_t device,
                                             int64_t* F_out, int64_t ld, int64_t stride, fnn_scan_stats* stats) {
    return emup_try([&] {
        EmuScanBackend be;
        return fnn::dist_batch_scan(be, "emus_bootscan_pair_counts_device_i64", seq, n, L, lds, starts, ends, windows, replicates, seed, lead, m, true, device,
                                    reinterpret_cast<double*>(F_out), true, ld, stride, stats);
    });
}

// The compact planes themselves: one launch of the draw over problems first ... first + count - 1 of the call, as the host logic
// lays out such a chunk.  plane_out: the chunk's compact rows back to back (row b: hi - lo bytes of its window); total_out: count;
// max_count_out: one word.  Returns the bytes of the planes through *bytes_out; plane_out may hold `capacity` bytes.
int32_t emus_bootscan_draw_planes(const int64_t* starts, const int64_t* ends, int64_t windows, int64_t replicates, int64_t lead, uint64_t seed, int64_t first,
                                  int64_t count, int32_t group_rows, int8_t* plane_out, int64_t capacity, int64_t* bytes_out, int64_t* total_out,
                                  uint32_t* max_count_out) {
    return emup_try([&]() -> int32_t {
        using namespace fnn;
        const int64_t P = replicates + lead;
        if (windows <= 0 || P <= 0 || first < 0 || count <= 0 || first + count > windows * P || group_rows < 1)
            return fail(FNN_EINVAL, "emus_bootscan_draw_planes: bad argument");
        EmuScanBackend be;
        std::vector<ScanWindow> wins;
        std::vector<ScanGroup> groups;
        int32_t span = 0;
        int64_t blocks = 0;
        const int64_t bytes = scan_chunk(starts, ends, P, seed, first, count, group_rows, wins, groups, &span, &blocks);
        *bytes_out = bytes;
        if (bytes > capacity) return fail(FNN_EINVAL, "emus_bootscan_draw_planes: the planes need more room");
        ScanArgs a{};
        a.planes = (int8_t*)be.alloc((size_t)bytes);
        ScanWindow* d_wins = (ScanWindow*)be.alloc(sizeof(ScanWindow) * wins.size());
        a.total = (int64_t*)be.alloc(sizeof(int64_t) * (size_t)count);
        a.bad = (int32_t*)be.alloc(sizeof(int32_t) * (size_t)count);
        a.sat = (int32_t*)be.alloc(sizeof(int32_t) * (size_t)count);
        a.max_count = (uint32_t*)be.alloc(sizeof(uint32_t));
        if (!a.planes || !d_wins || !a.total || !a.bad || !a.sat || !a.max_count) return fail(FNN_ENOMEM, "emus_bootscan_draw_planes: out of memory");
        std::memcpy(d_wins, wins.data(), sizeof(ScanWindow) * wins.size());
        a.windows = d_wins; a.first = first; a.per_window = P; a.lead = lead; a.cnt = count;
        *a.max_count = 0;
        double t = 0.0;
        if (be.run_draw_ranges(a, count, span, &t) != FNN_OK) return fail(FNN_EHIP, be.err());
        for (int64_t r = 0; r < count; r++)
            if (a.bad[r] != 0 || a.sat[r] != 0) return fail(FNN_ESTATE, "emus_bootscan_draw_planes: a flag was not zeroed");
        // (every group lies inside the planes and its rows are the chunk's rows in order)
        int64_t at = 0, row = 0;
        for (const ScanGroup& g : groups) {
            if (g.plane != at || g.row0 != row || g.rows < 1 || g.rows > group_rows) return fail(FNN_ESTATE, "emus_bootscan_draw_planes: a group is out of place");
            at += (int64_t)g.rows * (g.hi - g.lo);
            row += g.rows;
        }
        if (at != bytes || row != count) return fail(FNN_ESTATE, "emus_bootscan_draw_planes: the groups do not cover the chunk");
        std::memcpy(plane_out, a.planes, (size_t)bytes);
        std::memcpy(total_out, a.total, sizeof(int64_t) * (size_t)count);
        *max_count_out = *a.max_count;
        return FNN_OK;
    });
}

// the counts and bootstrap entries behind the same backend: what the bootscan entries are compared with
int32_t emus_alignment_distances_model_batch_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch, int64_t ldc,
                                                 const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                 fnn_dist_model_stats* stats) {
    return emup_try([&] {
        EmuScanBackend be;
        return fnn::dist_batch_model(be, "emus_alignment_distances_model_batch_f64", seq, n, L, lds, counts, batch, ldc, m, device, D_out, false, ld, stride,
                                     stats);
    });
}

int32_t emus_alignment_distances_model_batch_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch,
                                                        int64_t ldc, const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                        fnn_dist_model_stats* stats) {
    return emup_try([&] {
        EmuScanBackend be;
        return fnn::dist_batch_model(be, "emus_alignment_distances_model_batch_device_f64", seq, n, L, lds, counts, batch, ldc, m, device, D_out, true, ld,
                                     stride, stats);
    });
}

int32_t emus_alignment_pair_counts_batch_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch, int64_t ldc,
                                             int32_t device, int64_t* F_out, int64_t ld, int64_t stride, fnn_dist_model_stats* stats) {
    return emup_try([&] {
        EmuScanBackend be;
        return fnn::dist_batch_pair_counts(be, "emus_alignment_pair_counts_batch_i64", seq, n, L, lds, counts, batch, ldc, device, F_out, false, ld, stride,
                                           stats);
    });
}

int32_t emus_alignment_pair_counts_batch_device_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch,
                                                    int64_t ldc, int32_t device, int64_t* F_out, int64_t ld, int64_t stride, fnn_dist_model_stats* stats) {
    return emup_try([&] {
        EmuScanBackend be;
        return fnn::dist_batch_pair_counts(be, "emus_alignment_pair_counts_batch_device_i64", seq, n, L, lds, counts, batch, ldc, device, F_out, true, ld,
                                           stride, stats);
    });
}

int32_t emus_bootstrap_counts(int64_t L, int64_t batch, uint64_t seed, uint16_t* counts_out) {
    return emup_try([&] { return fnn::dist_bootstrap_counts("emus_bootstrap_counts", L, batch, seed, counts_out); });
}

int32_t emus_bootstrap_draw_max_sites(void) { return fnn::DRAW_MAX_SITES; }

int32_t emus_bootstrap_distances_batch_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, int64_t batch, uint64_t seed, int64_t lead,
                                           const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride, fnn_boot_stats* stats) {
    return emup_try([&] {
        EmuScanBackend be;
        return fnn::dist_bootstrap_batch(be, "emus_bootstrap_distances_batch_f64", seq, n, L, lds, batch, seed, lead, m, device, D_out, false, ld, stride,
                                         stats);
    });
}

int32_t emus_bootstrap_distances_batch_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, int64_t batch, uint64_t seed, int64_t lead,
                                                  const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                  fnn_boot_stats* stats) {
    return emup_try([&] {
        EmuScanBackend be;
        return fnn::dist_bootstrap_batch(be, "emus_bootstrap_distances_batch_device_f64", seq, n, L, lds, batch, seed, lead, m, device, D_out, true, ld,
                                         stride, stats);
    });
}

}  // extern "C"

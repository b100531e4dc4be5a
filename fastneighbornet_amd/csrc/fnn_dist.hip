// fnn_dist.hip -- p-distance matrices of bootstrap replicates from one alignment on the int8 matrix cores (the per-lane
// steps and the host side of the call are fnn_dist.h).
//
// k_dist<P, MISSING>: a workgroup is 4 waves; wave w takes pair tile 4 * (tile group) + w (taxon i against j0 ... j0 + 15)
// and the workgroup's 64 replicates as 4 tiles of 16.  Per 64 sites a lane loads 16 bytes of row i and of its row j, makes
// the 0/1 operand bytes in registers, loads 16 bytes of each digit plane of each of its 4 replicates and issues
// 4 x P (x 2 with MISSING) v_mfma_i32_16x16x64_i8.  No LDS, no atomics, no hand-over; vector stores and plain C++ only.
//
// k_draw (fnn_draw.h) makes the digit planes of a bootstrap on the device, one workgroup per row.
//
// k_dist_ranges, k_dist_ranges_pairs (fnn_dist_ranges.h): the same pair tiles against problems that are site
// ranges.  The B operand is made in registers from a range's two bounds and the walk covers the span of the wave's window tile.
//
// k_draw_ranges, k_dist_scan, k_dist_scan_pairs (fnn_scan.h): bootstrap replicates of every site range.  The
// draw writes one compact plane row per problem, as long as its window's span; a wave walks one window's span against one group of
// that window's rows.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "fnn_dist.h"
#include "fnn_ragged_hip.h"

namespace fnn {

// grid: (tile groups) x (replicate groups) workgroups in one dimension, the replicate group the slow index: workgroups
// that run at the same time read the same rows of the planes
template <int P, bool MISSING>
__global__ __launch_bounds__(DIST_THREADS) void k_dist(const DistArgs a, const uint32_t tile_groups) {
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const uint32_t rg = blockIdx.x / tile_groups, tg = blockIdx.x - rg * tile_groups;
    const DistTile t = a.tiles[(size_t)tg * DIST_WAVES + (size_t)wave];
    const int64_t b0 = (int64_t)rg * DIST_REPS;
    DistAcc am[DIST_RT][P], av[DIST_RT][MISSING ? P : 1];
    for (int rt = 0; rt < DIST_RT; rt++)
        for (int d = 0; d < P; d++) {
            am[rt][d] = DistAcc{{0, 0, 0, 0}};
            av[rt][MISSING ? d : 0] = DistAcc{{0, 0, 0, 0}};
        }
    for (int64_t s = 0; s < a.lpad; s += DIST_K) {
        DistFrag fm, fv;
        dist_lane_a<MISSING>(a, t, lane, s, fm, fv);
#pragma unroll
        for (int rt = 0; rt < DIST_RT; rt++)
#pragma unroll
            for (int d = 0; d < P; d++) {
                const DistFrag fb = dist_lane_b(a, b0, rt, d, lane, s);
                am[rt][d] = dist_mma(fm, fb, am[rt][d]);
                if (MISSING) av[rt][d] = dist_mma(fv, fb, av[rt][d]);
            }
    }
#pragma unroll
    for (int rt = 0; rt < DIST_RT; rt++) dist_lane_store<P, MISSING>(a, t, b0 + DIST_TILE * rt, lane, am[rt], av[rt]);
}

// k_dist_model<MODEL, P, MISSING, RT>: the same walk for a corrected distance, RT replicate tiles per
// wave (dist_model_rt; the grid's replicate groups hold 16 RT replicates).  JC69 differs from k_dist in the epilogue only; K2P
// makes the transition operand from the same two loads and keeps a third accumulator set: 4 x P x (2 or 3) instructions
// per 64 sites.  GAMMA: the epilogue reads the shape of gamma-distributed rates; without it the shape is the
// constant 0.0 there and the correction folds away: the equal-rates variants are the kernels they were.
template <int MODEL, int P, bool MISSING, int RT, bool GAMMA>
__global__ __launch_bounds__(DIST_THREADS) void k_dist_model(const DistArgs a, const DistModel dm_in, const uint32_t tile_groups) {
    constexpr bool K2P = MODEL == FNN_DIST_K2P;
    DistModel dm = dm_in;
    if (!GAMMA) dm.shape = 0.0;
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const uint32_t rg = blockIdx.x / tile_groups, tg = blockIdx.x - rg * tile_groups;
    const DistTile t = a.tiles[(size_t)tg * DIST_WAVES + (size_t)wave];
    const int64_t b0 = (int64_t)rg * (DIST_TILE * RT);
    DistAcc am[RT][P], av[RT][MISSING ? P : 1], at[RT][K2P ? P : 1];
    for (int rt = 0; rt < RT; rt++)
        for (int d = 0; d < P; d++) {
            am[rt][d] = DistAcc{{0, 0, 0, 0}};
            av[rt][MISSING ? d : 0] = DistAcc{{0, 0, 0, 0}};
            at[rt][K2P ? d : 0] = DistAcc{{0, 0, 0, 0}};
        }
    for (int64_t s = 0; s < a.lpad; s += DIST_K) {
        DistFrag fm, fv, ft;
        if (K2P) dist_lane_a_ts<MISSING>(a, t, lane, s, fm, fv, ft);
        else dist_lane_a<MISSING>(a, t, lane, s, fm, fv);
#pragma unroll
        for (int rt = 0; rt < RT; rt++)
#pragma unroll
            for (int d = 0; d < P; d++) {
                const DistFrag fb = dist_lane_b(a, b0, rt, d, lane, s);
                am[rt][d] = dist_mma(fm, fb, am[rt][d]);
                if (MISSING) av[rt][d] = dist_mma(fv, fb, av[rt][d]);
                if (K2P) at[rt][d] = dist_mma(ft, fb, at[rt][d]);
            }
    }
#pragma unroll
    for (int rt = 0; rt < RT; rt++) dist_lane_store_model<MODEL, P, MISSING>(a, dm, t, b0 + DIST_TILE * rt, lane, am[rt], av[rt], at[rt]);
}

// k_dist_pairs<MODEL, P, RT>: the same walk for the 4 x 4 table of state pairs (the steps are
// fnn_dist_pairs.h), RT replicate tiles per wave (dist_pairs_rt).  Sixteen 0/1 operands from the two loads, each against every
// digit plane: 16 x P x RT instructions per 64 sites.  MODEL: FNN_DIST_F81 ... FNN_DIST_LOGDET, or DIST_PAIR_COUNTS for the table.
// GAMMA: as k_dist_model's (F81, F84 and TN93 only).
template <int MODEL, int P, int RT, bool GAMMA>
__global__ __launch_bounds__(DIST_THREADS) void k_dist_pairs(const DistArgs a, const DistPairs dp_in, const uint32_t tile_groups) {
    DistPairs dp = dp_in;
    if (!GAMMA) dp.shape = 0.0;
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const uint32_t rg = blockIdx.x / tile_groups, tg = blockIdx.x - rg * tile_groups;
    const DistTile t = a.tiles[(size_t)tg * DIST_WAVES + (size_t)wave];
    const int64_t b0 = (int64_t)rg * (DIST_TILE * RT);
    DistAcc acc[RT][DIST_PAIR_CELLS][P];
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
        for (int c = 0; c < DIST_PAIR_CELLS; c++)
#pragma unroll
            for (int d = 0; d < P; d++) acc[rt][c][d] = DistAcc{{0, 0, 0, 0}};
    for (int64_t s = 0; s < a.lpad; s += DIST_K) {
        DistFrag f[DIST_PAIR_CELLS];
        dist_lane_a_pairs(a, t, lane, s, f);
#pragma unroll
        for (int rt = 0; rt < RT; rt++)
#pragma unroll
            for (int d = 0; d < P; d++) {
                const DistFrag fb = dist_lane_b(a, b0, rt, d, lane, s);
#pragma unroll
                for (int c = 0; c < DIST_PAIR_CELLS; c++) acc[rt][c][d] = dist_mma(f[c], fb, acc[rt][c][d]);
            }
    }
#pragma unroll
    for (int rt = 0; rt < RT; rt++) dist_lane_store_pairs<MODEL, P>(a, dp, t, b0 + DIST_TILE * rt, lane, acc[rt]);
}

// k_dist_ranges<MODEL, MISSING, GAMMA>: k_dist (MODEL = FNN_DIST_P) and k_dist_model for problems that are site ranges
// (the steps are fnn_dist_ranges.h).  A wave takes one pair tile and one window tile of 16 ranges (the
// grid's slow index is the window tile); a lane reads the bounds of its column once.  The walk covers the tile's span from the
// host's table, wave-uniform; per 64 sites a lane makes the A operands as the kernels above do and the 0/1 B operand from the
// bounds: no plane is loaded, one digit.  The epilogues are the ones above with P = 1.
template <int MODEL, bool MISSING, bool GAMMA>
__global__ __launch_bounds__(DIST_THREADS) void k_dist_ranges(const DistArgs a, const DistRanges dr, const DistModel dm_in, const uint32_t tile_groups) {
    constexpr bool K2P = MODEL == FNN_DIST_K2P;
    DistModel dm = dm_in;
    if (!GAMMA) dm.shape = 0.0;
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const uint32_t wt = blockIdx.x / tile_groups, tg = blockIdx.x - wt * tile_groups;
    const DistTile t = a.tiles[(size_t)tg * DIST_WAVES + (size_t)wave];
    const int64_t b0 = (int64_t)wt * DIST_TILE;
    const DistSpan sp = dr.spans[wt];
    const DistRangeLane rl = dist_lane_range(dr, b0, lane);
    DistAcc am[1] = {DistAcc{{0, 0, 0, 0}}}, av[1] = {DistAcc{{0, 0, 0, 0}}}, at[1] = {DistAcc{{0, 0, 0, 0}}};
    for (int32_t s = sp.lo; s < sp.hi; s += DIST_K) {
        DistFrag fm, fv, ft;
        if (K2P) dist_lane_a_ts<MISSING>(a, t, lane, s, fm, fv, ft);
        else dist_lane_a<MISSING>(a, t, lane, s, fm, fv);
        const DistFrag fb = dist_lane_b_range(rl, lane, s);
        am[0] = dist_mma(fm, fb, am[0]);
        if (MISSING) av[0] = dist_mma(fv, fb, av[0]);
        if (K2P) at[0] = dist_mma(ft, fb, at[0]);
    }
    if constexpr (MODEL == FNN_DIST_P) dist_lane_store<1, MISSING>(a, t, b0, lane, am, av);
    else dist_lane_store_model<MODEL, 1, MISSING>(a, dm, t, b0, lane, am, av, at);
}

// k_dist_ranges_pairs<MODEL, GAMMA>: k_dist_pairs for problems that are site ranges, in the same way.
template <int MODEL, bool GAMMA>
__global__ __launch_bounds__(DIST_THREADS) void k_dist_ranges_pairs(const DistArgs a, const DistRanges dr, const DistPairs dp_in, const uint32_t tile_groups) {
    DistPairs dp = dp_in;
    if (!GAMMA) dp.shape = 0.0;
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const uint32_t wt = blockIdx.x / tile_groups, tg = blockIdx.x - wt * tile_groups;
    const DistTile t = a.tiles[(size_t)tg * DIST_WAVES + (size_t)wave];
    const int64_t b0 = (int64_t)wt * DIST_TILE;
    const DistSpan sp = dr.spans[wt];
    const DistRangeLane rl = dist_lane_range(dr, b0, lane);
    DistAcc acc[DIST_PAIR_CELLS][1];
#pragma unroll
    for (int c = 0; c < DIST_PAIR_CELLS; c++) acc[c][0] = DistAcc{{0, 0, 0, 0}};
    for (int32_t s = sp.lo; s < sp.hi; s += DIST_K) {
        DistFrag f[DIST_PAIR_CELLS];
        dist_lane_a_pairs(a, t, lane, s, f);
        const DistFrag fb = dist_lane_b_range(rl, lane, s);
#pragma unroll
        for (int c = 0; c < DIST_PAIR_CELLS; c++) acc[c][0] = dist_mma(f[c], fb, acc[c][0]);
    }
    dist_lane_store_pairs<MODEL, 1>(a, dp, t, b0, lane, acc);
}

// k_draw: one workgroup makes one row of the digit planes of a bootstrap (the steps are fnn_draw.h).
// Dynamic LDS: the row's histogram, 2 * lpad bytes <= DRAW_LDS_BYTES.  grid: the chunk's padded rows.
__global__ __launch_bounds__(DRAW_THREADS) void k_draw(const DrawArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t draw_hist[];
    const int tid = (int)threadIdx.x;
    const int64_t row = (int64_t)blockIdx.x;
    uint32_t most = 0;
    if (row < a.cnt) {  // (uniform over the workgroup)
        draw_lane_zero(draw_hist, a.lpad, tid, DRAW_THREADS);
        __syncthreads();
        draw_lane_count(a, draw_hist, row, tid, DRAW_THREADS);
        __syncthreads();
        most = draw_lane_planes(a, draw_hist, row, tid, DRAW_THREADS);
    } else
        draw_lane_planes(a, nullptr, row, tid, DRAW_THREADS);
    draw_lane_row_words(a, row, tid);
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)most, off);
        most = o > most ? o : most;
    }
    if ((tid & 63) == 0 && most > 0) atomicMax(a.max_count, most);
}

// k_draw_ranges: one workgroup makes one compact row of a bootscan's plane (the steps are fnn_scan.h): k_draw
// over the span [lo, hi) of the row's window.  Dynamic LDS: the histogram of the chunk's widest span, 2 bytes per site
// <= DRAW_LDS_BYTES.  grid: the chunk's rows, all of them problems.
__global__ __launch_bounds__(DRAW_THREADS) void k_draw_ranges(const ScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t scan_hist[];
    const int tid = (int)threadIdx.x;
    const int64_t row = (int64_t)blockIdx.x;
    const ScanWindow w = scan_row_window(a, row);
    draw_lane_zero(scan_hist, w.hi - w.lo, tid, DRAW_THREADS);
    __syncthreads();
    scan_lane_count(a, w, scan_hist, row, tid, DRAW_THREADS);
    __syncthreads();
    uint32_t most = scan_lane_plane(a, w, scan_hist, row, tid, DRAW_THREADS);
    scan_lane_row_words(a, w, row, tid);
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)most, off);
        most = o > most ? o : most;
    }
    if ((tid & 63) == 0 && most > 0) atomicMax(a.max_count, most);
}

// k_dist_scan<MODEL, MISSING, GAMMA>: k_dist (MODEL = FNN_DIST_P) and k_dist_model for a bootscan (the steps
// are fnn_scan.h).  A wave takes one pair tile and one column group - up to DIST_RT tiles of 16 rows of ONE window (the grid's slow
// index is the group) - and walks that window's span, wave-uniform; per 64 sites a lane makes the A operands as the kernels above
// do and loads 16 bytes of its column's compact row at s - lo for each tile the group has.  One digit; the epilogues are the ones
// above with P = 1, bounded by the group's last row.
template <int MODEL, bool MISSING, bool GAMMA>
__global__ __launch_bounds__(DIST_THREADS) void k_dist_scan(const DistArgs a, const ScanArgs sa, const DistModel dm_in, const uint32_t tile_groups) {
    constexpr bool K2P = MODEL == FNN_DIST_K2P;
    DistModel dm = dm_in;
    if (!GAMMA) dm.shape = 0.0;
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const uint32_t cg = blockIdx.x / tile_groups, tg = blockIdx.x - cg * tile_groups;
    const DistTile t = a.tiles[(size_t)tg * DIST_WAVES + (size_t)wave];
    const ScanGroup g = sa.groups[cg];
    const int8_t* rows[DIST_RT];
    DistAcc am[DIST_RT][1], av[DIST_RT][1], at[DIST_RT][1];
#pragma unroll
    for (int rt = 0; rt < DIST_RT; rt++) {
        rows[rt] = scan_lane_row(sa, g, rt, lane);
        am[rt][0] = DistAcc{{0, 0, 0, 0}};
        av[rt][0] = DistAcc{{0, 0, 0, 0}};
        at[rt][0] = DistAcc{{0, 0, 0, 0}};
    }
    for (int32_t s = g.lo; s < g.hi; s += DIST_K) {
        DistFrag fm, fv, ft;
        if (K2P) dist_lane_a_ts<MISSING>(a, t, lane, s, fm, fv, ft);
        else dist_lane_a<MISSING>(a, t, lane, s, fm, fv);
#pragma unroll
        for (int rt = 0; rt < DIST_RT; rt++) {
            if (DIST_TILE * rt >= g.rows) continue;  // (uniform over the wave)
            const DistFrag fb = scan_lane_b(rows[rt], g, s);
            am[rt][0] = dist_mma(fm, fb, am[rt][0]);
            if (MISSING) av[rt][0] = dist_mma(fv, fb, av[rt][0]);
            if (K2P) at[rt][0] = dist_mma(ft, fb, at[rt][0]);
        }
    }
    const DistArgs al = scan_group_args(a, g);
#pragma unroll
    for (int rt = 0; rt < DIST_RT; rt++) {
        if constexpr (MODEL == FNN_DIST_P) dist_lane_store<1, MISSING>(al, t, (int64_t)g.row0 + DIST_TILE * rt, lane, am[rt], av[rt]);
        else dist_lane_store_model<MODEL, 1, MISSING>(al, dm, t, (int64_t)g.row0 + DIST_TILE * rt, lane, am[rt], av[rt], at[rt]);
    }
}

// k_dist_scan_pairs<MODEL, GAMMA>: k_dist_pairs for a bootscan, in the same way; a column group is dist_pairs_rt(1) tiles.
template <int MODEL, bool GAMMA>
__global__ __launch_bounds__(DIST_THREADS) void k_dist_scan_pairs(const DistArgs a, const ScanArgs sa, const DistPairs dp_in, const uint32_t tile_groups) {
    constexpr int RT = dist_pairs_rt(1);
    DistPairs dp = dp_in;
    if (!GAMMA) dp.shape = 0.0;
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const uint32_t cg = blockIdx.x / tile_groups, tg = blockIdx.x - cg * tile_groups;
    const DistTile t = a.tiles[(size_t)tg * DIST_WAVES + (size_t)wave];
    const ScanGroup g = sa.groups[cg];
    const int8_t* rows[RT];
    DistAcc acc[RT][DIST_PAIR_CELLS][1];
#pragma unroll
    for (int rt = 0; rt < RT; rt++) {
        rows[rt] = scan_lane_row(sa, g, rt, lane);
#pragma unroll
        for (int c = 0; c < DIST_PAIR_CELLS; c++) acc[rt][c][0] = DistAcc{{0, 0, 0, 0}};
    }
    for (int32_t s = g.lo; s < g.hi; s += DIST_K) {
        DistFrag f[DIST_PAIR_CELLS];
        dist_lane_a_pairs(a, t, lane, s, f);
#pragma unroll
        for (int rt = 0; rt < RT; rt++) {
            if (DIST_TILE * rt >= g.rows) continue;  // (uniform over the wave)
            const DistFrag fb = scan_lane_b(rows[rt], g, s);
#pragma unroll
            for (int c = 0; c < DIST_PAIR_CELLS; c++) acc[rt][c][0] = dist_mma(f[c], fb, acc[rt][c][0]);
        }
    }
    const DistArgs al = scan_group_args(a, g);
#pragma unroll
    for (int rt = 0; rt < RT; rt++) dist_lane_store_pairs<MODEL, 1>(al, dp, t, (int64_t)g.row0 + DIST_TILE * rt, lane, acc[rt]);
}

struct DistHipBackend : HipBatchBase {
    int32_t run_draw(const DrawArgs& a, int64_t rows, double* t_draw_s) {
        const int32_t lds_bytes = draw_lds_bytes(a.lpad);
        if (lds_bytes > DRAW_LDS_BYTES || rows >= ((int64_t)1 << 31)) { last = "too many sites or rows for the draw kernel"; return FNN_EHIP; }
        return timed_launch(reinterpret_cast<const void*>(&k_draw), "k_draw", lds_bytes, [&] {
            hipLaunchKernelGGL(k_draw, dim3((unsigned)rows), dim3(DRAW_THREADS), (size_t)lds_bytes, stream, a);
        }, t_draw_s);
    }
    template <int MODEL, int P, bool MISSING, bool GAMMA>
    int32_t launch_model_rates(const DistArgs& a, const DistModel& dm, int64_t tile_groups, int64_t cnt, double* t_kernel_s) {
        constexpr int RT = dist_model_rt(MODEL, P, MISSING);
        const int64_t rep_groups = round_up(cnt, (int64_t)(DIST_TILE * RT)) / (DIST_TILE * RT);
        if (tile_groups * rep_groups >= ((int64_t)1 << 31)) { last = "too many workgroups for one launch"; return FNN_EHIP; }
        return timed_launch(reinterpret_cast<const void*>(&k_dist_model<MODEL, P, MISSING, RT, GAMMA>), "k_dist_model", 0, [&] {
            hipLaunchKernelGGL((k_dist_model<MODEL, P, MISSING, RT, GAMMA>), dim3((unsigned)(tile_groups * rep_groups)), dim3(DIST_THREADS), 0, stream, a,
                               dm, (uint32_t)tile_groups);
        }, t_kernel_s);
    }
    template <int MODEL, int P, bool MISSING>
    int32_t launch_model(const DistArgs& a, const DistModel& dm, int64_t tile_groups, int64_t cnt, double* t_kernel_s) {
        return dm.shape != 0.0 ? launch_model_rates<MODEL, P, MISSING, true>(a, dm, tile_groups, cnt, t_kernel_s)
                               : launch_model_rates<MODEL, P, MISSING, false>(a, dm, tile_groups, cnt, t_kernel_s);
    }
    template <int MODEL>
    int32_t run_model_of(int32_t P, bool missing, const DistArgs& a, const DistModel& dm, int64_t tile_groups, int64_t cnt, double* t_kernel_s) {
        switch (P * 2 + (missing ? 1 : 0)) {
            case 2: return launch_model<MODEL, 1, false>(a, dm, tile_groups, cnt, t_kernel_s);
            case 3: return launch_model<MODEL, 1, true>(a, dm, tile_groups, cnt, t_kernel_s);
            case 4: return launch_model<MODEL, 2, false>(a, dm, tile_groups, cnt, t_kernel_s);
            case 5: return launch_model<MODEL, 2, true>(a, dm, tile_groups, cnt, t_kernel_s);
            case 6: return launch_model<MODEL, 3, false>(a, dm, tile_groups, cnt, t_kernel_s);
            case 7: return launch_model<MODEL, 3, true>(a, dm, tile_groups, cnt, t_kernel_s);
        }
        last = "no kernel for " + std::to_string(P) + " digits";
        return FNN_EHIP;
    }
    int32_t run_model(int32_t model, int32_t P, bool missing, const DistArgs& a, const DistModel& dm, int64_t tile_groups, int64_t cnt, double* t_kernel_s) {
        if (model == FNN_DIST_JC69) return run_model_of<FNN_DIST_JC69>(P, missing, a, dm, tile_groups, cnt, t_kernel_s);
        if (model == FNN_DIST_K2P) return run_model_of<FNN_DIST_K2P>(P, missing, a, dm, tile_groups, cnt, t_kernel_s);
        last = "no kernel for model " + std::to_string(model);
        return FNN_EHIP;
    }
    template <int MODEL, int P, bool GAMMA>
    int32_t launch_pairs_rates(const DistArgs& a, const DistPairs& dp, int64_t tile_groups, int64_t cnt, double* t_kernel_s) {
        constexpr int RT = dist_pairs_rt(P);
        const int64_t rep_groups = round_up(cnt, (int64_t)(DIST_TILE * RT)) / (DIST_TILE * RT);
        if (tile_groups * rep_groups >= ((int64_t)1 << 31)) { last = "too many workgroups for one launch"; return FNN_EHIP; }
        return timed_launch(reinterpret_cast<const void*>(&k_dist_pairs<MODEL, P, RT, GAMMA>), "k_dist_pairs", 0, [&] {
            hipLaunchKernelGGL((k_dist_pairs<MODEL, P, RT, GAMMA>), dim3((unsigned)(tile_groups * rep_groups)), dim3(DIST_THREADS), 0, stream, a, dp,
                               (uint32_t)tile_groups);
        }, t_kernel_s);
    }
    template <int MODEL, int P>
    int32_t launch_pairs(const DistArgs& a, const DistPairs& dp, int64_t tile_groups, int64_t cnt, double* t_kernel_s) {
        if constexpr (MODEL == FNN_DIST_F81 || MODEL == FNN_DIST_F84 || MODEL == FNN_DIST_TN93) {  // (the models with a gamma form)
            if (dp.shape != 0.0) return launch_pairs_rates<MODEL, P, true>(a, dp, tile_groups, cnt, t_kernel_s);
        }
        return launch_pairs_rates<MODEL, P, false>(a, dp, tile_groups, cnt, t_kernel_s);
    }
    template <int MODEL>
    int32_t run_pairs_of(int32_t P, const DistArgs& a, const DistPairs& dp, int64_t tile_groups, int64_t cnt, double* t_kernel_s) {
        switch (P) {
            case 1: return launch_pairs<MODEL, 1>(a, dp, tile_groups, cnt, t_kernel_s);
            case 2: return launch_pairs<MODEL, 2>(a, dp, tile_groups, cnt, t_kernel_s);
            case 3: return launch_pairs<MODEL, 3>(a, dp, tile_groups, cnt, t_kernel_s);
        }
        last = "no kernel for " + std::to_string(P) + " digits";
        return FNN_EHIP;
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
    // ---- site ranges: window tiles of 16 problems in place of replicate groups
    template <int MODEL, bool MISSING, bool GAMMA>
    int32_t launch_ranges(const DistArgs& a, const DistRanges& dr, const DistModel& dm, int64_t tile_groups, int64_t cnt, double* t_kernel_s) {
        const int64_t win_tiles = round_up(cnt, (int64_t)DIST_TILE) / DIST_TILE;
        if (tile_groups * win_tiles >= ((int64_t)1 << 31)) { last = "too many workgroups for one launch"; return FNN_EHIP; }
        return timed_launch(reinterpret_cast<const void*>(&k_dist_ranges<MODEL, MISSING, GAMMA>), "k_dist_ranges", 0, [&] {
            hipLaunchKernelGGL((k_dist_ranges<MODEL, MISSING, GAMMA>), dim3((unsigned)(tile_groups * win_tiles)), dim3(DIST_THREADS), 0, stream, a, dr, dm,
                               (uint32_t)tile_groups);
        }, t_kernel_s);
    }
    template <int MODEL>
    int32_t run_ranges_of(bool missing, const DistArgs& a, const DistRanges& dr, const DistModel& dm, int64_t tile_groups, int64_t cnt, double* t_kernel_s) {
        if constexpr (MODEL != FNN_DIST_P) {  // (the models with a gamma form)
            if (dm.shape != 0.0)
                return missing ? launch_ranges<MODEL, true, true>(a, dr, dm, tile_groups, cnt, t_kernel_s)
                               : launch_ranges<MODEL, false, true>(a, dr, dm, tile_groups, cnt, t_kernel_s);
        }
        return missing ? launch_ranges<MODEL, true, false>(a, dr, dm, tile_groups, cnt, t_kernel_s)
                       : launch_ranges<MODEL, false, false>(a, dr, dm, tile_groups, cnt, t_kernel_s);
    }
    int32_t run_ranges(int32_t model, bool missing, const DistArgs& a, const DistRanges& dr, const DistModel& dm, int64_t tile_groups, int64_t cnt,
                       double* t_kernel_s) {
        if (model == FNN_DIST_P) return run_ranges_of<FNN_DIST_P>(missing, a, dr, dm, tile_groups, cnt, t_kernel_s);
        if (model == FNN_DIST_JC69) return run_ranges_of<FNN_DIST_JC69>(missing, a, dr, dm, tile_groups, cnt, t_kernel_s);
        if (model == FNN_DIST_K2P) return run_ranges_of<FNN_DIST_K2P>(missing, a, dr, dm, tile_groups, cnt, t_kernel_s);
        last = "no kernel for model " + std::to_string(model);
        return FNN_EHIP;
    }
    template <int MODEL, bool GAMMA>
    int32_t launch_ranges_pairs(const DistArgs& a, const DistRanges& dr, const DistPairs& dp, int64_t tile_groups, int64_t cnt, double* t_kernel_s) {
        const int64_t win_tiles = round_up(cnt, (int64_t)DIST_TILE) / DIST_TILE;
        if (tile_groups * win_tiles >= ((int64_t)1 << 31)) { last = "too many workgroups for one launch"; return FNN_EHIP; }
        return timed_launch(reinterpret_cast<const void*>(&k_dist_ranges_pairs<MODEL, GAMMA>), "k_dist_ranges_pairs", 0, [&] {
            hipLaunchKernelGGL((k_dist_ranges_pairs<MODEL, GAMMA>), dim3((unsigned)(tile_groups * win_tiles)), dim3(DIST_THREADS), 0, stream, a, dr, dp,
                               (uint32_t)tile_groups);
        }, t_kernel_s);
    }
    template <int MODEL>
    int32_t run_ranges_pairs_of(const DistArgs& a, const DistRanges& dr, const DistPairs& dp, int64_t tile_groups, int64_t cnt, double* t_kernel_s) {
        if constexpr (MODEL == FNN_DIST_F81 || MODEL == FNN_DIST_F84 || MODEL == FNN_DIST_TN93) {  // (the models with a gamma form)
            if (dp.shape != 0.0) return launch_ranges_pairs<MODEL, true>(a, dr, dp, tile_groups, cnt, t_kernel_s);
        }
        return launch_ranges_pairs<MODEL, false>(a, dr, dp, tile_groups, cnt, t_kernel_s);
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
    // ---- bootscan: column groups of one window's rows in place of replicate groups
    int32_t run_draw_ranges(const ScanArgs& a, int64_t rows, int32_t span, double* t_draw_s) {
        const int32_t lds_bytes = draw_lds_bytes(span);
        if (lds_bytes > DRAW_LDS_BYTES || rows >= ((int64_t)1 << 31)) { last = "too many sites or rows for the draw kernel"; return FNN_EHIP; }
        return timed_launch(reinterpret_cast<const void*>(&k_draw_ranges), "k_draw_ranges", lds_bytes, [&] {
            hipLaunchKernelGGL(k_draw_ranges, dim3((unsigned)rows), dim3(DRAW_THREADS), (size_t)lds_bytes, stream, a);
        }, t_draw_s);
    }
    template <int MODEL, bool MISSING, bool GAMMA>
    int32_t launch_scan(const DistArgs& a, const ScanArgs& sa, const DistModel& dm, int64_t tile_groups, int64_t groups, double* t_kernel_s) {
        if (tile_groups * groups >= ((int64_t)1 << 31)) { last = "too many workgroups for one launch"; return FNN_EHIP; }
        return timed_launch(reinterpret_cast<const void*>(&k_dist_scan<MODEL, MISSING, GAMMA>), "k_dist_scan", 0, [&] {
            hipLaunchKernelGGL((k_dist_scan<MODEL, MISSING, GAMMA>), dim3((unsigned)(tile_groups * groups)), dim3(DIST_THREADS), 0, stream, a, sa, dm,
                               (uint32_t)tile_groups);
        }, t_kernel_s);
    }
    template <int MODEL>
    int32_t run_scan_of(bool missing, const DistArgs& a, const ScanArgs& sa, const DistModel& dm, int64_t tile_groups, int64_t groups, double* t_kernel_s) {
        if constexpr (MODEL != FNN_DIST_P) {  // (the models with a gamma form)
            if (dm.shape != 0.0)
                return missing ? launch_scan<MODEL, true, true>(a, sa, dm, tile_groups, groups, t_kernel_s)
                               : launch_scan<MODEL, false, true>(a, sa, dm, tile_groups, groups, t_kernel_s);
        }
        return missing ? launch_scan<MODEL, true, false>(a, sa, dm, tile_groups, groups, t_kernel_s)
                       : launch_scan<MODEL, false, false>(a, sa, dm, tile_groups, groups, t_kernel_s);
    }
    int32_t run_scan(int32_t model, bool missing, const DistArgs& a, const ScanArgs& sa, const DistModel& dm, int64_t tile_groups, int64_t groups,
                     double* t_kernel_s) {
        if (model == FNN_DIST_P) return run_scan_of<FNN_DIST_P>(missing, a, sa, dm, tile_groups, groups, t_kernel_s);
        if (model == FNN_DIST_JC69) return run_scan_of<FNN_DIST_JC69>(missing, a, sa, dm, tile_groups, groups, t_kernel_s);
        if (model == FNN_DIST_K2P) return run_scan_of<FNN_DIST_K2P>(missing, a, sa, dm, tile_groups, groups, t_kernel_s);
        last = "no kernel for model " + std::to_string(model);
        return FNN_EHIP;
    }
    template <int MODEL, bool GAMMA>
    int32_t launch_scan_pairs(const DistArgs& a, const ScanArgs& sa, const DistPairs& dp, int64_t tile_groups, int64_t groups, double* t_kernel_s) {
        if (tile_groups * groups >= ((int64_t)1 << 31)) { last = "too many workgroups for one launch"; return FNN_EHIP; }
        return timed_launch(reinterpret_cast<const void*>(&k_dist_scan_pairs<MODEL, GAMMA>), "k_dist_scan_pairs", 0, [&] {
            hipLaunchKernelGGL((k_dist_scan_pairs<MODEL, GAMMA>), dim3((unsigned)(tile_groups * groups)), dim3(DIST_THREADS), 0, stream, a, sa, dp,
                               (uint32_t)tile_groups);
        }, t_kernel_s);
    }
    template <int MODEL>
    int32_t run_scan_pairs_of(const DistArgs& a, const ScanArgs& sa, const DistPairs& dp, int64_t tile_groups, int64_t groups, double* t_kernel_s) {
        if constexpr (MODEL == FNN_DIST_F81 || MODEL == FNN_DIST_F84 || MODEL == FNN_DIST_TN93) {  // (the models with a gamma form)
            if (dp.shape != 0.0) return launch_scan_pairs<MODEL, true>(a, sa, dp, tile_groups, groups, t_kernel_s);
        }
        return launch_scan_pairs<MODEL, false>(a, sa, dp, tile_groups, groups, t_kernel_s);
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
    template <int P, bool MISSING>
    int32_t launch(const DistArgs& a, int64_t tile_groups, int64_t rep_groups, double* t_kernel_s) {
        return timed_launch(reinterpret_cast<const void*>(&k_dist<P, MISSING>), "k_dist", 0, [&] {
            hipLaunchKernelGGL((k_dist<P, MISSING>), dim3((unsigned)(tile_groups * rep_groups)), dim3(DIST_THREADS), 0, stream, a, (uint32_t)tile_groups);
        }, t_kernel_s);
    }
    int32_t run(int32_t P, bool missing, const DistArgs& a, int64_t tile_groups, int64_t rep_groups, double* t_kernel_s) {
        if (tile_groups * rep_groups >= ((int64_t)1 << 31)) { last = "too many workgroups for one launch"; return FNN_EHIP; }
        switch (P * 2 + (missing ? 1 : 0)) {
            case 2: return launch<1, false>(a, tile_groups, rep_groups, t_kernel_s);
            case 3: return launch<1, true>(a, tile_groups, rep_groups, t_kernel_s);
            case 4: return launch<2, false>(a, tile_groups, rep_groups, t_kernel_s);
            case 5: return launch<2, true>(a, tile_groups, rep_groups, t_kernel_s);
            case 6: return launch<3, false>(a, tile_groups, rep_groups, t_kernel_s);
            case 7: return launch<3, true>(a, tile_groups, rep_groups, t_kernel_s);
        }
        last = "no kernel for " + std::to_string(P) + " digits";
        return FNN_EHIP;
    }
};

}  // namespace fnn

extern "C" {

int32_t fnn_alignment_distances_batch_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch, int64_t ldc,
                                          int32_t model, int32_t device, double* D_out, int64_t ld, int64_t stride, fnn_dist_stats* stats) {
    FNN_BATCH_TRY(
        fnn::DistHipBackend be;
        return fnn::dist_batch(be, "fnn_alignment_distances_batch_f64", seq, n, L, lds, counts, batch, ldc, model, device, D_out, false, ld, stride, stats);
    )
}

int32_t fnn_alignment_distances_batch_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch,
                                                 int64_t ldc, int32_t model, int32_t device, double* d_D_out, int64_t ld, int64_t stride,
                                                 fnn_dist_stats* stats) {
    FNN_BATCH_TRY(
        fnn::DistHipBackend be;
        return fnn::dist_batch(be, "fnn_alignment_distances_batch_device_f64", seq, n, L, lds, counts, batch, ldc, model, device, d_D_out, true, ld, stride, stats);
    )
}

int32_t fnn_alignment_distances_model_batch_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch,
                                                int64_t ldc, const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                fnn_dist_model_stats* stats) {
    FNN_BATCH_TRY(
        fnn::DistHipBackend be;
        return fnn::dist_batch_model(be, "fnn_alignment_distances_model_batch_f64", seq, n, L, lds, counts, batch, ldc, m, device, D_out, false, ld, stride,
                                     stats);
    )
}

int32_t fnn_alignment_distances_model_batch_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch,
                                                       int64_t ldc, const fnn_dist_model* m, int32_t device, double* d_D_out, int64_t ld, int64_t stride,
                                                       fnn_dist_model_stats* stats) {
    FNN_BATCH_TRY(
        fnn::DistHipBackend be;
        return fnn::dist_batch_model(be, "fnn_alignment_distances_model_batch_device_f64", seq, n, L, lds, counts, batch, ldc, m, device, d_D_out, true, ld,
                                     stride, stats);
    )
}

int32_t fnn_alignment_pair_counts_batch_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch, int64_t ldc,
                                            int32_t device, int64_t* F_out, int64_t ld, int64_t stride, fnn_dist_model_stats* stats) {
    FNN_BATCH_TRY(
        fnn::DistHipBackend be;
        return fnn::dist_batch_pair_counts(be, "fnn_alignment_pair_counts_batch_i64", seq, n, L, lds, counts, batch, ldc, device, F_out, false, ld, stride, stats);
    )
}

int32_t fnn_alignment_pair_counts_batch_device_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch,
                                                   int64_t ldc, int32_t device, int64_t* d_F_out, int64_t ld, int64_t stride,
                                                   fnn_dist_model_stats* stats) {
    FNN_BATCH_TRY(
        fnn::DistHipBackend be;
        return fnn::dist_batch_pair_counts(be, "fnn_alignment_pair_counts_batch_device_i64", seq, n, L, lds, counts, batch, ldc, device, d_F_out, true, ld,
                                           stride, stats);
    )
}

int32_t fnn_bootstrap_counts(int64_t L,int64_t batch, uint64_t seed, uint16_t* counts_out) {
    FNN_BATCH_TRY(return fnn::dist_bootstrap_counts("fnn_bootstrap_counts", L, batch, seed, counts_out);)
}

int32_t fnn_bootstrap_distances_batch_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, int64_t batch, uint64_t seed, int64_t lead,
                                          const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride, fnn_boot_stats* stats) {
    FNN_BATCH_TRY(
        fnn::DistHipBackend be;
        return fnn::dist_bootstrap_batch(be, "fnn_bootstrap_distances_batch_f64", seq, n, L, lds, batch, seed, lead, m, device, D_out, false, ld, stride, stats);
    )
}

int32_t fnn_bootstrap_distances_batch_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, int64_t batch, uint64_t seed, int64_t lead,
                                                 const fnn_dist_model* m, int32_t device, double* d_D_out, int64_t ld, int64_t stride,
                                                 fnn_boot_stats* stats) {
    FNN_BATCH_TRY(
        fnn::DistHipBackend be;
        return fnn::dist_bootstrap_batch(be, "fnn_bootstrap_distances_batch_device_f64", seq, n, L, lds, batch, seed, lead, m, device, d_D_out, true, ld,
                                         stride, stats);
    )
}

int32_t fnn_bootstrap_draw_max_sites(void) { return fnn::DRAW_MAX_SITES; }

int32_t fnn_alignment_distances_ranges_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts, const int64_t* ends, int64_t batch,
                                           const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride, fnn_range_stats* stats) {
    FNN_BATCH_TRY(
        fnn::DistHipBackend be;
        return fnn::dist_batch_ranges(be, "fnn_alignment_distances_ranges_f64", seq, n, L, lds, starts, ends, batch, m, false, device, D_out, false, ld, stride,
                                      stats);
    )
}

int32_t fnn_alignment_distances_ranges_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts, const int64_t* ends,
                                                  int64_t batch, const fnn_dist_model* m, int32_t device, double* d_D_out, int64_t ld, int64_t stride,
                                                  fnn_range_stats* stats) {
    FNN_BATCH_TRY(
        fnn::DistHipBackend be;
        return fnn::dist_batch_ranges(be, "fnn_alignment_distances_ranges_device_f64", seq, n, L, lds, starts, ends, batch, m, false, device, d_D_out, true, ld,
                                      stride, stats);
    )
}

int32_t fnn_alignment_pair_counts_ranges_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts, const int64_t* ends, int64_t batch,
                                             int32_t device, int64_t* F_out, int64_t ld, int64_t stride, fnn_range_stats* stats) {
    FNN_BATCH_TRY(
        fnn::DistHipBackend be;
        return fnn::dist_batch_ranges(be, "fnn_alignment_pair_counts_ranges_i64", seq, n, L, lds, starts, ends, batch, nullptr, true, device,
                                      reinterpret_cast<double*>(F_out), false, ld, stride, stats);
    )
}

int32_t fnn_alignment_pair_counts_ranges_device_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts, const int64_t* ends,
                                                    int64_t batch, int32_t device, int64_t* d_F_out, int64_t ld, int64_t stride, fnn_range_stats* stats) {
    FNN_BATCH_TRY(
        fnn::DistHipBackend be;
        return fnn::dist_batch_ranges(be, "fnn_alignment_pair_counts_ranges_device_i64", seq, n, L, lds, starts, ends, batch, nullptr, true, device,
                                      reinterpret_cast<double*>(d_F_out), true, ld, stride, stats);
    )
}

int32_t fnn_bootscan_counts(int64_t L, const int64_t* starts, const int64_t* ends, int64_t windows, int64_t replicates, int64_t lead, uint64_t seed,
                            int64_t first, int64_t count, uint16_t* counts_out) {
    FNN_BATCH_TRY(return fnn::dist_bootscan_counts("fnn_bootscan_counts", L, starts, ends, windows, replicates, lead, seed, first, count, counts_out);)
}

int32_t fnn_bootscan_distances_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts, const int64_t* ends, int64_t windows,
                                   int64_t replicates, uint64_t seed, int64_t lead, const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld,
                                   int64_t stride, fnn_scan_stats* stats) {
    FNN_BATCH_TRY(
        fnn::DistHipBackend be;
        return fnn::dist_batch_scan(be, "fnn_bootscan_distances_f64", seq, n, L, lds, starts, ends, windows, replicates, seed, lead, m, false, device, D_out,
                                    false, ld, stride, stats);
    )
}

int32_t fnn_bootscan_distances_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts, const int64_t* ends, int64_t windows,
                                          int64_t replicates, uint64_t seed, int64_t lead, const fnn_dist_model* m, int32_t device, double* d_D_out,
                                          int64_t ld, int64_t stride, fnn_scan_stats* stats) {
    FNN_BATCH_TRY(
        fnn::DistHipBackend be;
        return fnn::dist_batch_scan(be, "fnn_bootscan_distances_device_f64", seq, n, L, lds, starts, ends, windows, replicates, seed, lead, m, false, device,
                                    d_D_out, true, ld, stride, stats);
    )
}

int32_t fnn_bootscan_pair_counts_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts, const int64_t* ends, int64_t windows,
                                     int64_t replicates, uint64_t seed, int64_t lead, const fnn_dist_model* m, int32_t device, int64_t* F_out, int64_t ld,
                                     int64_t stride, fnn_scan_stats* stats) {
    FNN_BATCH_TRY(
        fnn::DistHipBackend be;
        return fnn::dist_batch_scan(be, "fnn_bootscan_pair_counts_i64", seq, n, L, lds, starts, ends, windows, replicates, seed, lead, m, true, device,
                                    reinterpret_cast<double*>(F_out), false, ld, stride, stats);
    )
}

int32_t fnn_bootscan_pair_counts_device_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts, const int64_t* ends,
                                            int64_t windows, int64_t replicates, uint64_t seed, int64_t lead, const fnn_dist_model* m, int32_t device,
                                            int64_t* d_F_out, int64_t ld, int64_t stride, fnn_scan_stats* stats) {
    FNN_BATCH_TRY(
        fnn::DistHipBackend be;
        return fnn::dist_batch_scan(be, "fnn_bootscan_pair_counts_device_i64", seq, n, L, lds, starts, ends, windows, replicates, seed, lead, m, true, device,
                                    reinterpret_cast<double*>(d_F_out), true, ld, stride, stats);
    )
}

}  // extern "C"

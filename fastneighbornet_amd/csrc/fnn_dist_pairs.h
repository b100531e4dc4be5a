// fnn_dist_pairs.h -- the 4 x 4 table of state pairs of every (b, i, j) on the int8 matrix cores: the
// per-lane steps of k_dist_pairs (fnn_dist.hip), shared with the CPU driver (tests/emu/fnn_dist_pairs_emu.cpp).  Included by
// fnn_dist.h, whose walk, lane maps, digit planes and host side it uses.
//
// The alignment is in K2P's codes (A 0, C 1, G 2, T 3, 255 missing).  Operand (s, t) of a lane is the 0/1 byte "row i shows s
// and row j shows t", sixteen fragments from the same two 16-byte loads as k_dist_model's; each is multiplied with every digit
// plane, so a replicate tile holds 16 x P accumulator sets.  255 matches no code: a pair's valid count is the sum of its table
// and the kernel has no MISSING variant.  What a lane does with the exact table is fnn_dist_model.h.
#ifndef FNN_DIST_PAIRS_H
#define FNN_DIST_PAIRS_H

namespace fnn {

constexpr int32_t DIST_PAIR_CELLS = 16;
constexpr int32_t DIST_PAIR_COUNTS = 100;  // MODEL of k_dist_pairs that stores the table itself (not a value of fnn_dist_model.model)

// what k_dist_pairs needs beyond DistArgs
struct DistPairs {
    double sat_value;        // stored for a saturated pair: the cap, or +inf when the call is going to fail
    double deg_value;        // stored for a degenerate pair: the cap, or -inf when the call is going to fail
    int32_t* sat;            // sat[b] = 1: some pair of replicate b is saturated or degenerate (written like bad[])
    double shape;            // 0.0: equal rates; alpha > 0: gamma-distributed rates (F81, F84, TN93)
};
// replicate tiles per wave: 64 P RT accumulator registers beside the sixteen operand fragments (DESIGN.md section 18 has the
// register table)
constexpr int32_t dist_pairs_rt(int32_t P) { return P == 1 ? 2 : 1; }
constexpr bool dist_is_pair_model(int32_t model) { return model >= FNN_DIST_F81 && model <= FNN_DIST_LOGDET; }

// the sixteen operands of one lane from its 16 bytes of row i and of row j.  Per byte of a word x in codes: bit 0 and bit 1
// pick the code, and bit 7 tells 255 (whose low bits read as code 3) from a code.
FNN_HD void dist_code_bytes(uint32_t x, uint32_t* e) {
    const uint32_t M = 0x01010101u;
    const uint32_t lo = x & M, hi = (x >> 1) & M, present = ((x >> 7) & M) ^ M;
    const uint32_t nlo = lo ^ M, nhi = hi ^ M;
    e[0] = nlo & nhi;
    e[1] = lo & nhi;
    e[2] = nlo & hi;
    e[3] = lo & hi & present;
}
FNN_HD void dist_pair_frags(const DistFrag& ri, const DistFrag& rj, DistFrag* f) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
        uint32_t ei[4], ej[4];
        dist_code_bytes(ri.w[q], ei);
        dist_code_bytes(rj.w[q], ej);
#pragma unroll
        for (int s = 0; s < 4; s++)
#pragma unroll
            for (int t = 0; t < 4; t++) f[4 * s + t].w[q] = ei[s] & ej[t];
    }
}
FNN_HD void dist_lane_a_pairs(const DistArgs& a, const DistTile& t, int lane, int64_t s, DistFrag* f) {
    const int64_t off = s + dist_lane_k(lane);
    const DistFrag ri = dist_load16(a.seq + (int64_t)t.i * a.lpad + off);
    const DistFrag rj = dist_load16(a.seq + (int64_t)(t.j0 + dist_lane_rc(lane)) * a.lpad + off);
    dist_pair_frags(ri, rj, f);
}

// ---- the epilogue of one lane for one replicate tile.  acc[c][d]: cell c = 4 s + t, digit d.  b0: the first replicate of the
// TILE.  MODEL == DIST_PAIR_COUNTS: a.out is read as int64_t, entry (b, i, j, s, t) at b stride + (i ld + j) 16 + 4 s + t, the
// transposed table at (b, j, i), zeros on the diagonal; nothing is flagged.  A model: as dist_lane_store_model, with the third
// kind.
template <int MODEL, int P>
FNN_HD void dist_lane_store_pairs(const DistArgs& a, const DistPairs& dp, const DistTile& t, int64_t b0, int lane, const DistAcc (*acc)[P]) {
    const int64_t b = b0 + dist_lane_rc(lane);
    if (b >= a.cnt || t.i >= a.n) return;
    if (MODEL == DIST_PAIR_COUNTS) {
        int64_t* T = (int64_t*)a.out + b * a.stride;
        if (t.j0 == t.i + 1 && lane < 16)
#pragma unroll
            for (int c = 0; c < DIST_PAIR_CELLS; c++) T[dist_store_index(t.i, t.i, a.ld) * DIST_PAIR_CELLS + c] = 0;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int32_t j = t.j0 + dist_lane_row(lane, r);
            if (j >= a.n) continue;
#pragma unroll
            for (int s = 0; s < 4; s++)
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int64_t x = dist_combine<P>(acc[4 * s + u], r);
                    T[dist_store_index(t.i, j, a.ld) * DIST_PAIR_CELLS + 4 * s + u] = x;
                    T[dist_store_index(j, t.i, a.ld) * DIST_PAIR_CELLS + 4 * u + s] = x;
                }
        }
        return;
    }
    double* D = a.out + b * a.stride;
    if (t.j0 == t.i + 1 && lane < 16) D[dist_store_index(t.i, t.i, a.ld)] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int32_t j = t.j0 + dist_lane_row(lane, r);
        if (j >= a.n) continue;
        DistTable tb;
#pragma unroll
        for (int c = 0; c < DIST_PAIR_CELLS; c++) tb.F[c] = dist_combine<P>(acc[c], r);
        dist_table_sums(tb);
        double d = 0.0;
        if (tb.v == 0) { a.bad[b] = 1; d = __builtin_nan(""); }
        else if (tb.mism != 0) {
            const int32_t kind = MODEL == FNN_DIST_F81 ? dist_f81(tb, d, dp.shape) : MODEL == FNN_DIST_F84 ? dist_f84(tb, d, dp.shape)
                               : MODEL == FNN_DIST_TN93 ? dist_tn93(tb, d, dp.shape) : dist_logdet(tb, d);
            if (kind == DIST_KIND_DEGENERATE) { dp.sat[b] = 1; d = dp.deg_value; }
            else if (kind == DIST_KIND_SATURATED) { dp.sat[b] = 1; d = dp.sat_value; }
        }
        D[dist_store_index(t.i, j, a.ld)] = d;
        D[dist_store_index(j, t.i, a.ld)] = d;
    }
}

}  // namespace fnn
#endif

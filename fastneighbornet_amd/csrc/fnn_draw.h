// fnn_draw.h -- bootstrap replicates drawn on the device: the per-lane steps of k_draw (fnn_dist.hip),
// shared with the CPU driver (tests/emu/fnn_draw_emu.cpp).  Included by fnn_dist.h, whose DistFrag, dist_load16 and dist_digit
// it uses; the host side of the call is there.
//
// The counts of a bootstrap are a pure function of (seed, L, replicate): draw k of replicate r is
// x = splitmix64_at(seed, r L + k) and increments site floor(x L / 2^64) - fnn_bootstrap_counts' definition.  One workgroup
// makes one row of the digit planes that k_dist / k_dist_model read:
//   1. zero a histogram of lpad site counters in LDS, two 16-bit counters per 32-bit word (a count never exceeds L, and
//      L <= DRAW_MAX_SITES < 65536: a counter cannot carry into its neighbour);
//   2. the threads stride over k and add 1 to their draw's counter with an integer atomic add in LDS (integer additions
//      commute: the histogram does not depend on the order, the result is deterministic);
//   3. each thread turns 16 counters at a time into 16 bytes of every digit plane (dist_digit) and stores them with one
//      16-byte vector store per plane, the zero padding of the sites >= L included (their counters are zero);
//   4. the largest count of the row is reduced over each wave and ends in an integer atomic max on one global word.
// Rows behind the chunk's last problem are padding: all zero.  The row also gets its total[] (L: every replicate draws L
// sites) and its zeroed flags, so that the host uploads nothing per chunk.
#ifndef FNN_DRAW_H
#define FNN_DRAW_H

namespace fnn {

constexpr int32_t DRAW_THREADS = 256;
// The LDS budget of a workgroup: 64 KiB, what a kernel gets without asking for more and what leaves room for two workgroups
// on the 160 KiB of a CU.  A site needs 2 bytes, and the histogram is as long as the padded row (lpad = round_up(L, 64)
// <= 32768 when L <= 32768): DRAW_MAX_SITES = 65536 / 2.
constexpr int32_t DRAW_LDS_BYTES = 64 * 1024;
constexpr int32_t DRAW_MAX_SITES = DRAW_LDS_BYTES / 2;
static_assert(DRAW_MAX_SITES % DIST_K == 0 && DRAW_MAX_SITES <= 65535, "a padded row fits the histogram; a count fits 16 bits");

struct DrawArgs {
    int8_t* planes;          // digit d of the chunk's row b: planes + d * plane_stride + b * lpad (DistArgs' layout)
    int64_t plane_stride, lpad, L;
    int32_t digits;          // planes to write
    int64_t cnt;             // rows 0 ... cnt - 1 are problems, the rows behind them padding
    int64_t first, lead;     // row b is problem first + b of the call; problems below `lead` are the original data
    uint64_t seed;
    int64_t* total;          // total[b] = L, 0 for padding
    int32_t* bad;            // zeroed
    int32_t* sat;            // zeroed; may be null
    uint32_t* max_count;     // one word: the largest count seen so far
};

inline int32_t draw_lds_bytes(int64_t lpad) { return (int32_t)(2 * lpad); }

#if defined(__HIP_DEVICE_COMPILE__)
#define FNN_DRAW_ADD(p, v) atomicAdd((p), (v))
FNN_HD uint64_t draw_site(uint64_t x, uint64_t L) { return __umul64hi(x, L); }
#else
#define FNN_DRAW_ADD(p, v) (*(p) += (v))
FNN_HD uint64_t draw_site(uint64_t x, uint64_t L) { return (uint64_t)(((unsigned __int128)x * (unsigned __int128)L) >> 64); }
#endif
FNN_HD void draw_store16(void* p, const DistFrag& f) { __builtin_memcpy(__builtin_assume_aligned(p, 16), &f, 16); }

// step 1
FNN_HD void draw_lane_zero(uint32_t* hist, int64_t lpad, int tid, int nt) {
    for (int64_t w = tid; w < lpad / 2; w += nt) hist[w] = 0u;
}
// step 2 (an original-data row counts every site once)
FNN_HD void draw_lane_count(const DrawArgs& a, uint32_t* hist, int64_t row, int tid, int nt) {
    const int64_t problem = a.first + row;
    const uint64_t at = (uint64_t)(problem - a.lead) * (uint64_t)a.L;
    for (int64_t k = tid; k < a.L; k += nt) {
        const uint64_t site = problem < a.lead ? (uint64_t)k : draw_site(splitmix64_at(a.seed, at + (uint64_t)k), (uint64_t)a.L);
        FNN_DRAW_ADD(&hist[site >> 1], 1u << (16 * (uint32_t)(site & 1)));
    }
}
// step 3; hist == nullptr: a padding row.  Returns the largest count the lane has seen.
FNN_HD uint32_t draw_lane_planes(const DrawArgs& a, const uint32_t* hist, int64_t row, int tid, int nt) {
    uint32_t most = 0;
    for (int64_t g = tid; g < a.lpad / 16; g += nt) {
        DistFrag c[2] = {DistFrag{{0, 0, 0, 0}}, DistFrag{{0, 0, 0, 0}}};  // 16 counters
        if (hist) { c[0] = dist_load16(hist + 8 * g); c[1] = dist_load16(hist + 8 * g + 4); }
        for (int d = 0; d < a.digits; d++) {
            DistFrag f;
            for (int q = 0; q < 4; q++) {
                uint32_t bytes = 0;
                for (int t = 0; t < 4; t++) {
                    const int s = 4 * q + t;
                    const uint32_t count = (c[s >> 3].w[(s >> 1) & 3] >> (16 * (s & 1))) & 0xffffu;
                    if (d == 0) most = count > most ? count : most;
                    bytes |= (uint32_t)(uint8_t)dist_digit((uint16_t)count, d) << (8 * t);
                }
                f.w[q] = bytes;
            }
            draw_store16(a.planes + (int64_t)d * a.plane_stride + row * a.lpad + 16 * g, f);
        }
    }
    return most;
}
// what k_dist reads of the row beside its planes
FNN_HD void draw_lane_row_words(const DrawArgs& a, int64_t row, int tid) {
    if (tid != 0) return;
    a.total[row] = row < a.cnt ? a.L : 0;
    a.bad[row] = 0;
    if (a.sat) a.sat[row] = 0;
}

}  // namespace fnn
#endif

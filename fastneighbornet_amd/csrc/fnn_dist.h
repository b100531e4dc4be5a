// fnn_dist.h -- p-distance matrices of bootstrap replicates from one alignment: the per-lane
// steps of k_dist (fnn_dist.hip) and the host side of fnn_alignment_distances_batch[_device]_f64, both shared with the
// CPU driver (tests/emu/fnn_dist_emu.cpp) the way fnn_small.h is.
//
// For one alignment and all replicates the counts are a matrix product, C[pair][b] = sum_s M[pair][s] * W[s][b], with M
// the 0/1 indicator of a mismatch (or of "both present") and W the site multiplicities.  One wave takes one TILE of 16
// pairs - one taxon i against 16 consecutive taxa j0 ... j0 + 15 - and DIST_RT tiles of 16 replicates, and walks the
// sites 64 at a time on v_mfma_i32_16x16x64_i8:
//   A (pairs x sites)       lane l holds A[row l & 15][k = 16 (l >> 4) + t], t = 0 ... 15: sixteen 0/1 bytes made in registers
//                           from 16 bytes of row i and 16 bytes of row j0 + (l & 15) (packed-byte arithmetic, no LDS);
//   B (sites x replicates)  lane l holds B[k = 16 (l >> 4) + t][col l & 15]: 16 consecutive bytes of one replicate's row of a
//                           DIGIT PLANE of the counts (int8 operands are signed: a count is split into base-128 digits,
//                           one plane and one int32 accumulator per digit);
//   C / D                   lane l holds C[row 4 (l >> 4) + r][col l & 15] in register r = 0 ... 3.
// The device images are padded by the host: the alignment to n + 16 rows of lpad = round_up(L, 64) bytes, padding 255;
// the planes to round_up(replicates of the chunk, 64) rows of lpad bytes, padding 0.  Padded pairs and replicates compute
// values that are never stored, so the kernel has no tail branch in its loop and a 16-byte load never leaves its buffer.
// Every (b, i, j) is stored by exactly one lane; no atomics, no LDS, no hand-over between workgroups.
//
// Corrected distances (k_dist_model): JC69 changes the epilogue only; K2P adds a third 0/1 operand,
// "both present and a transition", made from the same two 16-byte loads, and a third accumulator set.  What a lane does
// with the exact counts is fnn_dist_model.h.
//
// Bootstrap replicates drawn on the device (k_draw): the planes of a bootstrap are made by a kernel
// from the seed instead of on the host from counts; its per-lane steps are fnn_draw.h, the host side is the one below.
//
// The 4 x 4 table of state pairs (k_dist_pairs): sixteen operands from the same two loads, F81, F84,
// TN93 and LogDet on the exact table, or the table itself; its per-lane steps are fnn_dist_pairs.h, the host side is the one
// below.
//
// Gamma-distributed rates: a shape in DistModel / DistPairs, read by the two model epilogues and filled by
// the host side from a fnn_dist_model_rates; 0.0 is equal rates.  What a lane does with it is fnn_dist_model.h (dist_rate_log).
//
// Site ranges (k_dist_ranges, k_dist_ranges_pairs): problem b is the sites [start_b, end_b), the B operand
// is made in registers from the two bounds and the walk covers the ranges' span only; the per-lane steps are fnn_dist_ranges.h,
// the host side is the one below.
//
// Bootscan (k_draw_ranges, k_dist_scan, k_dist_scan_pairs): P problems per site range, the range's original
// data and bootstrap replicates of the range alone, drawn on the device into compact planes as long as the range's span; the
// per-lane steps are fnn_scan.h, the host side is the one below.
#ifndef FNN_DIST_H
#define FNN_DIST_H

#include <stdint.h>

#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "fnn_dist_model.h"
#include "fnn_small.h"  // batch_chunk (FNN_BATCH_CHUNK), round_up; fnn_engine.h: fail, now_s, the FNN_* codes

namespace fnn {

constexpr int32_t DIST_TILE = 16;          // pairs per tile = replicates per tile (M = N of the instruction)
constexpr int32_t DIST_K = 64;             // sites per instruction
constexpr int32_t DIST_RT = 4;             // replicate tiles per wave: one A fragment serves 4 x digits (x 2) products
constexpr int32_t DIST_WAVES = 4;          // waves per workgroup: 4 pair tiles against the same replicates
constexpr int32_t DIST_THREADS = 64 * DIST_WAVES;
constexpr int32_t DIST_REPS = DIST_TILE * DIST_RT;  // replicates per workgroup
constexpr int32_t DIST_PAD_ROWS = 16;      // rows of 255 behind the alignment: j0 + 15 <= n + 15
constexpr int32_t DIST_MAX_DIGITS = 3;     // 65535 < 128^3

struct alignas(16) DistFrag { uint32_t w[4]; };  // 16 operand bytes of one lane
struct DistAcc { int32_t r[4]; };                // the 4 accumulator registers of one lane
struct DistTile { int32_t i, j0; };              // taxon i against j0 ... j0 + 15; i == n: a filler tile, nothing stored

struct DistArgs {
    const uint8_t* seq;      // n + DIST_PAD_ROWS rows of lpad bytes
    int64_t lpad;
    const DistTile* tiles;   // a multiple of DIST_WAVES
    const int8_t* planes;    // digit d of the chunk's replicate b: planes + d * plane_stride + b * lpad
    int64_t plane_stride;
    const int64_t* total;    // sum of the counts of replicate b: `valid` of every pair when no byte is missing
    int32_t n;
    int64_t cnt;             // replicates of the chunk
    double* out;             // replicate b at out + b * stride, row stride ld
    int64_t ld, stride;
    int32_t* bad;            // bad[b] = 1: some pair of replicate b has valid == 0 (its entries are NaN)
};
// what k_dist_model needs beyond DistArgs
struct DistModel {
    int32_t states;          // JC69: k
    double sat_value;        // stored for a saturated pair: the cap, or +inf when the call is going to fail
    int32_t* sat;            // sat[b] = 1: some pair of replicate b is saturated (written like bad[])
    double shape;            // 0.0: equal rates; alpha > 0: gamma-distributed rates
};
// replicate tiles per wave of k_dist_model: K2P with three digit planes and `valid` counted holds 9 accumulator sets per
// replicate tile; at DIST_RT tiles the compiler fills all 256 VGPRs and parks 15 more values in AGPRs inside the loop (no
// scratch yet, and no margin), at 2 tiles it needs 184 + 72
constexpr int32_t dist_model_rt(int32_t model, int32_t P, bool missing) { return model == FNN_DIST_K2P && P == 3 && missing ? 2 : DIST_RT; }

// ---- fragment construction from bytes
FNN_HD DistFrag dist_load16(const void* p) {
    DistFrag f;
    __builtin_memcpy(&f, __builtin_assume_aligned(p, 16), 16);
    return f;
}
// per byte of x: 1 where the byte is not zero, else 0
FNN_HD uint32_t dist_nonzero_bytes(uint32_t x) { return ((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u) >> 7; }
// the A operands of one lane from its 16 bytes of row i and of row j: mism = both present and different, valid = both
// present (MISSING only; without a missing byte in the alignment mism is "different" and valid is not needed)
template <bool MISSING>
FNN_HD void dist_a_frags(const DistFrag& ri, const DistFrag& rj, DistFrag& mism, DistFrag& valid) {
    for (int q = 0; q < 4; q++) {
        uint32_t d = dist_nonzero_bytes(ri.w[q] ^ rj.w[q]);
        if (MISSING) {
            const uint32_t p = dist_nonzero_bytes(~ri.w[q]) & dist_nonzero_bytes(~rj.w[q]);  // (~x == 0: the byte is 255)
            valid.w[q] = p;
            d &= p;
        }
        mism.w[q] = d;
    }
}
// the same with the K2P operand: ts = both present and the codes (A 0, C 1, G 2, T 3) differ by a transition, i.e. their
// xor is 2 (A ^ G = C ^ T = 2).  A missing byte is 255: 255 ^ code is never 2, so without MISSING no mask is needed.
template <bool MISSING>
FNN_HD void dist_a_frags_ts(const DistFrag& ri, const DistFrag& rj, DistFrag& mism, DistFrag& valid, DistFrag& ts) {
    dist_a_frags<MISSING>(ri, rj, mism, valid);
    for (int q = 0; q < 4; q++) {
        uint32_t s = ~dist_nonzero_bytes((ri.w[q] ^ rj.w[q]) ^ 0x02020202u) & 0x01010101u;
        if (MISSING) s &= valid.w[q];
        ts.w[q] = s;
    }
}
// lane maps of the 16 x 16 x 64 int8 form (verified with exact integers: tests/dist_common.py, case "lane maps")
FNN_HD int dist_lane_rc(int lane) { return lane & 15; }        // A: row (pair of the tile); B, C: column (replicate)
FNN_HD int dist_lane_k(int lane) { return 16 * (lane >> 4); }  // A, B: first of the lane's 16 consecutive k (sites)
FNN_HD int dist_lane_row(int lane, int r) { return 4 * (lane >> 4) + r; }  // C: row (pair) of accumulator register r

template <bool MISSING>
FNN_HD void dist_lane_a(const DistArgs& a, const DistTile& t, int lane, int64_t s, DistFrag& mism, DistFrag& valid) {
    const int64_t off = s + dist_lane_k(lane);
    const DistFrag ri = dist_load16(a.seq + (int64_t)t.i * a.lpad + off);
    const DistFrag rj = dist_load16(a.seq + (int64_t)(t.j0 + dist_lane_rc(lane)) * a.lpad + off);
    dist_a_frags<MISSING>(ri, rj, mism, valid);
}
template <bool MISSING>
FNN_HD void dist_lane_a_ts(const DistArgs& a, const DistTile& t, int lane, int64_t s, DistFrag& mism, DistFrag& valid, DistFrag& ts) {
    const int64_t off = s + dist_lane_k(lane);
    const DistFrag ri = dist_load16(a.seq + (int64_t)t.i * a.lpad + off);
    const DistFrag rj = dist_load16(a.seq + (int64_t)(t.j0 + dist_lane_rc(lane)) * a.lpad + off);
    dist_a_frags_ts<MISSING>(ri, rj, mism, valid, ts);
}
// b0: the first replicate of the workgroup (a multiple of DIST_REPS), rt: the replicate tile, d: the digit
FNN_HD DistFrag dist_lane_b(const DistArgs& a, int64_t b0, int rt, int d, int lane, int64_t s) {
    return dist_load16(a.planes + (int64_t)d * a.plane_stride + (b0 + DIST_TILE * rt + dist_lane_rc(lane)) * a.lpad + s + dist_lane_k(lane));
}

// ---- digit split and combine
FNN_HD int8_t dist_digit(uint16_t c, int d) { return (int8_t)((c >> (7 * d)) & 127); }
template <int P>
FNN_HD int64_t dist_combine(const DistAcc* acc, int r) {  // (each digit's sum is below 2^31: 127 L < 2^31 is an argument check)
    int64_t v = 0;
    for (int d = P; d-- > 0;) v = v * 128 + (int64_t)acc[d].r[r];
    return v;
}
FNN_HD double dist_divide(int64_t mism, int64_t valid) { return (double)mism / (double)valid; }  // one IEEE division
FNN_HD int64_t dist_store_index(int64_t i, int64_t j, int64_t ld) { return i * ld + j; }

// ---- the tile product over the 64 lanes' fragments.  Device: the instruction; host: loops from the lane maps above.
#if defined(__HIPCC__)
typedef int dist_v4i __attribute__((ext_vector_type(4)));
__device__ __forceinline__ DistAcc dist_mma(const DistFrag& a, const DistFrag& b, const DistAcc& c) {
#if defined(__HIP_DEVICE_COMPILE__)
    const dist_v4i va = {(int)a.w[0], (int)a.w[1], (int)a.w[2], (int)a.w[3]}, vb = {(int)b.w[0], (int)b.w[1], (int)b.w[2], (int)b.w[3]};
    const dist_v4i vc = {c.r[0], c.r[1], c.r[2], c.r[3]};
    const dist_v4i o = __builtin_amdgcn_mfma_i32_16x16x64_i8(va, vb, vc, 0, 0, 0);
    return DistAcc{{o[0], o[1], o[2], o[3]}};
#else
    return c;  // (the host pass only parses the kernel)
#endif
}
#endif
#if !defined(__HIP_DEVICE_COMPILE__)
inline void dist_tile_product(const DistFrag* A, const DistFrag* B, DistAcc* C) {  // 64 lanes each; C += A * B
    for (int lane = 0; lane < 64; lane++)
        for (int r = 0; r < 4; r++) {
            const int row = dist_lane_row(lane, r), col = dist_lane_rc(lane);
            int32_t sum = C[lane].r[r];
            for (int g = 0; g < 4; g++) {  // k = 16 g + t lives in lane (g, row) of A and lane (g, col) of B
                int8_t ab[16], bb[16];
                std::memcpy(ab, &A[16 * g + row], 16);
                std::memcpy(bb, &B[16 * g + col], 16);
                for (int t = 0; t < 16; t++) sum += (int32_t)ab[t] * (int32_t)bb[t];
            }
            C[lane].r[r] = sum;
        }
}
#endif

// ---- the epilogue of one lane for one replicate tile: combine, divide, store both triangles (and the diagonal, by the
// first tile of each taxon).  b0: the first replicate of the TILE.
template <int P, bool MISSING>
FNN_HD void dist_lane_store(const DistArgs& a, const DistTile& t, int64_t b0, int lane, const DistAcc* mism, const DistAcc* valid) {
    const int64_t b = b0 + dist_lane_rc(lane);
    if (b >= a.cnt || t.i >= a.n) return;
    double* D = a.out + b * a.stride;
    if (t.j0 == t.i + 1 && lane < 16) D[dist_store_index(t.i, t.i, a.ld)] = 0.0;
    for (int r = 0; r < 4; r++) {
        const int32_t j = t.j0 + dist_lane_row(lane, r);
        if (j >= a.n) continue;
        const int64_t m = dist_combine<P>(mism, r);
        const int64_t v = MISSING ? dist_combine<P>(valid, r) : a.total[b];
        double d;
        if (v == 0) { a.bad[b] = 1; d = __builtin_nan(""); }
        else d = dist_divide(m, v);
        D[dist_store_index(t.i, j, a.ld)] = d;
        D[dist_store_index(j, t.i, a.ld)] = d;
    }
}

// The same for a corrected distance (MODEL = FNN_DIST_JC69 or FNN_DIST_K2P; `ts` is read by K2P only): an empty pair is NaN
// and flags bad[b] as above; a saturated pair is dm.sat_value and flags dm.sat[b]; no mismatch is +0.0.  With dm.shape > 0 a
// pair whose expm1' overflows is saturated too (fnn_dist_model.h, dist_rate_log).
template <int MODEL, int P, bool MISSING>
FNN_HD void dist_lane_store_model(const DistArgs& a, const DistModel& dm, const DistTile& t, int64_t b0, int lane, const DistAcc* mism,
                                  const DistAcc* valid, const DistAcc* ts) {
    const int64_t b = b0 + dist_lane_rc(lane);
    if (b >= a.cnt || t.i >= a.n) return;
    double* D = a.out + b * a.stride;
    if (t.j0 == t.i + 1 && lane < 16) D[dist_store_index(t.i, t.i, a.ld)] = 0.0;
    for (int r = 0; r < 4; r++) {
        const int32_t j = t.j0 + dist_lane_row(lane, r);
        if (j >= a.n) continue;
        const int64_t m = dist_combine<P>(mism, r);
        const int64_t v = MISSING ? dist_combine<P>(valid, r) : a.total[b];
        double d;
        if (v == 0) { a.bad[b] = 1; d = __builtin_nan(""); }
        else if (m == 0) d = 0.0;
        else {
            const int64_t s = MODEL == FNN_DIST_K2P ? dist_combine<P>(ts, r) : 0;
            const bool sat = MODEL == FNN_DIST_K2P ? dist_k2p_saturated(s, m - s, v) : dist_jc69_saturated(dm.states, m, v);
            if (sat) { dm.sat[b] = 1; d = dm.sat_value; }
            else {
                bool over = false;
                d = MODEL == FNN_DIST_K2P ? dist_k2p(s, m - s, v, dm.shape, over) : dist_jc69(dm.states, m, v, dm.shape, over);
                if (over) { dm.sat[b] = 1; d = dm.sat_value; }
            }
        }
        D[dist_store_index(t.i, j, a.ld)] = d;
        D[dist_store_index(j, t.i, a.ld)] = d;
    }
}

}  // namespace fnn
#include "fnn_draw.h"  // the per-lane steps of k_draw: the planes of a bootstrap made where they are read
#include "fnn_dist_pairs.h"  // the per-lane steps of k_dist_pairs: the 4 x 4 table of state pairs and its models
#include "fnn_dist_ranges.h"  // the per-lane steps of the range kernels: the B operand from a range's bounds
#include "fnn_scan.h"  // the per-lane steps of the bootscan kernels: compact planes of a bootstrap of every range
namespace fnn {

// ------------------------------------------------------------------------------------------------ host side
// tiles of taxon i: j0 = i + 1 + 16 t while j0 < n, and at least one (it stores the diagonal entry); filled up to a
// multiple of DIST_WAVES with {n, n}
inline std::vector<DistTile> dist_tiles(int32_t n) {
    std::vector<DistTile> t;
    for (int32_t i = 0; i < n; i++) {
        t.push_back(DistTile{i, i + 1});
        for (int64_t j0 = (int64_t)i + 1 + DIST_TILE; j0 < n; j0 += DIST_TILE) t.push_back(DistTile{i, (int32_t)j0});
    }
    while (t.size() % DIST_WAVES) t.push_back(DistTile{n, n});
    return t;
}
inline bool dist_force_missing() {
    const char* e = std::getenv("FNN_DIST_FORCE_MISSING");
    return e && std::atoi(e) == 1;
}
// FNN_DIST_FORCE_DIGITS=2|3 (tests): at least that many digit planes are allocated, filled and multiplied; the high ones are
// all zero wherever the counts do not need them, and the counts are exact integers: the same bytes come out
inline int32_t dist_force_digits() {
    const char* e = std::getenv("FNN_DIST_FORCE_DIGITS");
    const int v = e ? std::atoi(e) : 0;
    return v == 2 || v == 3 ? v : 1;
}
// FNN_DRAW_ROUTE=device|host (tests): where a bootstrap is drawn; anything else leaves the choice to the call
inline int32_t dist_draw_route_switch() {
    const char* e = std::getenv("FNN_DRAW_ROUTE");
    if (e && std::strcmp(e, "device") == 0) return FNN_DRAW_DEVICE;
    if (e && std::strcmp(e, "host") == 0) return FNN_DRAW_HOST;
    return -1;
}
inline int32_t dist_digits_of(uint32_t cmax) { return cmax <= 127 ? 1 : (cmax <= 16383 ? 2 : 3); }
inline int32_t dist_fail_no_site(const std::string& W, int64_t b, int64_t i, int64_t j) {
    return fail(FNN_EINVAL, W + "no site with both taxa present (valid == 0) at (b, i, j) = (" + std::to_string(b) + ", " + std::to_string(i) +
                                ", " + std::to_string(j) + ")");
}

// fnn_bootstrap_counts: replicate b draws k = 0 ... L - 1 and increments site floor(x L / 2^64), x = splitmix64_at(seed, b L + k)
inline int32_t dist_bootstrap_counts(const char* who, int64_t L, int64_t batch, uint64_t seed, uint16_t* counts_out) {
    const std::string W = std::string(who) + ": ";
    if (L <= 0 || batch < 0) return fail(FNN_EINVAL, W + "needs L > 0 and batch >= 0");
    if (batch == 0) return FNN_OK;
    if (!counts_out) return fail(FNN_EINVAL, W + "NULL argument");
    std::vector<uint32_t> row((size_t)L);
    for (int64_t b = 0; b < batch; b++) {
        std::fill(row.begin(), row.end(), 0u);
        for (int64_t k = 0; k < L; k++) {
            const uint64_t x = splitmix64_at(seed, (uint64_t)b * (uint64_t)L + (uint64_t)k);
            row[(size_t)(uint64_t)(((unsigned __int128)x * (unsigned __int128)(uint64_t)L) >> 64)]++;
        }
        for (int64_t s = 0; s < L; s++) {
            if (row[(size_t)s] > 65535u) return fail(FNN_EINVAL, W + "replicate " + std::to_string(b) + ": a site was drawn more than 65535 times");
            counts_out[b * L + s] = (uint16_t)row[(size_t)s];
        }
    }
    return FNN_OK;
}

// fnn_alignment_distances_batch[_device]_f64 over a backend B (HIP: fnn_dist.hip; CPU driver: tests/emu):
//   open(device); alloc; h2d / d2h; run(digits, missing, args, tile groups, replicate groups, &t_kernel_s); err()
// The host variant writes D_out only when the whole call has succeeded.
// A backend that has the corrected distances adds run_model(model, digits, missing, args, model args, tile groups,
// replicates of the chunk, &t_kernel_s) and sizes its grid from dist_model_rt; one without it knows FNN_DIST_P only.
template <class B, class = void>
struct dist_runs_models : std::false_type {};
template <class B>
struct dist_runs_models<B, std::void_t<decltype(&B::run_model)>> : std::true_type {};

// A backend that has the 4 x 4 tables adds run_pairs(model or DIST_PAIR_COUNTS, digits, args, pair args, tile groups, replicates
// of the chunk, &t_kernel_s) and sizes its grid from dist_pairs_rt; one without it refuses FNN_DIST_F81 ... FNN_DIST_LOGDET.
template <class B, class = void>
struct dist_runs_pairs : std::false_type {};
template <class B>
struct dist_runs_pairs<B, std::void_t<decltype(&B::run_pairs)>> : std::true_type {};

inline int32_t dist_fail_degenerate(const std::string& W, int64_t b, int64_t i, int64_t j) {
    return fail(FNN_EINVAL, W + "degenerate pair (a base that the model divides by does not occur in it) at (b, i, j) = (" + std::to_string(b) + ", " +
                                std::to_string(i) + ", " + std::to_string(j) + ")");
}
inline int32_t dist_fail_saturated(const std::string& W, int64_t b, int64_t i, int64_t j) {
    return fail(FNN_EINVAL, W + "saturated pair (the model's distance is infinite) at (b, i, j) = (" + std::to_string(b) + ", " + std::to_string(i) +
                                ", " + std::to_string(j) + ")");
}
// K2P's codes: A a -> 0, C c -> 1, G g -> 2, T t U u -> 3, 255 stays, every other byte -> 255
inline void dist_k2p_codes(uint8_t* lut) {
    std::memset(lut, FNN_SITE_MISSING, 256);
    const char* letters = "AaCcGgTtUu";
    const uint8_t code[10] = {0, 0, 1, 1, 2, 2, 3, 3, 3, 3};
    for (int k = 0; k < 10; k++) lut[(uint8_t)letters[k]] = code[k];
}

// A backend that can draw a bootstrap's planes itself adds run_draw(draw args, rows, &t_draw_s): one workgroup per row.
template <class B, class = void>
struct dist_runs_draw : std::false_type {};
template <class B>
struct dist_runs_draw<B, std::void_t<decltype(&B::run_draw)>> : std::true_type {};

// A backend that has the range kernels (and the models and tables: the ranges take every model) adds
// run_ranges(model, missing, args, ranges, model args, tile groups, problems of the chunk, &t_kernel_s) and
// run_ranges_pairs(model or DIST_PAIR_COUNTS, args, ranges, pair args, ...): one window tile of 16 problems per wave.
template <class B, class = void>
struct dist_runs_ranges : std::false_type {};
template <class B>
struct dist_runs_ranges<B, std::void_t<decltype(&B::run_ranges), decltype(&B::run_ranges_pairs)>> : std::true_type {};

// A backend that has the bootscan kernels (and the draw, the models and the tables) adds run_draw_ranges(scan args, rows, the widest
// span, &t_draw_s): one workgroup per row; run_scan(model, missing, args, scan args, model args, tile groups, column groups,
// &t_kernel_s) and run_scan_pairs(model or DIST_PAIR_COUNTS, args, scan args, pair args, ...): one column group per wave.
template <class B, class = void>
struct dist_runs_scan : std::false_type {};
template <class B>
struct dist_runs_scan<B, std::void_t<decltype(&B::run_draw_ranges), decltype(&B::run_scan), decltype(&B::run_scan_pairs)>> : std::true_type {};

// Where the site multiplicities of a call come from: the caller's array, or a bootstrap of `seed` - problems 0 ... lead - 1
// the original data (every site once), problem b >= lead replicate b - lead of fnn_bootstrap_counts(L, batch - lead, seed) -
// drawn on the host into such an array or on the device straight into the planes, or `batch` site
// ranges, whose 0/1 multiplicities exist nowhere, or a bootstrap of each of `windows` site ranges, per_window
// problems each, whose compact planes are drawn on the device.
struct DistSource {
    const uint16_t* counts = nullptr;
    int64_t ldc = 0;
    bool bootstrap = false;
    int32_t draw_route = FNN_DRAW_HOST;  // of a bootstrap
    uint64_t seed = 0;
    int64_t lead = 0;
    bool pair_counts = false;            // the call wants the 4 x 4 tables (16 int64_t per pair in place of one double), no distance
    bool ranges = false;                 // problem b is the sites starts[b] <= s < ends[b]
    const int64_t* starts = nullptr;
    const int64_t* ends = nullptr;
    fnn_range_stats* range_stats = nullptr;  // of a call on ranges: receives n_site_blocks, n_site_blocks_dense
    bool scan = false;                   // problem p is q = p % per_window of the window [starts[w], ends[w]), w = p / per_window; seed, lead
    int64_t windows = 0, per_window = 0;
    fnn_scan_stats* scan_stats = nullptr;    // of a bootscan: receives n_windows, n_site_blocks, n_site_blocks_dense, n_host_chunks
    int64_t base = 0;                    // problem 0 of this call is problem `base` of the caller's: what a failure names
};

template <class B>
int32_t dist_batch_source(B& be, const char* who, const uint8_t* seq, int32_t n, int64_t L, int64_t lds, DistSource src, int64_t batch,
                          const fnn_dist_model* mp, int32_t device, double* D_out, bool on_device, int64_t ld, int64_t stride, fnn_boot_stats* stats) {
    const double t0 = now_s();
    const std::string W = std::string(who) + ": ";
    fnn_boot_stats bst{};
    fnn_dist_model_stats& mst = bst.model;
    fnn_dist_stats& st = mst.base;
    const bool draw = src.bootstrap && src.draw_route == FNN_DRAW_DEVICE;
    bst.draw_route = draw ? FNN_DRAW_DEVICE : FNN_DRAW_HOST;
    if (n <= 0 || L <= 0 || batch < 0) return fail(FNN_EINVAL, W + "needs n > 0, L > 0 and batch >= 0");
    if (!mp) return fail(FNN_EINVAL, W + "NULL model");
    const bool tables = src.pair_counts;
    const int32_t model = tables ? DIST_PAIR_COUNTS : mp->model;
    const bool pairs = dist_runs_pairs<B>::value && (tables || dist_is_pair_model(model));
    const bool known = model == FNN_DIST_P || (dist_runs_models<B>::value && (model == FNN_DIST_JC69 || model == FNN_DIST_K2P)) || pairs;
    if (!known) return fail(FNN_EINVAL, W + "unknown model");
    const bool recoded = model == FNN_DIST_K2P || pairs;  // K2P's codes
    const int64_t cell = tables ? DIST_PAIR_CELLS : 1;   // 8-byte words per (i, j) of the output
    const bool cap = mp->on_saturation == FNN_DIST_SAT_CAP;
    if (mp->on_saturation != FNN_DIST_SAT_FAIL && !cap) return fail(FNN_EINVAL, W + "unknown saturation policy");
    // rates across sites: mp->reserved; with FNN_DIST_RATES_GAMMA mp is the first member of a fnn_dist_model_rates
    double shape = 0.0;
    if (!tables) {
        if (mp->reserved != FNN_DIST_RATES_EQUAL && mp->reserved != FNN_DIST_RATES_GAMMA)
            return fail(FNN_EINVAL, W + "unknown rates (the field `reserved` of fnn_dist_model: 0 equal, 1 gamma)");
        if (mp->reserved == FNN_DIST_RATES_GAMMA) {
            const fnn_dist_model_rates* mr = reinterpret_cast<const fnn_dist_model_rates*>(mp);
            if (model == FNN_DIST_P || model == FNN_DIST_LOGDET) return fail(FNN_EINVAL, W + "rates: this model has no gamma form (FNN_DIST_P, FNN_DIST_LOGDET)");
            if (!(mr->shape > 0.0 && mr->shape <= 1.7976931348623157e308)) return fail(FNN_EINVAL, W + "the shape of the gamma rates must be finite and > 0");
            if (mr->reserved[0] != 0.0 || mr->reserved[1] != 0.0 || mr->reserved[2] != 0.0)
                return fail(FNN_EINVAL, W + "the field `reserved` of fnn_dist_model_rates must be zero");
            shape = mr->shape;
        }
    }
    if (model == FNN_DIST_JC69 && (mp->states < 2 || mp->states > 255)) return fail(FNN_EINVAL, W + "JC69 needs 2 <= states <= 255");
    if (model != FNN_DIST_P && cap && !(mp->cap > 0.0 && mp->cap <= 1.7976931348623157e308))
        return fail(FNN_EINVAL, W + "the cap of saturated pairs must be finite and > 0");
    if (L > (((int64_t)1 << 31) - 1) / 127) return fail(FNN_EINVAL, W + "too many sites: 127 L must stay below 2^31 (the int32 digit accumulators)");
    if (batch == 0) { if (stats) *stats = bst; return FNN_OK; }
    const bool bounds = src.ranges || src.scan;  // the call has starts and ends, and no counts
    if (!seq || (!src.bootstrap && !bounds && !src.counts) || (bounds && (!src.starts || !src.ends)) || !D_out)
        return fail(FNN_EINVAL, W + "NULL argument");
    if (lds < L || (!src.bootstrap && !bounds && src.ldc < L)) return fail(FNN_EINVAL, W + (bounds ? "needs lds >= L" : "needs lds >= L and ldc >= L"));
    if (ld < n || stride < (int64_t)n * ld * cell) return fail(FNN_EINVAL, W + (tables ? "needs ld >= n and stride >= 16 * n * ld" : "needs ld >= n and stride >= n * ld"));
    if (src.ranges) {
        if (!dist_runs_ranges<B>::value) return fail(FNN_EINVAL, W + "this backend has no range kernels");
        for (int64_t b = 0; b < batch; b++)
            if (src.starts[b] < 0 || src.starts[b] > src.ends[b] || src.ends[b] > L)
                return fail(FNN_EINVAL, W + "range " + std::to_string(b) + ": needs 0 <= start <= end <= L, got [" + std::to_string(src.starts[b]) + ", " +
                                            std::to_string(src.ends[b]) + ")");
    }
    int32_t scan_widest = 0;  // the widest padded span of a bootscan's windows
    if (src.scan) {
        if (!dist_runs_scan<B>::value) return fail(FNN_EINVAL, W + "this backend has no bootscan kernels");
        for (int64_t w = 0; w < src.windows; w++) {
            if (src.starts[w] < 0 || src.starts[w] > src.ends[w] || src.ends[w] > L)
                return fail(FNN_EINVAL, W + "window " + std::to_string(w) + ": needs 0 <= start <= end <= L, got [" + std::to_string(src.starts[w]) + ", " +
                                            std::to_string(src.ends[w]) + ")");
            const int32_t span = scan_ceil64(src.ends[w]) - scan_floor64(src.starts[w]);
            scan_widest = span > scan_widest ? span : scan_widest;
        }
        const int32_t sw = dist_draw_route_switch();
        if (sw == FNN_DRAW_DEVICE && scan_widest > DRAW_MAX_SITES)
            return fail(FNN_EINVAL, W + "the draw kernel takes windows of at most " + std::to_string(DRAW_MAX_SITES) + " padded sites (FNN_DRAW_ROUTE=device)");
        src.draw_route = sw >= 0 ? sw : (scan_widest <= DRAW_MAX_SITES ? FNN_DRAW_DEVICE : FNN_DRAW_HOST);
        bst.draw_route = src.draw_route;
    }
    if (draw && !dist_runs_draw<B>::value) return fail(FNN_EINVAL, W + "this backend has no draw kernel");
    if (draw && L > DRAW_MAX_SITES)
        return fail(FNN_EINVAL, W + "the draw kernel takes at most " + std::to_string(DRAW_MAX_SITES) + " sites (FNN_DRAW_ROUTE=device)");
    st.n_problems = batch;
    st.n_pairs = (int64_t)n * (n - 1) / 2;
    st.n_sites = L;
    st.block_threads = DIST_THREADS;

    // one look at the inputs: a missing byte, the largest count, every replicate's total
    bool missing = dist_force_missing();
    uint8_t lut[256];
    if (recoded) {  // what the recoding turns into 255 is missing too
        dist_k2p_codes(lut);
        for (int32_t i = 0; i < n; i++) {
            const uint8_t* row = seq + (int64_t)i * lds;
            for (int64_t s = 0; s < L; s++) {
                if (lut[row[s]] != FNN_SITE_MISSING) continue;
                missing = true;
                if (row[s] != FNN_SITE_MISSING) mst.n_recoded++;
            }
        }
    } else if (model == FNN_DIST_JC69) {
        bool seen[256] = {};
        for (int32_t i = 0; i < n; i++) {
            const uint8_t* row = seq + (int64_t)i * lds;
            for (int64_t s = 0; s < L; s++) seen[row[s]] = true;
        }
        int32_t distinct = 0;
        for (int k = 0; k < FNN_SITE_MISSING; k++) distinct += seen[k] ? 1 : 0;
        if (distinct > mp->states)
            return fail(FNN_EINVAL, W + "the alignment holds " + std::to_string(distinct) + " distinct states, more than states = " + std::to_string(mp->states));
        missing = missing || seen[FNN_SITE_MISSING];
    } else
        for (int32_t i = 0; i < n && !missing; i++) missing = std::memchr(seq + (int64_t)i * lds, FNN_SITE_MISSING, (size_t)L) != nullptr;
    st.has_missing = missing ? 1 : 0;
    // a bootstrap drawn on the host: the counts this call would have been given
    std::vector<uint16_t> drawn;
    if (src.bootstrap && !draw) {
        drawn.assign((size_t)batch * (size_t)L, (uint16_t)1);  // (the rows below `lead` stay all ones)
        const int32_t rd = dist_bootstrap_counts(who, L, batch - src.lead, src.seed, drawn.data() + src.lead * L);
        if (rd != FNN_OK) return rd;
        src.counts = drawn.data();
        src.ldc = L;
    }
    const uint16_t* counts = src.counts;
    const int64_t ldc = src.ldc;
    // (drawn on the device: every row's total is L > 0, and the largest count is the kernel's to report)
    // (a bootscan: a row's total is its window's width, the device route has one digit and the kernel reports the largest count)
    std::vector<int64_t> total(draw || src.scan ? 0 : (size_t)batch, 0);
    uint32_t cmax = 0;
    for (int64_t b = 0; b < batch && !draw && !bounds; b++) {
        const uint16_t* c = counts + b * ldc;
        int64_t t = 0;
        for (int64_t s = 0; s < L; s++) { t += c[s]; cmax = c[s] > cmax ? c[s] : cmax; }
        total[(size_t)b] = t;
    }
    // (ranges: the row's total is the range's length, every count is 0 or 1 and there is one digit, whatever the switch says)
    for (int64_t b = 0; b < batch && src.ranges; b++) {
        total[(size_t)b] = src.ends[b] - src.starts[b];
        if (total[(size_t)b] > 0) cmax = 1;
    }
    int32_t P = dist_digits_of(cmax);
    if (dist_force_digits() > P && !bounds) P = dist_force_digits();
    // valid is the total: an empty replicate has valid == 0 for every pair, (0, 1) the lowest (with missing bytes the
    // kernel flags it, so that a lower replicate with one empty pair is named first; so it does when a saturated pair fails
    // the call, for the same reason)
    const bool sat_fails = model != FNN_DIST_P && !cap && !tables;
    if (n >= 2 && !missing && !sat_fails && !tables)
        for (int64_t b = 0; b < batch && !draw && !src.scan; b++)
            if (total[(size_t)b] == 0) return dist_fail_no_site(W, src.base + b, 0, 1);
    if (src.scan && n >= 2 && !missing && !sat_fails && !tables)  // (an empty window is P empty rows: its first problem is the lowest)
        for (int64_t w = 0; w < src.windows; w++)
            if (src.starts[w] == src.ends[w]) return dist_fail_no_site(W, src.base + w * src.per_window, 0, 1);
    const int64_t lpad = round_up(L, (int64_t)DIST_K), nn = (int64_t)n * n;
    int64_t site_blocks = 0, host_chunks = 0;
    // what ends every successful call: the host variant's output, the stats
    auto finish = [&](const std::vector<double>& staged) {
        if (!on_device)
            for (int64_t b = 0; b < batch; b++)
                for (int32_t r = 0; r < n; r++)
                    std::memcpy(D_out + b * stride + (int64_t)r * ld * cell, &staged[(size_t)b * (size_t)(nn * cell) + (size_t)r * (size_t)(n * cell)],
                                sizeof(double) * (size_t)(n * cell));
        st.digit_passes = P;
        bst.max_count = (int32_t)cmax;
        const int64_t dense = (batch + DIST_TILE - 1) / DIST_TILE * (lpad / DIST_K);
        if (src.range_stats) {
            src.range_stats->n_site_blocks = site_blocks;
            src.range_stats->n_site_blocks_dense = dense;
        }
        if (src.scan_stats) {
            src.scan_stats->n_windows = src.windows;
            src.scan_stats->n_site_blocks = site_blocks;
            src.scan_stats->n_site_blocks_dense = dense;
            src.scan_stats->n_host_chunks = host_chunks;
        }
        st.t_total_s = now_s() - t0;
        if (stats) *stats = bst;
        return FNN_OK;
    };
    // A bootscan's host route is the definition itself: slices of fnn_bootscan_counts through the counts source above, on a backend
    // of their own, at most SCAN_COUNTS_BYTES of counts at a time.  It serves a whole call (a window wider than the draw kernel
    // takes, FNN_DRAW_ROUTE=host) or single chunks of the device route (a chunk that needs more than one digit).  Such rows walk
    // the whole alignment: they count as dense in n_site_blocks.
    auto scan_host_rows = [&](int64_t first, int64_t count, double* dst, bool dst_on_device, int64_t dld, int64_t dstride) -> int32_t {
        const int64_t most = SCAN_COUNTS_BYTES / (2 * L) > 1 ? SCAN_COUNTS_BYTES / (2 * L) : 1;
        std::vector<uint16_t> rows;
        for (int64_t f = first; f < first + count; f += most) {
            const int64_t c = first + count - f < most ? first + count - f : most;
            rows.resize((size_t)c * (size_t)L);
            int32_t r = dist_bootscan_counts(who, L, src.starts, src.ends, src.windows, src.per_window - src.lead, src.lead, src.seed, f, c, rows.data());
            if (r != FNN_OK) return r;
            DistSource cs;
            cs.counts = rows.data();
            cs.ldc = L;
            cs.pair_counts = src.pair_counts;
            cs.base = src.base + f;
            fnn_boot_stats sub{};
            B side;
            r = dist_batch_source(side, who, seq, n, L, lds, cs, c, mp, device, dst + (f - first) * dstride, dst_on_device, dld, dstride, &sub);
            if (r != FNN_OK) return r;
            st.t_upload_s += sub.model.base.t_upload_s;
            st.t_kernel_s += sub.model.base.t_kernel_s;
            mst.n_saturated_problems += sub.model.n_saturated_problems;
            cmax = (uint32_t)sub.max_count > cmax ? (uint32_t)sub.max_count : cmax;
            P = sub.model.base.digit_passes > P ? sub.model.base.digit_passes : P;
            site_blocks += (c + DIST_TILE - 1) / DIST_TILE * (lpad / DIST_K);
        }
        return FNN_OK;
    };
    if (src.scan && src.draw_route == FNN_DRAW_HOST) {
        std::vector<double> staged(on_device ? 0 : (size_t)(nn * cell) * (size_t)batch);
        const int64_t chunk = batch_chunk(batch, 8 * nn * cell + 2 * L, false);
        for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
            const int64_t cnt = batch - b0 < chunk ? batch - b0 : chunk;
            st.chunks++;
            const int32_t rh = on_device ? scan_host_rows(b0, cnt, D_out + b0 * stride, true, ld, stride)
                                         : scan_host_rows(b0, cnt, &staged[(size_t)b0 * (size_t)(nn * cell)], false, n, nn * cell);
            if (rh != FNN_OK) return rh;
        }
        return finish(staged);
    }

    int32_t rc = be.open(device);
    if (rc != FNN_OK) return fail(rc, W + be.err());
    const double tu0 = now_s();
    const std::vector<DistTile> tiles = dist_tiles(n);
    const int64_t chunk = batch_chunk(batch, 8 * nn * cell + (src.ranges ? 0 : src.scan ? (int64_t)scan_widest : (int64_t)P * lpad), false),
                  cpad = round_up(chunk, (int64_t)DIST_REPS);
    const size_t seq_bytes = (size_t)(n + DIST_PAD_ROWS) * (size_t)lpad;
    // a bootscan's planes are compact: the bytes of the chunk that needs most; its draw reports one largest count per chunk
    const int32_t scan_group = DIST_TILE * scan_rt(pairs);
    const int64_t n_chunks = (batch + chunk - 1) / chunk;
    std::vector<ScanWindow> s_wins;
    std::vector<ScanGroup> s_groups;
    size_t scan_bytes = 0, scan_wins = 0, scan_groups = 0;
    for (int64_t b0 = 0; b0 < batch && src.scan; b0 += chunk) {
        int32_t span = 0;
        int64_t blocks = 0;
        const size_t bytes = (size_t)scan_chunk(src.starts, src.ends, src.per_window, src.seed, b0, batch - b0 < chunk ? batch - b0 : chunk, scan_group, s_wins,
                                                s_groups, &span, &blocks);
        scan_bytes = bytes > scan_bytes ? bytes : scan_bytes;
        scan_wins = s_wins.size() > scan_wins ? s_wins.size() : scan_wins;
        scan_groups = s_groups.size() > scan_groups ? s_groups.size() : scan_groups;
    }
    const size_t plane_bytes = src.scan ? scan_bytes : (size_t)cpad * (size_t)lpad;
    uint8_t* d_seq = (uint8_t*)be.alloc(seq_bytes);
    DistTile* d_tiles = (DistTile*)be.alloc(sizeof(DistTile) * tiles.size());
    int8_t* d_planes = src.ranges ? nullptr : (int8_t*)be.alloc(plane_bytes * (size_t)P);
    ScanWindow* d_wins = src.scan ? (ScanWindow*)be.alloc(sizeof(ScanWindow) * scan_wins) : nullptr;
    ScanGroup* d_groups = src.scan ? (ScanGroup*)be.alloc(sizeof(ScanGroup) * scan_groups) : nullptr;
    int64_t* d_starts = src.ranges ? (int64_t*)be.alloc(sizeof(int64_t) * (size_t)cpad) : nullptr;
    int64_t* d_ends = src.ranges ? (int64_t*)be.alloc(sizeof(int64_t) * (size_t)cpad) : nullptr;
    DistSpan* d_spans = src.ranges ? (DistSpan*)be.alloc(sizeof(DistSpan) * (size_t)(cpad / DIST_TILE)) : nullptr;
    int64_t* d_total = (int64_t*)be.alloc(sizeof(int64_t) * (size_t)cpad);
    int32_t* d_bad = (int32_t*)be.alloc(sizeof(int32_t) * (size_t)cpad);
    int32_t* d_sat = model != FNN_DIST_P ? (int32_t*)be.alloc(sizeof(int32_t) * (size_t)cpad) : nullptr;
    double* d_out = on_device ? nullptr : (double*)be.alloc(sizeof(double) * (size_t)(nn * cell) * (size_t)chunk);
    uint32_t* d_max = draw ? (uint32_t*)be.alloc(sizeof(uint32_t)) : src.scan ? (uint32_t*)be.alloc(sizeof(uint32_t) * (size_t)n_chunks) : nullptr;
    if (!d_seq || !d_tiles || (!src.ranges && !d_planes) || (src.ranges && (!d_starts || !d_ends || !d_spans)) || !d_total || !d_bad ||
        (model != FNN_DIST_P && !d_sat) || (!on_device && !d_out) || ((draw || src.scan) && !d_max) || (src.scan && (!d_wins || !d_groups)))
        return fail(FNN_ENOMEM, W + "device allocation failed");
    {
        std::vector<uint8_t> img(seq_bytes, (uint8_t)FNN_SITE_MISSING);
        for (int32_t i = 0; i < n; i++) {
            uint8_t* row = &img[(size_t)i * (size_t)lpad];
            std::memcpy(row, seq + (int64_t)i * lds, (size_t)L);
            if (recoded)
                for (int64_t s = 0; s < L; s++) row[s] = lut[row[s]];
        }
        const uint32_t zero = 0;
        const std::vector<uint32_t> zeros(src.scan ? (size_t)n_chunks : 0, 0u);
        if (be.h2d(d_seq, img.data(), seq_bytes) != FNN_OK || be.h2d(d_tiles, tiles.data(), sizeof(DistTile) * tiles.size()) != FNN_OK ||
            (draw && be.h2d(d_max, &zero, sizeof(zero)) != FNN_OK) || (src.scan && be.h2d(d_max, zeros.data(), sizeof(uint32_t) * zeros.size()) != FNN_OK))
            return fail(FNN_EHIP, W + "upload failed (" + be.err() + ")");
    }
    st.t_upload_s += now_s() - tu0;
    std::vector<int8_t> planes(draw || bounds ? 0 : plane_bytes * (size_t)P);
    std::vector<int64_t> r_starts, r_ends;
    std::vector<DistSpan> r_spans;
    std::vector<int64_t> tot(draw ? 0 : (size_t)cpad);
    std::vector<int32_t> bad((size_t)cpad), sat(model != FNN_DIST_P ? (size_t)cpad : 0);
    std::vector<double> stage(on_device ? 0 : (size_t)(nn * cell) * (size_t)batch), one;
    for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
        const int64_t cnt = batch - b0 < chunk ? batch - b0 : chunk;
        st.chunks++;
        ScanArgs sa{};
        // the planes of this chunk, the rows' totals and their zeroed flags
        if (src.scan) {
            if constexpr (dist_runs_scan<B>::value) {
                // The tables of the chunk's windows and column groups are the uploads; the kernel writes one compact plane and
                // reports the chunk's largest count in a word of its own.  A chunk that needs a second digit (no honest bootstrap
                // has one: a digit holds 127) is the host route's, and so is every chunk under FNN_DIST_FORCE_DIGITS.
                bool host_chunk = dist_force_digits() > 1;
                if (!host_chunk) {
                    const double tu = now_s();
                    int32_t span = 0;
                    int64_t blocks = 0;
                    scan_chunk(src.starts, src.ends, src.per_window, src.seed, b0, cnt, scan_group, s_wins, s_groups, &span, &blocks);
                    if (be.h2d(d_wins, s_wins.data(), sizeof(ScanWindow) * s_wins.size()) != FNN_OK ||
                        be.h2d(d_groups, s_groups.data(), sizeof(ScanGroup) * s_groups.size()) != FNN_OK)
                        return fail(FNN_EHIP, W + "upload failed (" + be.err() + ")");
                    st.t_upload_s += now_s() - tu;
                    sa.planes = d_planes; sa.windows = d_wins; sa.groups = d_groups; sa.first = b0; sa.per_window = src.per_window; sa.lead = src.lead;
                    sa.cnt = cnt; sa.total = d_total; sa.bad = d_bad; sa.sat = d_sat; sa.max_count = d_max + b0 / chunk;
                    double td = 0.0;
                    uint32_t most = 0;
                    if (be.run_draw_ranges(sa, cnt, span, &td) != FNN_OK) return fail(FNN_EHIP, W + "kernel failed (" + be.err() + ")");
                    bst.t_draw_s += td;
                    if (be.d2h(&most, sa.max_count, sizeof(most)) != FNN_OK) return fail(FNN_EHIP, W + "download failed (" + be.err() + ")");
                    cmax = most > cmax ? most : cmax;
                    host_chunk = dist_digits_of(most) > 1;
                    if (!host_chunk) site_blocks += blocks;
                }
                if (host_chunk) {
                    host_chunks++;
                    const int32_t rh = on_device ? scan_host_rows(b0, cnt, D_out + b0 * stride, true, ld, stride)
                                                 : scan_host_rows(b0, cnt, &stage[(size_t)b0 * (size_t)(nn * cell)], false, n, nn * cell);
                    if (rh != FNN_OK) return rh;
                    continue;
                }
            }
        } else if (draw) {
            if constexpr (dist_runs_draw<B>::value) {
                // The kernel writes P planes and reports the largest count of the call so far in one word, the only one of the
                // counts that crosses the bus.  A count that needs more planes than were written (no honest bootstrap has
                // one: P = 1 holds 127) repeats the chunk with as many as it needs; later chunks keep them.
                for (;;) {
                    DrawArgs da{};
                    da.planes = d_planes; da.plane_stride = (int64_t)plane_bytes; da.lpad = lpad; da.L = L; da.digits = P;
                    da.cnt = cnt; da.first = b0; da.lead = src.lead; da.seed = src.seed;
                    da.total = d_total; da.bad = d_bad; da.sat = d_sat; da.max_count = d_max;
                    double td = 0.0;
                    if (be.run_draw(da, cpad, &td) != FNN_OK) return fail(FNN_EHIP, W + "kernel failed (" + be.err() + ")");
                    bst.t_draw_s += td;
                    if (be.d2h(&cmax, d_max, sizeof(cmax)) != FNN_OK) return fail(FNN_EHIP, W + "download failed (" + be.err() + ")");
                    if (dist_digits_of(cmax) <= P) break;
                    P = dist_digits_of(cmax);
                    d_planes = (int8_t*)be.alloc(plane_bytes * (size_t)P);
                    if (!d_planes) return fail(FNN_ENOMEM, W + "device allocation failed");
                }
            }
        } else if (src.ranges) {  // the bounds and the tiles' spans in place of planes
            const double tu = now_s();
            site_blocks += dist_range_chunk(src.starts + b0, src.ends + b0, cnt, cpad, r_starts, r_ends, r_spans);
            std::fill(tot.begin(), tot.end(), (int64_t)0);
            std::fill(bad.begin(), bad.end(), 0);
            for (int64_t b = 0; b < cnt; b++) tot[(size_t)b] = total[(size_t)(b0 + b)];
            if (be.h2d(d_starts, r_starts.data(), sizeof(int64_t) * (size_t)cpad) != FNN_OK || be.h2d(d_ends, r_ends.data(), sizeof(int64_t) * (size_t)cpad) != FNN_OK ||
                be.h2d(d_spans, r_spans.data(), sizeof(DistSpan) * r_spans.size()) != FNN_OK ||
                be.h2d(d_total, tot.data(), sizeof(int64_t) * (size_t)cpad) != FNN_OK || be.h2d(d_bad, bad.data(), sizeof(int32_t) * (size_t)cpad) != FNN_OK ||
                (d_sat && be.h2d(d_sat, bad.data(), sizeof(int32_t) * (size_t)cpad) != FNN_OK))  // (zeros)
                return fail(FNN_EHIP, W + "upload failed (" + be.err() + ")");
            st.t_upload_s += now_s() - tu;
        } else {
            const double tu = now_s();
            std::memset(planes.data(), 0, planes.size());  // (padding: zero counts)
            std::fill(tot.begin(), tot.end(), (int64_t)0);
            std::fill(bad.begin(), bad.end(), 0);
            for (int64_t b = 0; b < cnt; b++) {
                const uint16_t* c = counts + (b0 + b) * ldc;
                tot[(size_t)b] = total[(size_t)(b0 + b)];
                for (int d = 0; d < P; d++) {
                    int8_t* row = &planes[(size_t)d * plane_bytes + (size_t)b * (size_t)lpad];
                    for (int64_t s = 0; s < L; s++) row[s] = dist_digit(c[s], d);
                }
            }
            if (be.h2d(d_planes, planes.data(), planes.size()) != FNN_OK || be.h2d(d_total, tot.data(), sizeof(int64_t) * (size_t)cpad) != FNN_OK ||
                be.h2d(d_bad, bad.data(), sizeof(int32_t) * (size_t)cpad) != FNN_OK ||
                (d_sat && be.h2d(d_sat, bad.data(), sizeof(int32_t) * (size_t)cpad) != FNN_OK))  // (zeros)
                return fail(FNN_EHIP, W + "upload failed (" + be.err() + ")");
            st.t_upload_s += now_s() - tu;
        }
        DistArgs a{};
        a.seq = d_seq; a.lpad = lpad; a.tiles = d_tiles; a.planes = d_planes; a.plane_stride = (int64_t)plane_bytes; a.total = d_total;
        a.n = n; a.cnt = cnt; a.bad = d_bad;
        if (on_device) { a.out = D_out + b0 * stride; a.ld = ld; a.stride = stride; }
        else { a.out = d_out; a.ld = n; a.stride = nn * cell; }
        double tk = 0.0;
        int32_t rk = FNN_OK;
        bool ran = false;
        if constexpr (dist_runs_scan<B>::value) {
            if (src.scan) {  // (the model and pair arguments as below)
                if (pairs) {
                    DistPairs dp{};
                    dp.sat_value = cap ? mp->cap : __builtin_huge_val();
                    dp.deg_value = cap ? mp->cap : -__builtin_huge_val();
                    dp.sat = d_sat;
                    dp.shape = shape;
                    rk = be.run_scan_pairs(model, a, sa, dp, (int64_t)(tiles.size() / DIST_WAVES), (int64_t)s_groups.size(), &tk);
                } else {
                    DistModel dm{};
                    dm.states = mp->states;
                    dm.sat_value = cap ? mp->cap : __builtin_huge_val();
                    dm.sat = d_sat;
                    dm.shape = shape;
                    rk = be.run_scan(model, missing, a, sa, dm, (int64_t)(tiles.size() / DIST_WAVES), (int64_t)s_groups.size(), &tk);
                }
                ran = true;
            }
        }
        if constexpr (dist_runs_ranges<B>::value) {
            if (src.ranges) {  // (the model and pair arguments as below)
                DistRanges dr{};
                dr.starts = d_starts; dr.ends = d_ends; dr.spans = d_spans;
                if (pairs) {
                    DistPairs dp{};
                    dp.sat_value = cap ? mp->cap : __builtin_huge_val();
                    dp.deg_value = cap ? mp->cap : -__builtin_huge_val();
                    dp.sat = d_sat;
                    dp.shape = shape;
                    rk = be.run_ranges_pairs(model, a, dr, dp, (int64_t)(tiles.size() / DIST_WAVES), cnt, &tk);
                } else {
                    DistModel dm{};
                    dm.states = mp->states;
                    dm.sat_value = cap ? mp->cap : __builtin_huge_val();
                    dm.sat = d_sat;
                    dm.shape = shape;
                    rk = be.run_ranges(model, missing, a, dr, dm, (int64_t)(tiles.size() / DIST_WAVES), cnt, &tk);
                }
                ran = true;
            }
        }
        if constexpr (dist_runs_pairs<B>::value) {
            if (pairs && !ran) {  // a degenerate pair is told from a saturated one by the sign of the infinity it leaves
                DistPairs dp{};
                dp.sat_value = cap ? mp->cap : __builtin_huge_val();
                dp.deg_value = cap ? mp->cap : -__builtin_huge_val();
                dp.sat = d_sat;
                dp.shape = shape;
                rk = be.run_pairs(model, P, a, dp, (int64_t)(tiles.size() / DIST_WAVES), cnt, &tk);
            }
        }
        if constexpr (dist_runs_models<B>::value) {
            if (!pairs && !ran) {
                DistModel dm{};
                dm.states = mp->states;
                dm.sat_value = cap ? mp->cap : __builtin_huge_val();
                dm.sat = d_sat;
                dm.shape = shape;
                rk = model != FNN_DIST_P ? be.run_model(model, P, missing, a, dm, (int64_t)(tiles.size() / DIST_WAVES), cnt, &tk)
                                         : be.run(P, missing, a, (int64_t)(tiles.size() / DIST_WAVES), round_up(cnt, (int64_t)DIST_REPS) / DIST_REPS, &tk);
            }
        } else if (!pairs && !ran)
            rk = be.run(P, missing, a, (int64_t)(tiles.size() / DIST_WAVES), round_up(cnt, (int64_t)DIST_REPS) / DIST_REPS, &tk);
        if (rk != FNN_OK) return fail(FNN_EHIP, W + "kernel failed (" + be.err() + ")");
        st.t_kernel_s += tk;
        if (be.d2h(bad.data(), d_bad, sizeof(int32_t) * (size_t)cnt) != FNN_OK || (d_sat && be.d2h(sat.data(), d_sat, sizeof(int32_t) * (size_t)cnt) != FNN_OK))
            return fail(FNN_EHIP, W + "download failed (" + be.err() + ")");
        for (int64_t b = 0; b < cnt; b++) {
            const bool saturated = d_sat && sat[(size_t)b];
            if (saturated && cap) mst.n_saturated_problems++;
            if (!bad[(size_t)b] && !(saturated && sat_fails)) continue;
            // the lowest replicate with an empty pair (NaN entries) or, where that fails the call, a saturated one (+inf): its
            // matrix names the pair
            const size_t span = (size_t)((int64_t)(n - 1) * a.ld + n);
            one.resize(span);
            if (be.d2h(one.data(), a.out + b * a.stride, sizeof(double) * span) != FNN_OK) return fail(FNN_EHIP, W + "download failed (" + be.err() + ")");
            for (int32_t i = 0; i < n; i++)
                for (int32_t j = i + 1; j < n; j++) {
                    const double x = one[(size_t)dist_store_index(i, j, a.ld)];
                    if (x != x) return dist_fail_no_site(W, src.base + b0 + b, i, j);
                    if (sat_fails && x == __builtin_huge_val()) return dist_fail_saturated(W, src.base + b0 + b, i, j);
                    if (sat_fails && x == -__builtin_huge_val()) return dist_fail_degenerate(W, src.base + b0 + b, i, j);
                }
            return fail(FNN_EHIP, W + "replicate " + std::to_string(src.base + b0 + b) + ": flagged without an empty pair");
        }
        if (!on_device && be.d2h(&stage[(size_t)b0 * (size_t)(nn * cell)], d_out, sizeof(double) * (size_t)(nn * cell) * (size_t)cnt) != FNN_OK)
            return fail(FNN_EHIP, W + "download failed (" + be.err() + ")");
    }
    return finish(stage);
}

// the counts entries: the caller's array
template <class B>
int32_t dist_batch_model(B& be, const char* who, const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch,
                         int64_t ldc, const fnn_dist_model* mp, int32_t device, double* D_out, bool on_device, int64_t ld, int64_t stride,
                         fnn_dist_model_stats* stats) {
    DistSource src;
    src.counts = counts;
    src.ldc = ldc;
    fnn_boot_stats bst{};
    const int32_t rc = dist_batch_source(be, who, seq, n, L, lds, src, batch, mp, device, D_out, on_device, ld, stride, &bst);
    if (rc == FNN_OK && stats) *stats = bst.model;
    return rc;
}

// fnn_bootstrap_distances_batch[_device]_f64: up to DRAW_MAX_SITES sites the replicates are drawn on the device, above that
// on the host; the bytes are the same
template <class B>
int32_t dist_bootstrap_batch(B& be, const char* who, const uint8_t* seq, int32_t n, int64_t L, int64_t lds, int64_t batch, uint64_t seed, int64_t lead,
                             const fnn_dist_model* mp, int32_t device, double* D_out, bool on_device, int64_t ld, int64_t stride, fnn_boot_stats* stats) {
    if (lead < 0 || lead > 1 || lead > batch) return fail(FNN_EINVAL, std::string(who) + ": needs 0 <= lead <= 1 and lead <= batch");
    DistSource src;
    src.bootstrap = true;
    src.seed = seed;
    src.lead = lead;
    const int32_t sw = dist_draw_route_switch();
    src.draw_route = sw >= 0 ? sw : (L <= DRAW_MAX_SITES ? FNN_DRAW_DEVICE : FNN_DRAW_HOST);
    return dist_batch_source(be, who, seq, n, L, lds, src, batch, mp, device, D_out, on_device, ld, stride, stats);
}

// fnn_alignment_pair_counts_batch[_device]_i64: the tables in place of a distance (the 8-byte words of the output are int64_t)
template <class B>
int32_t dist_batch_pair_counts(B& be, const char* who, const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch,
                               int64_t ldc, int32_t device, int64_t* F_out, bool on_device, int64_t ld, int64_t stride, fnn_dist_model_stats* stats) {
    DistSource src;
    src.counts = counts;
    src.ldc = ldc;
    src.pair_counts = true;
    fnn_dist_model pm{};
    fnn_boot_stats bst{};
    const int32_t rc = dist_batch_source(be, who, seq, n, L, lds, src, batch, &pm, device, reinterpret_cast<double*>(F_out), on_device, ld, stride, &bst);
    if (rc == FNN_OK && stats) *stats = bst.model;
    return rc;
}

// fnn_bootscan_distances[_device]_f64 and, with m == nullptr and tables, fnn_bootscan_pair_counts[_device]_i64: on the device while
// every window's padded span fits the draw kernel, else through fnn_bootscan_counts on the host; the bytes are the same
template <class B>
int32_t dist_batch_scan(B& be, const char* who, const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts, const int64_t* ends,
                        int64_t windows, int64_t replicates, uint64_t seed, int64_t lead, const fnn_dist_model* mp, bool tables, int32_t device, double* D_out,
                        bool on_device, int64_t ld, int64_t stride, fnn_scan_stats* stats) {
    const std::string W = std::string(who) + ": ";
    if (windows < 0 || replicates < 0) return fail(FNN_EINVAL, W + "needs windows >= 0 and replicates >= 0");
    if (lead < 0 || lead > 1) return fail(FNN_EINVAL, W + "needs 0 <= lead <= 1");
    const int64_t P = replicates + lead;
    if (P > 0 && windows > (((int64_t)1 << 62) / P)) return fail(FNN_EINVAL, W + "too many problems");
    fnn_scan_stats sst{};
    DistSource src;
    src.scan = true;
    src.starts = starts;
    src.ends = ends;
    src.windows = windows;
    src.per_window = P;
    src.seed = seed;
    src.lead = lead;
    src.pair_counts = tables;
    src.scan_stats = &sst;
    fnn_dist_model pm{};
    const int32_t rc = dist_batch_source(be, who, seq, n, L, lds, src, windows * P, tables ? &pm : mp, device, D_out, on_device, ld, stride, &sst.boot);
    sst.n_windows = windows;
    if (rc == FNN_OK && stats) *stats = sst;
    return rc;
}

// fnn_alignment_distances_ranges[_device]_f64 and, with m == nullptr and tables, fnn_alignment_pair_counts_ranges[_device]_i64
template <class B>
int32_t dist_batch_ranges(B& be, const char* who, const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts, const int64_t* ends,
                          int64_t batch, const fnn_dist_model* mp, bool tables, int32_t device, double* D_out, bool on_device, int64_t ld, int64_t stride,
                          fnn_range_stats* stats) {
    fnn_range_stats rst{};
    DistSource src;
    src.ranges = true;
    src.starts = starts;
    src.ends = ends;
    src.pair_counts = tables;
    src.range_stats = &rst;
    fnn_dist_model pm{};
    fnn_boot_stats bst{};
    const int32_t rc = dist_batch_source(be, who, seq, n, L, lds, src, batch, tables ? &pm : mp, device, D_out, on_device, ld, stride, &bst);
    rst.model = bst.model;
    if (rc == FNN_OK && stats) *stats = rst;
    return rc;
}

// the p-distance entries: FNN_DIST_P or nothing
template <class B>
int32_t dist_batch(B& be, const char* who, const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch,
                   int64_t ldc, int32_t model, int32_t device, double* D_out, bool on_device, int64_t ld, int64_t stride, fnn_dist_stats* stats) {
    if (n > 0 && L > 0 && batch >= 0 && model != FNN_DIST_P) return fail(FNN_EINVAL, std::string(who) + ": unknown model");
    fnn_dist_model pm{};
    fnn_dist_model_stats mst{};
    const int32_t rc = dist_batch_model(be, who, seq, n, L, lds, counts, batch, ldc, &pm, device, D_out, on_device, ld, stride, &mst);
    if (rc == FNN_OK && stats) *stats = mst.base;
    return rc;
}

}  // namespace fnn
#endif

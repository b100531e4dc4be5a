// fnn_dist_ranges.h -- alignment distances over site ranges: the per-lane steps of k_dist_ranges and
// k_dist_ranges_pairs (fnn_dist.hip), shared with the CPU driver (tests/emu/fnn_dist_ranges_emu.cpp).  Included by fnn_dist.h,
// whose walk, lane maps, A operands, epilogues and host side it uses.
//
// Problem b is the alignment restricted to the sites [start_b, end_b): a gene of a concatenated alignment, a window of a scan.
// Its row of the counts would be the 0/1 indicator of the range, so the B operand (sites x problems) of a lane is sixteen 0/1
// bytes made from the range's two bounds: no counts exist, no plane is stored, and there is one digit.  A WINDOW TILE is 16
// consecutive ranges in the caller's order, one N-tile of the instruction; its SPAN [lo, hi) is the run of 64-site blocks
// that some range of the tile touches, written by the host (as the pair-tile table is: the kernel decodes nothing).  A wave
// takes one pair tile and one window tile and walks that tile's span: the walk is as long as the ranges and not as the
// alignment.
//
// One window tile per wave is a measured choice (profiles/r20/tiles_*.jsonl).  A variant that took 4 tiles
// (2 for the tables), walked the union of their spans and reused a block's A fragments for every tile whose span held the
// block was 1.02 - 4.2 x slower on windows of 1000 sites every 250 - consecutive tiles hardly overlap there, and the wave holds 4
// times the accumulators - and between 0.77 and 1.16 x on windows every 8 sites, where they overlap almost wholly; the table
// kernels, at 256 registers and one wave per SIMD, lost at both (1.9 - 2.3 x, 1.4 - 1.5 x).  It is gone.
#ifndef FNN_DIST_RANGES_H
#define FNN_DIST_RANGES_H

namespace fnn {

struct DistSpan { int32_t lo, hi; };            // sites, multiples of DIST_K, 0 <= lo <= hi <= lpad; lo == hi: nothing to walk
struct DistRangeLane { int32_t start, end; };   // the bounds of a lane's column (L < 2^31 / 127: they fit)

// what the range kernels need beyond DistArgs (whose planes they do not read)
struct DistRanges {
    const int64_t* starts;   // of the chunk's problems, padded to a multiple of DIST_REPS with start = end = 0: such a column
    const int64_t* ends;     // multiplies by zero, as a padded row of the planes does
    const DistSpan* spans;   // one per window tile of the padded chunk
};

// ---- the B operand of one lane from its column's bounds
// b0: the first problem of the TILE.  Read once, before the site loop.
FNN_HD DistRangeLane dist_lane_range(const DistRanges& r, int64_t b0, int lane) {
    const int64_t b = b0 + dist_lane_rc(lane);
    return DistRangeLane{(int32_t)r.starts[b], (int32_t)r.ends[b]};
}
FNN_HD int32_t dist_clamp(int32_t x, int32_t hi) { return x < 0 ? 0 : (x > hi ? hi : x); }
FNN_HD uint32_t dist_low_bytes(int32_t k) { return (uint32_t)(((uint64_t)1 << (8 * k)) - 1); }  // bytes 0 ... k - 1 all ones, 0 <= k <= 4
// byte t is 1 iff start <= s + 16 (lane >> 4) + t < end: with the two offsets clamped to 0 ... 16, the bytes from..to - 1
FNN_HD DistFrag dist_lane_b_range(const DistRangeLane& rl, int lane, int64_t s) {
    const int32_t k0 = (int32_t)s + dist_lane_k(lane);
    const int32_t from = dist_clamp(rl.start - k0, 16), to = dist_clamp(rl.end - k0, 16);
    DistFrag f;
    for (int q = 0; q < 4; q++) f.w[q] = 0x01010101u & dist_low_bytes(dist_clamp(to - 4 * q, 4)) & ~dist_low_bytes(dist_clamp(from - 4 * q, 4));
    return f;
}

// ---- host side: the bounds and spans of one chunk (cnt problems from starts / ends, padded to cpad); returns the blocks walked
inline int64_t dist_range_chunk(const int64_t* starts, const int64_t* ends, int64_t cnt, int64_t cpad, std::vector<int64_t>& s_out,
                                std::vector<int64_t>& e_out, std::vector<DistSpan>& spans) {
    s_out.assign((size_t)cpad, 0);
    e_out.assign((size_t)cpad, 0);
    spans.assign((size_t)(cpad / DIST_TILE), DistSpan{0, 0});
    int64_t blocks = 0;
    for (int64_t b = 0; b < cnt; b++) {
        s_out[(size_t)b] = starts[b];
        e_out[(size_t)b] = ends[b];
        if (starts[b] == ends[b]) continue;
        DistSpan& sp = spans[(size_t)(b / DIST_TILE)];
        const int32_t lo = (int32_t)(starts[b] / DIST_K * DIST_K), hi = (int32_t)round_up(ends[b], (int64_t)DIST_K);
        if (sp.hi == sp.lo) sp = DistSpan{lo, hi};
        else {
            sp.lo = lo < sp.lo ? lo : sp.lo;
            sp.hi = hi > sp.hi ? hi : sp.hi;
        }
    }
    for (const DistSpan& sp : spans) blocks += (sp.hi - sp.lo) / DIST_K;
    return blocks;
}

}  // namespace fnn
#endif

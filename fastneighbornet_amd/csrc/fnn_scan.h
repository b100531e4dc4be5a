// fnn_scan.h -- bootscan: bootstrap replicates inside every site range: the per-lane steps of
// k_draw_ranges, k_dist_scan and k_dist_scan_pairs (fnn_dist.hip), shared with the CPU driver (tests/emu/fnn_bootscan_emu.cpp).
// Included by fnn_dist.h, whose walk, lane maps, A operands, epilogues, draw steps and host side it uses.
//
// A call has `windows` ranges [start_w, end_w) and P = replicates + lead problems per window, window-major: problem p is
// q = p % P of window w = p / P.  q < lead is the window's original data, counts[s] = [start_w <= s < end_w]; otherwise it is
// replicate r = q - lead of a bootstrap of the window alone: with width = end_w - start_w and seed_w = splitmix64_at(seed, w),
// draw k = 0 ... width - 1 is x = splitmix64_at(seed_w, r width + k) and increments site start_w + floor(x width / 2^64) -
// row r of fnn_bootstrap_counts(width, replicates, seed_w) placed at column start_w.
//
// The digit plane of such a row is zero outside the window's padded span [lo, hi) = [floor64(start_w), ceil64(end_w)), so only
// that part exists: a COMPACT row of hi - lo bytes, made by one workgroup of k_draw_ranges from a histogram in LDS (the steps
// of fnn_draw.h over the span) and read by the distance kernel at s - lo.  A COLUMN GROUP is up to 16 RT consecutive rows of
// one window - never of two: all its rows share [lo, hi) and a wave walks exactly that span.  The host writes one table entry
// per window and per group of a chunk (as the pair-tile table: the kernels decode nothing but p / P); a chunk boundary may fall
// inside a window.  Rows of a group behind its last problem do not exist: their lanes read the group's last row again and
// store nothing (the epilogues' own bound, set to the group's end).  One digit: a chunk whose largest count exceeds 127 goes
// through the counts entries on the host's rows (fnn_dist.h).
#ifndef FNN_SCAN_H
#define FNN_SCAN_H

namespace fnn {

// The counts buffer of the host route holds at most this many bytes at a time: at 10^6 sites the counts of a chunk, and not
// its output, are what limits it (2 bytes x L per problem against 8 n^2).
constexpr int64_t SCAN_COUNTS_BYTES = (int64_t)256 << 20;

struct ScanWindow {          // one window of a chunk
    int32_t start, end;      // sites
    int32_t lo, hi;          // floor64(start), ceil64(end): the compact rows are hi - lo bytes
    int64_t plane;           // byte offset, in the compact planes, of the row of the window's first problem IN THIS CHUNK
    int64_t row0;            // chunk row of that problem
    uint64_t seed;           // seed_w
};
struct ScanGroup {           // up to 16 RT consecutive rows of one window
    int32_t lo, hi;          // of its window
    int64_t plane;           // byte offset of its first row
    int32_t row0, rows;      // chunk row of its first row; 1 <= rows <= 16 RT problems
};
// what the three kernels need beyond DistArgs (whose planes they do not read; out, total, bad index chunk rows as ever)
struct ScanArgs {
    int8_t* planes;          // the chunk's compact rows, one digit
    const ScanWindow* windows;
    const ScanGroup* groups;
    int64_t first;           // chunk row b is problem first + b of the call
    int64_t per_window;      // P
    int64_t lead;
    int64_t cnt;             // rows of the chunk (all of them problems)
    int64_t* total;          // total[b] = width of the row's window
    int32_t* bad;            // zeroed
    int32_t* sat;            // zeroed; may be null
    uint32_t* max_count;     // one word: the largest count of the chunk
};
constexpr int32_t scan_rt(bool pairs) { return pairs ? dist_pairs_rt(1) : DIST_RT; }

FNN_HD const ScanWindow& scan_row_window(const ScanArgs& a, int64_t row) {
    return a.windows[(a.first + row) / a.per_window - a.first / a.per_window];
}
FNN_HD int8_t* scan_row_plane(const ScanArgs& a, const ScanWindow& w, int64_t row) { return a.planes + w.plane + (row - w.row0) * (int64_t)(w.hi - w.lo); }

// ---- k_draw_ranges: the steps of fnn_draw.h over the window's span.  Step 1 is draw_lane_zero(hist, hi - lo, ...).
// step 2: the row's draws, or every site of the window once for a lead row
FNN_HD void scan_lane_count(const ScanArgs& a, const ScanWindow& w, uint32_t* hist, int64_t row, int tid, int nt) {
    const int64_t q = (a.first + row) % a.per_window, width = w.end - w.start;
    const uint64_t at = (uint64_t)(q - a.lead) * (uint64_t)width, off = (uint64_t)(w.start - w.lo);
    for (int64_t k = tid; k < width; k += nt) {
        const uint64_t site = off + (q < a.lead ? (uint64_t)k : draw_site(splitmix64_at(w.seed, at + (uint64_t)k), (uint64_t)width));
        FNN_DRAW_ADD(&hist[site >> 1], 1u << (16 * (uint32_t)(site & 1)));
    }
}
// step 3: the compact row, hi - lo bytes in 16-byte stores, the zero bytes of [lo, start) and [end, hi) among them.  Returns
// the largest count the lane has seen (a count above 127 leaves a wrong byte: the host repeats such a chunk another way).
FNN_HD uint32_t scan_lane_plane(const ScanArgs& a, const ScanWindow& w, const uint32_t* hist, int64_t row, int tid, int nt) {
    uint32_t most = 0;
    int8_t* out = scan_row_plane(a, w, row);
    for (int64_t g = tid; g < (w.hi - w.lo) / 16; g += nt) {
        const DistFrag c[2] = {dist_load16(hist + 8 * g), dist_load16(hist + 8 * g + 4)};  // 16 counters
        DistFrag f;
        for (int q = 0; q < 4; q++) {
            uint32_t bytes = 0;
            for (int t = 0; t < 4; t++) {
                const int s = 4 * q + t;
                const uint32_t count = (c[s >> 3].w[(s >> 1) & 3] >> (16 * (s & 1))) & 0xffffu;
                most = count > most ? count : most;
                bytes |= (uint32_t)(uint8_t)dist_digit((uint16_t)count, 0) << (8 * t);
            }
            f.w[q] = bytes;
        }
        draw_store16(out + 16 * g, f);
    }
    return most;
}
// what the distance kernel reads of the row beside its plane
FNN_HD void scan_lane_row_words(const ScanArgs& a, const ScanWindow& w, int64_t row, int tid) {
    if (tid != 0) return;
    a.total[row] = w.end - w.start;
    a.bad[row] = 0;
    if (a.sat) a.sat[row] = 0;
}

// ---- k_dist_scan, k_dist_scan_pairs: the B operand of one lane, 16 bytes of its column's compact row at s - lo.  rt: the
// tile of the group; a column behind the group's last row reads that last row (its products are never stored).
FNN_HD const int8_t* scan_lane_row(const ScanArgs& a, const ScanGroup& g, int rt, int lane) {
    const int32_t col = DIST_TILE * rt + dist_lane_rc(lane), r = col < g.rows ? col : g.rows - 1;
    return a.planes + g.plane + (int64_t)r * (int64_t)(g.hi - g.lo) + dist_lane_k(lane);
}
FNN_HD DistFrag scan_lane_b(const int8_t* row, const ScanGroup& g, int32_t s) { return dist_load16(row + (s - g.lo)); }
// the epilogues' arguments for one group: rows behind the group's last are not stored
FNN_HD DistArgs scan_group_args(const DistArgs& a, const ScanGroup& g) {
    DistArgs al = a;
    al.cnt = (int64_t)g.row0 + g.rows;
    return al;
}

// ---- host side
inline int32_t scan_floor64(int64_t s) { return (int32_t)(s / DIST_K * DIST_K); }
inline int32_t scan_ceil64(int64_t e) { return (int32_t)round_up(e, (int64_t)DIST_K); }

// The tables of one chunk: problems b0 ... b0 + cnt - 1 of a call with P problems per window, groups of `group_rows` rows.
// Returns the bytes of the chunk's compact planes; *max_span: the widest span; *blocks: the 64-site blocks walked, per tile of
// 16 rows.
inline int64_t scan_chunk(const int64_t* starts, const int64_t* ends, int64_t P, uint64_t seed, int64_t b0, int64_t cnt, int32_t group_rows,
                          std::vector<ScanWindow>& wins, std::vector<ScanGroup>& groups, int32_t* max_span, int64_t* blocks) {
    wins.clear();
    groups.clear();
    int64_t bytes = 0;
    *max_span = 0;
    *blocks = 0;
    for (int64_t w = b0 / P; w <= (b0 + cnt - 1) / P; w++) {
        const int64_t p_lo = w * P > b0 ? w * P : b0, p_hi = (w + 1) * P < b0 + cnt ? (w + 1) * P : b0 + cnt;  // the window's problems in the chunk
        ScanWindow sw{};
        sw.start = (int32_t)starts[w]; sw.end = (int32_t)ends[w];
        sw.lo = scan_floor64(starts[w]); sw.hi = scan_ceil64(ends[w]);
        sw.plane = bytes; sw.row0 = p_lo - b0; sw.seed = splitmix64_at(seed, (uint64_t)w);
        wins.push_back(sw);
        const int32_t span = sw.hi - sw.lo;
        *max_span = span > *max_span ? span : *max_span;
        for (int64_t r = 0; r < p_hi - p_lo; r += group_rows) {
            ScanGroup g{};
            g.lo = sw.lo; g.hi = sw.hi;
            g.plane = bytes + r * span;
            g.row0 = (int32_t)(sw.row0 + r);
            g.rows = (int32_t)(p_hi - p_lo - r < group_rows ? p_hi - p_lo - r : group_rows);
            groups.push_back(g);
            *blocks += (int64_t)((g.rows + DIST_TILE - 1) / DIST_TILE) * (span / DIST_K);
        }
        bytes += (p_hi - p_lo) * span;
    }
    return bytes;
}

// fnn_bootscan_counts: rows first ... first + count - 1 of the definition above
inline int32_t dist_bootscan_counts(const char* who, int64_t L, const int64_t* starts, const int64_t* ends, int64_t windows, int64_t replicates,
                                    int64_t lead, uint64_t seed, int64_t first, int64_t count, uint16_t* counts_out) {
    const std::string W = std::string(who) + ": ";
    if (L <= 0 || windows < 0 || replicates < 0) return fail(FNN_EINVAL, W + "needs L > 0, windows >= 0 and replicates >= 0");
    if (lead < 0 || lead > 1) return fail(FNN_EINVAL, W + "needs 0 <= lead <= 1");
    const int64_t P = replicates + lead;
    if (P > 0 && windows > (((int64_t)1 << 62) / P)) return fail(FNN_EINVAL, W + "too many problems");
    if (windows > 0 && (!starts || !ends)) return fail(FNN_EINVAL, W + "NULL argument");
    for (int64_t w = 0; w < windows; w++)
        if (starts[w] < 0 || starts[w] > ends[w] || ends[w] > L)
            return fail(FNN_EINVAL, W + "window " + std::to_string(w) + ": needs 0 <= start <= end <= L, got [" + std::to_string(starts[w]) + ", " +
                                        std::to_string(ends[w]) + ")");
    if (first < 0 || count < 0 || first > windows * P || count > windows * P - first)
        return fail(FNN_EINVAL, W + "needs 0 <= first, 0 <= count and first + count <= windows * (replicates + lead)");
    if (count == 0) return FNN_OK;
    if (!counts_out) return fail(FNN_EINVAL, W + "NULL argument");
    std::vector<uint32_t> row;
    for (int64_t p = first; p < first + count; p++) {
        const int64_t w = p / P, q = p % P, width = ends[w] - starts[w];
        uint16_t* out = counts_out + (p - first) * L;
        std::memset(out, 0, sizeof(uint16_t) * (size_t)L);
        if (q < lead) {
            for (int64_t s = starts[w]; s < ends[w]; s++) out[s] = 1;
            continue;
        }
        row.assign((size_t)width, 0u);
        const uint64_t seed_w = splitmix64_at(seed, (uint64_t)w), at = (uint64_t)(q - lead) * (uint64_t)width;
        for (int64_t k = 0; k < width; k++) row[(size_t)draw_site(splitmix64_at(seed_w, at + (uint64_t)k), (uint64_t)width)]++;
        for (int64_t s = 0; s < width; s++) {
            if (row[(size_t)s] > 65535u)
                return fail(FNN_EINVAL, W + "problem " + std::to_string(p) + ": a site was drawn more than 65535 times");
            out[starts[w] + s] = (uint16_t)row[(size_t)s];
        }
    }
    return FNN_OK;
}

}  // namespace fnn
#endif

// fnn_dist_ranges_emu_main.cpp -- TEST INFRASTRUCTURE: stand-alone program over the CPU driver of the alignment distances over
// site ranges (fnn_dist_ranges_emu.cpp), meant to be built with -fsanitize=address,undefined, as fnn_dist_gamma_emu_main.cpp is
// for the gamma rates.
//
// Runs the cases of tests/dist_ranges_common.py - the range operand at every k, grids of windows under every model without and
// with missing bytes, far-apart, nested and repeated ranges in both orders, a long walk, the failures, layouts and chunks.
// Every range call is compared with the driver's counts entry on the 0/1 counts of the
// ranges, built here: the same status, the same message behind the entry's name, the same words in the whole output array (whose
// bits are tests/test_dist_ranges_emu.py's business); n_site_blocks is compared with a plain loop over its definition.  The
// caller's arrays are heap blocks of EXACTLY the declared sizes, the outputs filled with 0xFF bytes first; the output's padding -
// and after a failure of the host entry all of it - must still hold those bytes.  Exit status 0: all well.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/fastnn.h"

extern "C" {
const char* emur_last_error(void);
int32_t emur_alignment_distances_ranges_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts, const int64_t* ends, int64_t batch,
                                            const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride, fnn_range_stats* stats);
int32_t emur_alignment_distances_ranges_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts, const int64_t* ends,
                                                   int64_t batch, const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                   fnn_range_stats* stats);
int32_t emur_alignment_pair_counts_ranges_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts, const int64_t* ends, int64_t batch,
                                              int32_t device, int64_t* F_out, int64_t ld, int64_t stride, fnn_range_stats* stats);
int32_t emur_alignment_pair_counts_ranges_device_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts, const int64_t* ends,
                                                     int64_t batch, int32_t device, int64_t* F_out, int64_t ld, int64_t stride, fnn_range_stats* stats);
int32_t emur_alignment_distances_model_batch_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch, int64_t ldc,
                                                 const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                 fnn_dist_model_stats* stats);
int32_t emur_alignment_distances_model_batch_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch,
                                                        int64_t ldc, const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                        fnn_dist_model_stats* stats);
int32_t emur_alignment_pair_counts_batch_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch, int64_t ldc,
                                             int32_t device, int64_t* F_out, int64_t ld, int64_t stride, fnn_dist_model_stats* stats);
int32_t emur_alignment_pair_counts_batch_device_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch,
                                                    int64_t ldc, int32_t device, int64_t* F_out, int64_t ld, int64_t stride, fnn_dist_model_stats* stats);
}

static uint64_t splitmix64(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

typedef std::vector<std::pair<int64_t, int64_t>> Ranges;
const int TABLES = 100;  // in place of a model: the 4 x 4 tables

struct Align {
    int n, L;
    int64_t lds;
    std::vector<uint8_t> bytes;  // (n - 1) * lds + L: copied to a heap block of exactly that size for every call
};

// about 10 % divergence from a common ancestor; missing_pct per cent of the bytes 255; the padding holds states, too
static Align make_align(int n, int L, int64_t lds, int missing_pct, uint64_t seed) {
    Align al{n, L, lds, std::vector<uint8_t>((size_t)((int64_t)(n - 1) * lds + L))};
    uint64_t s = seed;
    for (uint8_t& x : al.bytes) x = (uint8_t)"ACGT"[splitmix64(s) & 3];
    std::vector<uint8_t> base((size_t)L);
    for (int k = 0; k < L; k++) base[(size_t)k] = (uint8_t)"ACGT"[splitmix64(s) & 3];
    for (int i = 0; i < n; i++)
        for (int k = 0; k < L; k++) {
            uint8_t v = splitmix64(s) % 100 < 10 ? (uint8_t)"ACGT"[splitmix64(s) & 3] : base[(size_t)k];
            if ((int)(splitmix64(s) % 100) < missing_pct) v = FNN_SITE_MISSING;
            al.bytes[(size_t)((int64_t)i * lds + k)] = v;
        }
    return al;
}

static Ranges windows(int L, int width, int step) {
    Ranges r;
    for (int s = 0; s + width <= L; s += step) r.push_back({s, s + width});
    return r;
}

static int64_t tile_blocks(const Ranges& r, size_t from, size_t to) {
    int64_t total = 0;
    for (size_t k = from; k < to; k += 16) {
        int64_t lo = -1, hi = -1;
        for (size_t b = k; b < to && b < k + 16; b++) {
            if (r[b].first == r[b].second) continue;
            if (lo < 0 || r[b].first < lo) lo = r[b].first;
            if (r[b].second > hi) hi = r[b].second;
        }
        if (lo >= 0) total += (hi + 63) / 64 - lo / 64;
    }
    return total;
}

static std::string tail_of(const char* msg) {
    const std::string m = msg ? msg : "";
    const size_t at = m.find(": ");
    return at == std::string::npos ? m : m.substr(at + 2);
}

struct Call {
    int model = FNN_DIST_P;
    double shape = 0.0;          // > 0: gamma rates
    int policy = FNN_DIST_SAT_FAIL;
    int64_t ld = 0, stride = 0;  // 0: dense
    bool in_place = false;
    int chunk = 0;               // FNN_BATCH_CHUNK, 0: none
    int expect = FNN_OK;         // the status both entries must return
    const char* names = nullptr; // what the message must hold when the call fails
};

static int runs = 0;

// one range call against the counts entry on the ranges' 0/1 counts; `one_site`: the ranges [s, s + 1) come first, L of them
static int run(const char* tag, const Align& al, const Ranges& r, const Call& c, bool one_site = false) {
    const int n = al.n, L = al.L;
    const int64_t B = (int64_t)r.size(), cell = c.model == TABLES ? 16 : 1;
    const int64_t ld = c.ld ? c.ld : n, stride = c.stride ? c.stride : cell * n * ld;
    const size_t out_words = (size_t)((B - 1) * stride + ((int64_t)(n - 1) * ld + n) * cell);
    uint8_t* seq = (uint8_t*)std::malloc(al.bytes.size());
    int64_t* starts = (int64_t*)std::malloc(sizeof(int64_t) * (size_t)B);
    int64_t* ends = (int64_t*)std::malloc(sizeof(int64_t) * (size_t)B);
    uint16_t* counts = (uint16_t*)std::malloc(sizeof(uint16_t) * (size_t)B * (size_t)L);
    uint64_t* out = (uint64_t*)std::malloc(8 * out_words);
    uint64_t* want = (uint64_t*)std::malloc(8 * out_words);
    fnn_dist_model_rates* mr = (fnn_dist_model_rates*)std::malloc(sizeof(fnn_dist_model_rates));
    if (!seq || !starts || !ends || !counts || !out || !want || !mr) return 1;
    std::memcpy(seq, al.bytes.data(), al.bytes.size());
    for (int64_t b = 0; b < B; b++) {
        starts[b] = r[(size_t)b].first;
        ends[b] = r[(size_t)b].second;
        for (int k = 0; k < L; k++) counts[b * L + k] = (uint16_t)(k >= starts[b] && k < ends[b] ? 1 : 0);
    }
    std::memset(out, 0xFF, 8 * out_words);
    std::memset(want, 0xFF, 8 * out_words);
    std::memset(mr, 0, sizeof(*mr));
    mr->base.model = c.model == TABLES ? 0 : c.model;
    mr->base.states = 4;
    mr->base.on_saturation = c.policy;
    mr->base.cap = c.policy == FNN_DIST_SAT_CAP ? 12.5 : 0.0;
    mr->base.reserved = c.shape > 0.0 ? FNN_DIST_RATES_GAMMA : FNN_DIST_RATES_EQUAL;
    mr->shape = c.shape;
    if (c.chunk) setenv("FNN_BATCH_CHUNK", std::to_string(c.chunk).c_str(), 1); else unsetenv("FNN_BATCH_CHUNK");

    fnn_dist_model_stats cst{};
    const int32_t rc_counts = c.model == TABLES
        ? (c.in_place ? emur_alignment_pair_counts_batch_device_i64 : emur_alignment_pair_counts_batch_i64)(seq, n, L, al.lds, counts, B, L, 0, (int64_t*)want, ld, stride, &cst)
        : (c.in_place ? emur_alignment_distances_model_batch_device_f64 : emur_alignment_distances_model_batch_f64)(seq, n, L, al.lds, counts, B, L, &mr->base, 0,
                                                                                                                  (double*)want, ld, stride, &cst);
    const std::string msg_counts = tail_of(emur_last_error());
    int bad = 0;
    do {  // (left at the first finding)
        std::memset(out, 0xFF, 8 * out_words);
        fnn_range_stats st{};
        const int32_t rc = c.model == TABLES
            ? (c.in_place ? emur_alignment_pair_counts_ranges_device_i64 : emur_alignment_pair_counts_ranges_i64)(seq, n, L, al.lds, starts, ends, B, 0, (int64_t*)out, ld, stride, &st)
            : (c.in_place ? emur_alignment_distances_ranges_device_f64 : emur_alignment_distances_ranges_f64)(seq, n, L, al.lds, starts, ends, B, &mr->base, 0,
                                                                                                              (double*)out, ld, stride, &st);
        runs++;
        if (rc != c.expect || rc_counts != c.expect) {
            std::fprintf(stderr, "%s: status %d, the counts entry's %d, expected %d (%s)\n", tag, rc, rc_counts, c.expect, emur_last_error());
            bad = 1;
            break;
        }
        if (rc != FNN_OK) {
            const std::string msg = tail_of(emur_last_error());
            if (msg != msg_counts || (c.names && msg.find(c.names) == std::string::npos)) {
                std::fprintf(stderr, "%s: message '%s', the counts entry's '%s', expected to name %s\n", tag, msg.c_str(), msg_counts.c_str(),
                             c.names ? c.names : "-");
                bad = 1;
            }
            for (size_t k = 0; k < out_words && !bad && !c.in_place; k++)
                if (out[k] != ~0ull) { std::fprintf(stderr, "%s: the output was written although the call failed\n", tag); bad = 1; }
            break;
        }
        if (std::memcmp(out, want, 8 * out_words) != 0) {
            size_t k = 0;
            while (out[k] == want[k]) k++;
            std::fprintf(stderr, "%s: word %zu is %016llx, the counts entry's %016llx\n", tag, k, (unsigned long long)out[k], (unsigned long long)want[k]);
            bad = 1;
            break;
        }
        int64_t blocks = 0;
        const size_t per = c.chunk ? (size_t)c.chunk : r.size();
        for (size_t from = 0; from < r.size(); from += per) blocks += tile_blocks(r, from, from + per < r.size() ? from + per : r.size());
        const int64_t dense = (B + 15) / 16 * ((L + 63) / 64);
        if (st.n_site_blocks != blocks || st.n_site_blocks_dense != dense || st.model.base.digit_passes != 1 ||
            st.model.n_saturated_problems != cst.n_saturated_problems || st.model.base.has_missing != cst.base.has_missing || st.model.base.chunks != cst.base.chunks) {
            std::fprintf(stderr, "%s: stats: %lld blocks (expected %lld), %lld dense (%lld), %d passes, %lld saturated (%lld)\n", tag,
                         (long long)st.n_site_blocks, (long long)blocks, (long long)st.n_site_blocks_dense, (long long)dense, st.model.base.digit_passes,
                         (long long)st.model.n_saturated_problems, (long long)cst.n_saturated_problems);
            bad = 1;
            break;
        }
        for (int s = 0; one_site && s < L && !bad; s++)
            for (int i = 0; i < n; i++)
                for (int j = 0; j < n; j++) {
                    const double x = seq[(size_t)((int64_t)i * al.lds + s)] != seq[(size_t)((int64_t)j * al.lds + s)] ? 1.0 : 0.0;
                    double got;
                    std::memcpy(&got, &out[(size_t)((int64_t)s * stride + (int64_t)i * ld + j)], 8);
                    if (std::memcmp(&got, &x, 8) != 0) { std::fprintf(stderr, "%s: window %d entry (%d, %d) is %g\n", tag, s, i, j, got); bad = 1; }
                }
    } while (false);
    unsetenv("FNN_BATCH_CHUNK");
    std::free(seq); std::free(starts); std::free(ends); std::free(counts); std::free(out); std::free(want); std::free(mr);
    return bad;
}

int main() {
    const int P = FNN_DIST_P, J = FNN_DIST_JC69, K = FNN_DIST_K2P, E = FNN_DIST_F81, F = FNN_DIST_F84, T = FNN_DIST_TN93, D = FNN_DIST_LOGDET;
    // 1. the range operand at every k: n = 6, L = 130, B = 135
    {
        const Align al = make_align(6, 130, 130, 0, 9101);
        Ranges r;
        for (int s = 0; s < 130; s++) r.push_back({s, s + 1});
        for (auto x : Ranges{{15, 17}, {63, 65}, {127, 129}, {0, 130}, {129, 130}}) r.push_back(x);
        if (run("operand", al, r, Call{}, true)) return 1;
    }
    // 2. grids of windows under every model, without and with missing bytes.  Under SAT_CAP a pair that the generated alignment
    // happens to saturate is capped by both entries alike; an empty pair fails both alike.
    const int grids[3][4] = {{17, 200, 96, 8}, {33, 330, 128, 6}, {6, 1000, 150, 25}};
    for (int g = 0; g < 3; g++)
        for (int missing = 0; missing < 2; missing++) {
            const int n = grids[g][0], L = grids[g][1];
            const Align al = make_align(n, L, L, missing ? 2 : 0, 9110 + 2 * (uint64_t)g + (uint64_t)missing);
            Ranges r = windows(L, grids[g][2], grids[g][3]);
            for (auto x : Ranges{{0, L}, {L - 70, L}, {3, 93}, {L - 100, L}}) r.push_back(x);
            const struct { int model; double shape; } models[] = {{P, 0}, {J, 0}, {K, 0}, {E, 0}, {F, 0}, {T, 0}, {D, 0}, {K, 0.5}, {T, 0.5}, {TABLES, 0}};
            for (const auto& m : models) {
                if (g == 1 && !(m.model == P || (m.model == K && m.shape == 0) || (m.model == T && m.shape > 0) || m.model == TABLES)) continue;  // (the largest grid: one model of each kernel)
                Call c;
                c.model = m.model; c.shape = m.shape; c.policy = FNN_DIST_SAT_CAP;
                char tag[64];
                std::snprintf(tag, sizeof(tag), "grid %d missing=%d model=%d shape=%g", g, missing, m.model, m.shape);
                if (run(tag, al, r, c)) return 1;
            }
        }
    // 3. order and spans: far apart, nested and repeated within one window tile and across two; then sorted
    {
        const Align al = make_align(5, 1000, 1000, 0, 9120);
        Ranges r{{0, 3}, {997, 1000}, {500, 564}, {0, 1000}, {500, 564}, {510, 520}};
        uint64_t s = 9121;
        for (int k = 0; k < 14; k++) { const int64_t at = 50 * (int64_t)(splitmix64(s) % 19); r.push_back({at, at + 100}); }
        if (run("order", al, r, Call{})) return 1;
        Ranges sorted = r;
        for (size_t i = 1; i < sorted.size(); i++)
            for (size_t j = i; j > 0 && sorted[j] < sorted[j - 1]; j--) std::swap(sorted[j], sorted[j - 1]);
        if (run("order, sorted", al, sorted, Call{})) return 1;
        if (!(tile_blocks(sorted, 0, sorted.size()) < tile_blocks(r, 0, r.size()))) { std::fprintf(stderr, "order: sorting did not shorten the walk\n"); return 1; }
    }
    // 4. a long walk: offsets beyond one chunk of 64 blocks, spans that start far from 0
    {
        // (the counts entry walks all 313 blocks for every window: the last 61 windows only, and three taxa)
        const Align al = make_align(3, 20000, 20000, 2, 9130);
        Call c;
        c.model = K; c.policy = FNN_DIST_SAT_CAP;
        Ranges r = windows(20000, 500, 125);
        r.erase(r.begin(), r.end() - 61);
        if (run("long walk", al, r, c)) return 1;
    }
    // 5. failures
    {
        const Align full = make_align(5, 200, 200, 0, 9140);
        Call c;
        c.expect = FNN_EINVAL; c.names = "(2, 0, 1)";
        if (run("empty range, no missing byte", full, Ranges{{0, 200}, {10, 90}, {50, 50}, {100, 180}, {20, 20}}, c)) return 1;
        Align al = make_align(5, 200, 200, 2, 9141);
        for (int k = 100; k < 140; k++) al.bytes[(size_t)(1 * 200 + k)] = FNN_SITE_MISSING;
        for (int k = 140; k < 180; k++) al.bytes[(size_t)(3 * 200 + k)] = FNN_SITE_MISSING;
        for (int model : {P, J, K, T}) {
            Call e;
            e.model = model; e.expect = FNN_EINVAL; e.names = "(3, 1, 3)";
            if (run("empty pair below an empty range", al, Ranges{{0, 200}, {10, 90}, {90, 190}, {100, 180}, {20, 20}, {0, 100}}, e)) return 1;
            e.in_place = true;
            if (run("empty pair below an empty range, in place", al, Ranges{{0, 200}, {10, 90}, {90, 190}, {100, 180}, {20, 20}, {0, 100}}, e)) return 1;
        }
        Align sat{2, 128, 128, std::vector<uint8_t>(256, (uint8_t)'A')};
        for (int k = 64; k < 96; k++) sat.bytes[(size_t)(128 + k)] = (uint8_t)'C';
        const Ranges rs{{0, 128}, {64, 96}, {0, 64}, {32, 128}};
        for (int model : {J, K}) {
            Call f;
            f.model = model; f.expect = FNN_EINVAL; f.names = "(1, 0, 1)";
            if (run("saturated range, fail", sat, rs, f)) return 1;
            Call k;
            k.model = model; k.policy = FNN_DIST_SAT_CAP;
            if (run("saturated range, cap", sat, rs, k)) return 1;
        }
        Call t;
        t.model = TABLES;
        if (run("tables of an empty range", sat, Ranges{{0, 128}, {5, 5}, {64, 96}}, t)) return 1;
    }
    // 6. layouts and chunks: padded lds, ld, stride; FNN_BATCH_CHUNK=3 at B = 7 through both entries
    {
        const Align al = make_align(7, 165, 170, 5, 9150);
        const Ranges r{{0, 165}, {1, 120}, {40, 165}, {64, 128}, {63, 129}, {20, 150}, {0, 100}};
        for (int model : {P, K, T, TABLES})
            for (int in_place = 0; in_place < 2; in_place++)
                for (int chunk : {0, 3}) {
                    Call c;
                    c.model = model; c.policy = FNN_DIST_SAT_CAP; c.ld = 9; c.stride = (model == TABLES ? 16 : 1) * 7 * 9 + 7; c.in_place = in_place != 0; c.chunk = chunk;
                    if (run("layout", al, r, c)) return 1;
                }
    }
    std::printf("ok: %d runs\n", runs);
    return 0;
}

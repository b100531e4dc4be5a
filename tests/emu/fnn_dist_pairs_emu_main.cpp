// fnn_dist_pairs_emu_main.cpp -- TEST INFRASTRUCTURE: stand-alone program over the CPU driver of the 4 x 4 tables of state
// pairs (fnn_dist_pairs_emu.cpp), meant to be built with -fsanitize=address,undefined, as fnn_dist_model_emu_main.cpp is for
// JC69 and K2P.
//
// Runs shape, digit-plane and kind cases on generated inputs under both saturation policies, for the four models and the table
// entries.  The table of every (b, i, j) comes from a plain loop over the definition, the distance from fnn_dist_model.h's
// formulas on that table (their bits are tests/test_dist_pairs_emu.py's business); where the definition has an empty, a
// degenerate or a saturated pair the call must fail and name the lowest one with its kind, or store the cap.  The caller's
// arrays are heap blocks of EXACTLY the declared sizes, filled with 0xFF bytes first; the output's padding - and after a
// failure of the host entry all of it - must still hold those bytes.  Exit status 0: all well.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fastnn.h"
#include "../../fastneighbornet_amd/csrc/fnn_dist_model.h"

extern "C" {
const char* emup_last_error(void);
int32_t emup_alignment_distances_model_batch_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch, int64_t ldc,
                                                 const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                 fnn_dist_model_stats* stats);
int32_t emup_alignment_distances_model_batch_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch,
                                                        int64_t ldc, const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                        fnn_dist_model_stats* stats);
int32_t emup_alignment_pair_counts_batch_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch, int64_t ldc,
                                             int32_t device, int64_t* F_out, int64_t ld, int64_t stride, fnn_dist_model_stats* stats);
int32_t emup_alignment_pair_counts_batch_device_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch,
                                                    int64_t ldc, int32_t device, int64_t* F_out, int64_t ld, int64_t stride, fnn_dist_model_stats* stats);
}

static uint64_t splitmix64(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

const int COUNTS = -1;               // Case::model of the table entries

struct Case {
    int model;                       // FNN_DIST_F81 ... FNN_DIST_LOGDET, or COUNTS
    int n, L, B, cmax;
    int diverge_pct, missing_pct;    // per cent of bytes redrawn; per cent of bytes 255
    bool letters;                    // lower case, U and the ambiguity letters R, Y, N among the bytes
    int64_t lds, ldc, ld, stride;    // 0: dense (stride in units of one (i, j) entry: the table entries take 16 times as much)
    bool in_place;
    const char* chunk;               // FNN_BATCH_CHUNK or nullptr
    int passes;                      // expected digit_passes
};

static int code_of(uint8_t x) {
    switch (x) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': case 'U': case 'u': return 3;
    }
    return 255;
}

enum { FINITE = 0, EMPTY = 1, DEGENERATE = 2, SATURATED = 3 };
static const char* kind_word(int kind) { return kind == EMPTY ? "valid == 0" : kind == DEGENERATE ? "degenerate" : "saturated"; }

static int run_case(const Case& c, uint64_t seed, int policy) {
    const int n = c.n, L = c.L, B = c.B;
    const bool tables = c.model == COUNTS;
    const int64_t cell = tables ? 16 : 1;
    const double cap = 12.5;
    const int64_t lds = c.lds ? c.lds : L, ldc = c.ldc ? c.ldc : L, ld = c.ld ? c.ld : n, stride = (c.stride ? c.stride : (int64_t)n * ld) * cell;
    const size_t seq_bytes = (size_t)((int64_t)(n - 1) * lds + L), cnt_elems = (size_t)((int64_t)(B - 1) * ldc + L);
    const size_t out_elems = (size_t)((int64_t)(B - 1) * stride + ((int64_t)(n - 1) * ld + n) * cell);
    uint8_t* seq = (uint8_t*)std::malloc(seq_bytes);
    uint16_t* cnt = (uint16_t*)std::malloc(sizeof(uint16_t) * cnt_elems);
    uint64_t* out = (uint64_t*)std::malloc(8 * out_elems);   // (doubles or int64_t: compared as 8-byte words)
    if (!seq || !cnt || !out) return 1;
    uint64_t s = seed;
    const char* alphabet = c.letters ? "ACGTacgtUuRYN" : "ACGT";
    const uint64_t na = std::strlen(alphabet);
    for (size_t k = 0; k < seq_bytes; k++) seq[k] = (uint8_t)"ACGT"[splitmix64(s) & 3];   // padding that would change the result if read
    for (size_t k = 0; k < cnt_elems; k++) cnt[k] = 999;
    std::memset(out, 0xFF, 8 * out_elems);
    std::vector<uint8_t> base((size_t)L);
    for (int k = 0; k < L; k++) base[(size_t)k] = (uint8_t)"ACGT"[splitmix64(s) & 3];
    int64_t n_recoded = 0;
    for (int i = 0; i < n; i++)
        for (int k = 0; k < L; k++) {
            uint8_t v = (int)(splitmix64(s) % 100) < c.diverge_pct ? (uint8_t)alphabet[splitmix64(s) % na] : base[(size_t)k];
            if ((int)(splitmix64(s) % 100) < c.missing_pct) v = FNN_SITE_MISSING;
            if (v != FNN_SITE_MISSING && code_of(v) == 255) n_recoded++;
            seq[(size_t)((int64_t)i * lds + k)] = v;
        }
    for (int b = 0; b < B; b++)
        for (int k = 0; k < L; k++) cnt[(size_t)((int64_t)b * ldc + k)] = (uint16_t)(1 + splitmix64(s) % (uint64_t)c.cmax);
    cnt[(size_t)((int64_t)(B / 2) * ldc + L / 2)] = (uint16_t)c.cmax;

    // the definition
    std::vector<uint64_t> want(out_elems, 0);
    std::vector<char> written(out_elems, 0);
    int first_kind = FINITE, fb = -1, fi = -1, fj = -1;
    int64_t capped_problems = 0;
    for (int b = 0; b < B; b++) {
        bool any_capped = false;
        for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++) {
                const size_t at = (size_t)((int64_t)b * stride + ((int64_t)i * ld + j) * cell);
                for (int64_t q = 0; q < cell; q++) written[at + (size_t)q] = 1;
                if (i == j) continue;
                const int lo = i < j ? i : j, hi = i < j ? j : i;
                fnn::DistTable t{};
                for (int k = 0; k < L; k++) {
                    const int x = code_of(seq[(size_t)((int64_t)lo * lds + k)]), y = code_of(seq[(size_t)((int64_t)hi * lds + k)]);
                    if (x == 255 || y == 255) continue;
                    t.F[4 * x + y] += cnt[(size_t)((int64_t)b * ldc + k)];
                }
                if (tables) {  // the block at (hi, lo) is the transposed table
                    for (int x = 0; x < 4; x++)
                        for (int y = 0; y < 4; y++) want[at + (size_t)(i < j ? 4 * x + y : 4 * y + x)] = (uint64_t)t.F[4 * x + y];
                    continue;
                }
                fnn::dist_table_sums(t);
                int kind = FINITE;
                double d = 0.0;
                if (t.v == 0) kind = EMPTY;
                else if (t.mism != 0) {
                    const int32_t k = c.model == FNN_DIST_F81 ? fnn::dist_f81(t, d) : c.model == FNN_DIST_F84 ? fnn::dist_f84(t, d)
                                    : c.model == FNN_DIST_TN93 ? fnn::dist_tn93(t, d) : fnn::dist_logdet(t, d);
                    kind = k == fnn::DIST_KIND_DEGENERATE ? DEGENERATE : k == fnn::DIST_KIND_SATURATED ? SATURATED : FINITE;
                }
                if (kind == DEGENERATE || kind == SATURATED) { any_capped = true; d = cap; }
                const bool fails = kind == EMPTY || (kind != FINITE && policy == FNN_DIST_SAT_FAIL);
                if (fails && i < j && first_kind == FINITE) { first_kind = kind; fb = b; fi = i; fj = j; }
                std::memcpy(&want[at], &d, 8);
            }
        capped_problems += any_capped ? 1 : 0;
    }

    if (c.chunk) setenv("FNN_BATCH_CHUNK", c.chunk, 1); else unsetenv("FNN_BATCH_CHUNK");
    fnn_dist_model m{};
    m.model = c.model;
    m.on_saturation = policy;
    m.cap = policy == FNN_DIST_SAT_CAP ? cap : 0.0;
    fnn_dist_model_stats st{};
    int32_t rc;
    if (tables)
        rc = (c.in_place ? emup_alignment_pair_counts_batch_device_i64 : emup_alignment_pair_counts_batch_i64)(seq, n, L, lds, cnt, B, ldc, 0, (int64_t*)out, ld,
                                                                                                               stride, &st);
    else
        rc = (c.in_place ? emup_alignment_distances_model_batch_device_f64 : emup_alignment_distances_model_batch_f64)(seq, n, L, lds, cnt, B, ldc, &m, 0,
                                                                                                                       (double*)out, ld, stride, &st);
    int bad = 0;
    char tag[96];
    std::snprintf(tag, sizeof(tag), "model=%d policy=%d n=%d L=%d B=%d", c.model, policy, n, L, B);
    if (first_kind != FINITE) {
        char name[64];
        std::snprintf(name, sizeof(name), "(%d, %d, %d)", fb, fi, fj);
        const std::string msg = emup_last_error();
        if (rc != FNN_EINVAL || msg.find(name) == std::string::npos || msg.find(kind_word(first_kind)) == std::string::npos) {
            std::fprintf(stderr, "%s: status %d (%s), expected FNN_EINVAL naming %s as %s\n", tag, rc, msg.c_str(), name, kind_word(first_kind));
            bad = 1;
        }
        for (size_t k = 0; k < out_elems && !bad && !c.in_place; k++)
            if (out[k] != ~0ull) { std::fprintf(stderr, "%s: the output was written although the call failed\n", tag); bad = 1; }
    } else {
        if (rc != FNN_OK) { std::fprintf(stderr, "%s: status %d (%s)\n", tag, rc, emup_last_error()); bad = 1; }
        if (!bad && st.base.digit_passes != c.passes) { std::fprintf(stderr, "%s: %d digit passes, expected %d\n", tag, st.base.digit_passes, c.passes); bad = 1; }
        if (!bad && (st.n_recoded != n_recoded || st.n_saturated_problems != (policy == FNN_DIST_SAT_CAP && !tables ? capped_problems : 0))) {
            std::fprintf(stderr, "%s: n_recoded %lld, n_saturated_problems %lld\n", tag, (long long)st.n_recoded, (long long)st.n_saturated_problems);
            bad = 1;
        }
        for (size_t k = 0; k < out_elems && !bad; k++) {
            if (!written[k]) {
                if (out[k] != ~0ull) { std::fprintf(stderr, "%s: output padding at %zu was written\n", tag, k); bad = 1; }
            } else if (out[k] != want[k]) {
                std::fprintf(stderr, "%s: word %zu is %016llx, expected %016llx\n", tag, k, (unsigned long long)out[k], (unsigned long long)want[k]);
                bad = 1;
            }
        }
    }
    std::free(seq);
    std::free(cnt);
    std::free(out);
    return bad;
}

int main() {
    const int E = FNN_DIST_F81, F = FNN_DIST_F84, T = FNN_DIST_TN93, D = FNN_DIST_LOGDET, N = COUNTS;
    const Case cases[] = {
        // shape edges, without and with missing bytes (at few sites some of these have empty, degenerate or saturated pairs: named, or capped)
        {E, 1, 1, 1, 127, 10, 0, false, 0, 0, 0, 0, false, nullptr, 1},    {F, 2, 15, 15, 127, 10, 5, false, 0, 0, 0, 0, false, nullptr, 1},
        {T, 3, 16, 16, 127, 10, 5, false, 0, 0, 0, 0, false, nullptr, 1},  {D, 5, 17, 17, 127, 10, 0, false, 0, 0, 0, 0, false, nullptr, 1},
        {N, 6, 63, 33, 127, 10, 0, false, 0, 0, 0, 0, false, nullptr, 1},  {T, 7, 64, 1, 127, 10, 5, false, 0, 0, 0, 0, false, nullptr, 1},
        {D, 17, 65, 15, 127, 10, 0, false, 0, 0, 0, 0, false, nullptr, 1}, {F, 33, 130, 16, 127, 10, 5, false, 0, 0, 0, 0, false, nullptr, 1},
        {N, 33, 1, 17, 127, 0, 0, false, 0, 0, 0, 0, false, nullptr, 1},   {T, 33, 130, 33, 127, 10, 5, false, 0, 0, 0, 0, false, nullptr, 1},
        {E, 17, 130, 33, 127, 10, 0, false, 0, 0, 0, 0, false, nullptr, 1},
        // digit planes, without and with missing bytes; B = 33 with one plane and B = 17 with more: one more than a replicate group
        {T, 7, 65, 33, 127, 10, 0, false, 0, 0, 0, 0, false, nullptr, 1},   {N, 7, 65, 33, 127, 10, 10, false, 0, 0, 0, 0, false, nullptr, 1},
        {T, 7, 65, 17, 128, 10, 0, false, 0, 0, 0, 0, false, nullptr, 2},   {N, 7, 65, 17, 128, 10, 10, false, 0, 0, 0, 0, false, nullptr, 2},
        {D, 7, 65, 17, 16384, 10, 0, false, 0, 0, 0, 0, false, nullptr, 3}, {T, 7, 65, 17, 16384, 10, 10, false, 0, 0, 0, 0, false, nullptr, 3},
        {N, 7, 65, 17, 65535, 10, 10, false, 0, 0, 0, 0, false, nullptr, 3},
        // recoding: lower case, U, ambiguity letters
        {T, 9, 130, 5, 127, 15, 0, true, 0, 0, 0, 0, false, nullptr, 1},    {N, 9, 130, 5, 300, 15, 5, true, 140, 131, 10, 95, true, nullptr, 2},
        // kinds: few sites, far apart, many bytes missing
        {E, 4, 3, 5, 127, 60, 0, false, 0, 0, 0, 0, false, nullptr, 1},     {F, 4, 3, 5, 127, 60, 0, false, 0, 0, 0, 0, false, nullptr, 1},
        {T, 4, 6, 5, 127, 60, 30, false, 0, 0, 0, 0, false, nullptr, 1},    {D, 4, 6, 5, 127, 60, 30, true, 0, 0, 0, 0, false, nullptr, 1},
        {F, 5, 12, 7, 127, 50, 20, false, 15, 14, 6, 40, true, "3", 1},     {D, 5, 12, 7, 127, 50, 20, false, 15, 14, 6, 40, false, "3", 1},
        {T, 6, 16, 40, 127, 40, 10, false, 0, 0, 0, 0, false, nullptr, 1},  {E, 6, 8, 40, 127, 40, 10, false, 0, 0, 0, 0, true, nullptr, 1},
        {N, 4, 3, 5, 127, 60, 30, false, 0, 0, 0, 0, false, nullptr, 1},
        // layout, both entries, and chunking
        {T, 7, 65, 7, 300, 10, 10, false, 70, 68, 9, 74, false, nullptr, 2}, {N, 7, 65, 7, 300, 10, 10, false, 70, 68, 9, 74, true, nullptr, 2},
        {D, 7, 65, 7, 300, 10, 10, false, 0, 0, 9, 70, false, "3", 2},       {N, 7, 65, 7, 300, 10, 10, false, 0, 0, 9, 70, false, "3", 2},
    };
    int k = 0, runs = 0;
    for (const Case& c : cases) {
        for (int policy : {FNN_DIST_SAT_FAIL, FNN_DIST_SAT_CAP}) {
            if (run_case(c, 7000 + (uint64_t)k, policy)) return 1;
            runs++;
        }
        k++;
    }
    unsetenv("FNN_BATCH_CHUNK");
    std::printf("ok: %d cases, %d runs\n", k, runs);
    return 0;
}

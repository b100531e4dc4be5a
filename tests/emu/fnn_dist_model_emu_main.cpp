// fnn_dist_model_emu_main.cpp -- TEST INFRASTRUCTURE: stand-alone program over the CPU driver of the corrected alignment
// distances (fnn_dist_model_emu.cpp), meant to be built with -fsanitize=address,undefined, as fnn_dist_emu_main.cpp is for
// the p-distance.
//
// Runs shape, digit-plane, recoding and saturation cases on generated inputs under both saturation policies.  The counts of
// every (b, i, j) come from a plain loop over the definition, the distance from fnn_dist_model.h's formulas on those counts
// (their bits are tests/test_dist_model_emu.py's business); where the definition has an empty or a saturated pair the call
// must fail and name the lowest one, or store the cap.  The caller's arrays are heap blocks of EXACTLY the declared sizes,
// filled with 0xFF bytes first; the output's padding - and after a failure of the host entry all of it - must still hold
// those bytes.  Exit status 0: all well.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../fastneighbornet_amd/csrc/fnn_dist_model.h"
#include "../../include/fastnn.h"

extern "C" {
const char* emu_last_error(void);
int32_t emu_alignment_distances_model_batch_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch, int64_t ldc,
                                                const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                fnn_dist_model_stats* stats);
int32_t emu_alignment_distances_model_batch_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch,
                                                       int64_t ldc, const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                       fnn_dist_model_stats* stats);
}

static uint64_t splitmix64(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

struct Case {
    int model;                       // FNN_DIST_JC69 or FNN_DIST_K2P
    int n, L, B, cmax;
    int diverge_pct, missing_pct;    // per cent of bytes redrawn; per cent of bytes 255
    bool letters;                    // K2P: lower case, U and the ambiguity letters R, Y, N among the bytes
    int64_t lds, ldc, ld, stride;    // 0: dense
    bool in_place;
    const char* chunk;               // FNN_BATCH_CHUNK or nullptr
    int passes;                      // expected digit_passes
};

static int k2p_code(uint8_t x) {
    switch (x) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': case 'U': case 'u': return 3;
    }
    return 255;
}

enum { FINITE = 0, EMPTY = 1, SATURATED = 2 };

static int run_case(const Case& c, uint64_t seed, int policy) {
    const int n = c.n, L = c.L, B = c.B;
    const double cap = 12.5;
    const int64_t lds = c.lds ? c.lds : L, ldc = c.ldc ? c.ldc : L, ld = c.ld ? c.ld : n, stride = c.stride ? c.stride : (int64_t)n * ld;
    const size_t seq_bytes = (size_t)((int64_t)(n - 1) * lds + L), cnt_elems = (size_t)((int64_t)(B - 1) * ldc + L);
    const size_t out_elems = (size_t)((int64_t)(B - 1) * stride + (int64_t)(n - 1) * ld + n);
    uint8_t* seq = (uint8_t*)std::malloc(seq_bytes);
    uint16_t* cnt = (uint16_t*)std::malloc(sizeof(uint16_t) * cnt_elems);
    double* out = (double*)std::malloc(sizeof(double) * out_elems);
    if (!seq || !cnt || !out) return 1;
    uint64_t s = seed;
    const char* alphabet = c.letters ? "ACGTacgtUuRYN" : "ACGT";
    const uint64_t na = std::strlen(alphabet);
    // padding: states and counts that would change the result if read
    for (size_t k = 0; k < seq_bytes; k++) seq[k] = (uint8_t)"ACGT"[splitmix64(s) & 3];
    for (size_t k = 0; k < cnt_elems; k++) cnt[k] = 999;
    std::memset(out, 0xFF, sizeof(double) * out_elems);
    std::vector<uint8_t> base((size_t)L);
    for (int k = 0; k < L; k++) base[(size_t)k] = (uint8_t)"ACGT"[splitmix64(s) & 3];
    int64_t n_recoded = 0;
    for (int i = 0; i < n; i++)
        for (int k = 0; k < L; k++) {
            uint8_t v = (int)(splitmix64(s) % 100) < c.diverge_pct ? (uint8_t)alphabet[splitmix64(s) % na] : base[(size_t)k];
            if ((int)(splitmix64(s) % 100) < c.missing_pct) v = FNN_SITE_MISSING;
            if (c.model == FNN_DIST_K2P && v != FNN_SITE_MISSING && k2p_code(v) == 255) n_recoded++;
            seq[(size_t)((int64_t)i * lds + k)] = v;
        }
    for (int b = 0; b < B; b++)
        for (int k = 0; k < L; k++) cnt[(size_t)((int64_t)b * ldc + k)] = (uint16_t)(1 + splitmix64(s) % (uint64_t)c.cmax);
    cnt[(size_t)((int64_t)(B / 2) * ldc + L / 2)] = (uint16_t)c.cmax;

    // the definition
    std::vector<double> want(out_elems, 0.0);
    std::vector<char> written(out_elems, 0);
    int first_kind = FINITE, fb = -1, fi = -1, fj = -1;
    int64_t saturated_problems = 0;
    for (int b = 0; b < B; b++) {
        bool any_sat = false;
        for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++) {
                const size_t at = (size_t)((int64_t)b * stride + (int64_t)i * ld + j);
                written[at] = 1;
                if (i == j) continue;
                int64_t mism = 0, valid = 0, ts = 0;
                for (int k = 0; k < L; k++) {
                    int x = seq[(size_t)((int64_t)i * lds + k)], y = seq[(size_t)((int64_t)j * lds + k)];
                    if (c.model == FNN_DIST_K2P) { x = x == FNN_SITE_MISSING ? 255 : k2p_code((uint8_t)x); y = y == FNN_SITE_MISSING ? 255 : k2p_code((uint8_t)y); }
                    if (x == 255 || y == 255) continue;
                    const int64_t w = cnt[(size_t)((int64_t)b * ldc + k)];
                    valid += w;
                    if (x != y) mism += w;
                    if (c.model == FNN_DIST_K2P && (x ^ y) == 2) ts += w;
                }
                int kind = FINITE;
                double d = 0.0;
                if (valid == 0) kind = EMPTY;
                else if (mism == 0) d = 0.0;
                else if (c.model == FNN_DIST_JC69) {
                    if (fnn::dist_jc69_saturated(4, mism, valid)) kind = SATURATED; else d = fnn::dist_jc69(4, mism, valid);
                } else {
                    if (fnn::dist_k2p_saturated(ts, mism - ts, valid)) kind = SATURATED; else d = fnn::dist_k2p(ts, mism - ts, valid);
                }
                if (kind == SATURATED) { any_sat = true; d = cap; }
                const bool fails = kind == EMPTY || (kind == SATURATED && policy == FNN_DIST_SAT_FAIL);
                if (fails && i < j && first_kind == FINITE) { first_kind = kind; fb = b; fi = i; fj = j; }
                want[at] = d;
            }
        saturated_problems += any_sat ? 1 : 0;
    }

    if (c.chunk) setenv("FNN_BATCH_CHUNK", c.chunk, 1); else unsetenv("FNN_BATCH_CHUNK");
    fnn_dist_model m{};
    m.model = c.model;
    m.states = 4;
    m.on_saturation = policy;
    m.cap = policy == FNN_DIST_SAT_CAP ? cap : 0.0;
    fnn_dist_model_stats st{};
    const int32_t rc = (c.in_place ? emu_alignment_distances_model_batch_device_f64 : emu_alignment_distances_model_batch_f64)(
        seq, n, L, lds, cnt, B, ldc, &m, 0, out, ld, stride, &st);
    int bad = 0;
    char tag[96];
    std::snprintf(tag, sizeof(tag), "model=%d policy=%d n=%d L=%d B=%d", c.model, policy, n, L, B);
    if (first_kind != FINITE) {
        char name[64];
        std::snprintf(name, sizeof(name), "(%d, %d, %d)", fb, fi, fj);
        const std::string msg = emu_last_error();
        const bool says_saturated = msg.find("saturated") != std::string::npos;
        if (rc != FNN_EINVAL || msg.find(name) == std::string::npos || says_saturated != (first_kind == SATURATED)) {
            std::fprintf(stderr, "%s: status %d (%s), expected FNN_EINVAL naming %s as %s\n", tag, rc, msg.c_str(), name, first_kind == SATURATED ? "saturated" : "empty");
            bad = 1;
        }
        for (size_t k = 0; k < out_elems && !bad && !c.in_place; k++) {
            uint64_t bits;
            std::memcpy(&bits, &out[k], 8);
            if (bits != ~0ull) { std::fprintf(stderr, "%s: the output was written although the call failed\n", tag); bad = 1; }
        }
    } else {
        if (rc != FNN_OK) { std::fprintf(stderr, "%s: status %d (%s)\n", tag, rc, emu_last_error()); bad = 1; }
        if (!bad && st.base.digit_passes != c.passes) { std::fprintf(stderr, "%s: %d digit passes, expected %d\n", tag, st.base.digit_passes, c.passes); bad = 1; }
        if (!bad && (st.n_recoded != n_recoded || st.n_saturated_problems != (policy == FNN_DIST_SAT_CAP ? saturated_problems : 0))) {
            std::fprintf(stderr, "%s: n_recoded %lld, n_saturated_problems %lld\n", tag, (long long)st.n_recoded, (long long)st.n_saturated_problems);
            bad = 1;
        }
        for (size_t k = 0; k < out_elems && !bad; k++) {
            uint64_t bits;
            std::memcpy(&bits, &out[k], 8);
            if (!written[k]) {
                if (bits != ~0ull) { std::fprintf(stderr, "%s: output padding at %zu was written\n", tag, k); bad = 1; }
            } else if (std::memcmp(&out[k], &want[k], 8) != 0) {
                std::fprintf(stderr, "%s: element %zu is %.17g, expected %.17g\n", tag, k, out[k], want[k]);
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
    const int J = FNN_DIST_JC69, K = FNN_DIST_K2P;
    const Case cases[] = {
        // shape edges, without and with missing bytes (at few sites some of these saturate or have empty pairs: named, or capped)
        {J, 1, 1, 1, 127, 10, 0, false, 0, 0, 0, 0, false, nullptr, 1},    {K, 2, 15, 15, 127, 10, 5, false, 0, 0, 0, 0, false, nullptr, 1},
        {J, 3, 16, 16, 127, 10, 5, false, 0, 0, 0, 0, false, nullptr, 1},  {K, 5, 17, 17, 127, 10, 0, false, 0, 0, 0, 0, false, nullptr, 1},
        {J, 6, 63, 33, 127, 10, 0, false, 0, 0, 0, 0, false, nullptr, 1},  {K, 7, 64, 1, 127, 10, 5, false, 0, 0, 0, 0, false, nullptr, 1},
        {K, 17, 65, 15, 127, 10, 0, false, 0, 0, 0, 0, false, nullptr, 1}, {J, 33, 130, 16, 127, 10, 5, false, 0, 0, 0, 0, false, nullptr, 1},
        {K, 65, 1, 17, 127, 0, 0, false, 0, 0, 0, 0, false, nullptr, 1},   {K, 65, 130, 33, 127, 10, 5, false, 0, 0, 0, 0, false, nullptr, 1},
        {J, 65, 130, 33, 127, 10, 0, false, 0, 0, 0, 0, false, nullptr, 1},
        // digit planes with three accumulator sets, without and with missing bytes; B = 65: three replicate groups of 32
        {K, 7, 65, 17, 127, 10, 0, false, 0, 0, 0, 0, false, nullptr, 1},   {K, 7, 65, 17, 127, 10, 10, false, 0, 0, 0, 0, false, nullptr, 1},
        {K, 7, 65, 17, 128, 10, 0, false, 0, 0, 0, 0, false, nullptr, 2},   {K, 7, 65, 17, 128, 10, 10, false, 0, 0, 0, 0, false, nullptr, 2},
        {K, 7, 65, 17, 16384, 10, 0, false, 0, 0, 0, 0, false, nullptr, 3}, {K, 7, 65, 65, 16384, 10, 10, false, 0, 0, 0, 0, false, nullptr, 3},
        {J, 7, 65, 65, 65535, 10, 10, false, 0, 0, 0, 0, false, nullptr, 3},
        // recoding: lower case, U, ambiguity letters
        {K, 9, 130, 5, 127, 15, 0, true, 0, 0, 0, 0, false, nullptr, 1},    {K, 9, 130, 5, 300, 15, 5, true, 140, 131, 10, 95, true, nullptr, 2},
        // saturation and empty pairs: few sites, far apart, many bytes missing
        {J, 4, 3, 5, 127, 60, 0, false, 0, 0, 0, 0, false, nullptr, 1},     {K, 4, 3, 5, 127, 60, 0, false, 0, 0, 0, 0, false, nullptr, 1},
        {J, 4, 3, 5, 127, 60, 30, false, 0, 0, 0, 0, false, nullptr, 1},    {K, 4, 3, 5, 127, 60, 30, true, 0, 0, 0, 0, false, nullptr, 1},
        {J, 5, 6, 7, 127, 50, 20, false, 9, 8, 6, 40, true, "3", 1},        {K, 5, 6, 7, 127, 50, 20, false, 9, 8, 6, 40, false, "3", 1},
        {K, 6, 8, 40, 127, 40, 10, false, 0, 0, 0, 0, false, nullptr, 1},   {J, 6, 8, 40, 127, 40, 10, false, 0, 0, 0, 0, true, nullptr, 1},
        // layout, both entries, and chunking
        {K, 7, 65, 7, 300, 10, 10, false, 70, 68, 9, 74, false, nullptr, 2}, {K, 7, 65, 7, 300, 10, 10, false, 70, 68, 9, 74, true, nullptr, 2},
        {K, 7, 65, 7, 300, 10, 10, false, 0, 0, 9, 70, false, "3", 2},       {K, 7, 65, 7, 300, 10, 10, false, 0, 0, 9, 70, true, "3", 2},
    };
    int k = 0, runs = 0;
    for (const Case& c : cases) {
        for (int policy : {FNN_DIST_SAT_FAIL, FNN_DIST_SAT_CAP}) {
            if (run_case(c, 5000 + (uint64_t)k, policy)) return 1;
            runs++;
        }
        k++;
    }
    unsetenv("FNN_BATCH_CHUNK");
    std::printf("ok: %d cases, %d runs\n", k, runs);
    return 0;
}

// fnn_dist_gamma_emu_main.cpp -- TEST INFRASTRUCTURE: stand-alone program over the CPU driver of the corrected distances with
// gamma-distributed rates (fnn_dist_gamma_emu.cpp), meant to be built with -fsanitize=address,undefined, as
// fnn_dist_pairs_emu_main.cpp is for the equal-rates models.
//
// Runs shape, digit-plane, overflow and chunking cases on generated inputs under both saturation policies, for the five models
// that have a gamma form, through a fnn_dist_model_rates on the heap.  The counts of every (b, i, j) come from a plain loop over
// the definition, the distance from fnn_dist_model.h's formulas on those counts with the shape (their bits are
// tests/test_dist_gamma_emu.py's business); where the definition has an empty, a degenerate or a saturated pair - by overflow of
// expm1' among them - the call must fail and name the lowest one with its kind, or store the cap.  Then the bootstrap entries on
// both draw routes: the same words from both, problem 0 of lead = 1 equal to the counts entry on all ones.  The caller's arrays
// are heap blocks of EXACTLY the declared sizes, filled with 0xFF bytes first; the output's padding - and after a failure of the
// host entry all of it - must still hold those bytes.  Exit status 0: all well.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fastnn.h"
#include "../../fastneighbornet_amd/csrc/fnn_dist_model.h"

extern "C" {
const char* emug_last_error(void);
int32_t emug_alignment_distances_model_batch_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch, int64_t ldc,
                                                 const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                 fnn_dist_model_stats* stats);
int32_t emug_alignment_distances_model_batch_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch,
                                                        int64_t ldc, const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                        fnn_dist_model_stats* stats);
int32_t emug_bootstrap_distances_batch_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, int64_t batch, uint64_t seed, int64_t lead,
                                           const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride, fnn_boot_stats* stats);
int32_t emug_bootstrap_distances_batch_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, int64_t batch, uint64_t seed, int64_t lead,
                                                  const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                  fnn_boot_stats* stats);
}

static uint64_t splitmix64(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

struct Case {
    int model;                       // FNN_DIST_JC69, FNN_DIST_K2P, FNN_DIST_F81, FNN_DIST_F84, FNN_DIST_TN93
    double shape;
    int n, L, B, cmax;
    int diverge_pct, missing_pct;    // per cent of bytes redrawn; per cent of bytes 255
    int64_t lds, ldc, ld, stride;    // 0: dense
    bool in_place;
    const char* chunk;               // FNN_BATCH_CHUNK or nullptr
    int passes;                      // expected digit_passes
};

static int code_of(uint8_t x) { return x == 'A' ? 0 : x == 'C' ? 1 : x == 'G' ? 2 : x == 'T' ? 3 : 255; }

enum { FINITE = 0, EMPTY = 1, DEGENERATE = 2, SATURATED = 3 };
static const char* kind_word(int kind) { return kind == EMPTY ? "valid == 0" : kind == DEGENERATE ? "degenerate" : "saturated"; }

// the model struct on the heap, exactly sizeof(fnn_dist_model_rates) bytes
static fnn_dist_model_rates* make_rates(int model, int policy, double cap, double shape) {
    fnn_dist_model_rates* mr = (fnn_dist_model_rates*)std::malloc(sizeof(fnn_dist_model_rates));
    if (!mr) return nullptr;
    std::memset(mr, 0, sizeof(*mr));
    mr->base.model = model;
    mr->base.states = 4;
    mr->base.on_saturation = policy;
    mr->base.reserved = FNN_DIST_RATES_GAMMA;
    mr->base.cap = policy == FNN_DIST_SAT_CAP ? cap : 0.0;
    mr->shape = shape;
    return mr;
}

// (kind, distance) of one pair from the definition; lo < hi
static int pair_of(const Case& c, const uint8_t* seq, int64_t lds, const uint16_t* cnt, int lo, int hi, double& d) {
    fnn::DistTable t{};
    for (int k = 0; k < c.L; k++) {
        const int x = code_of(seq[(size_t)((int64_t)lo * lds + k)]), y = code_of(seq[(size_t)((int64_t)hi * lds + k)]);
        if (x == 255 || y == 255) continue;
        t.F[4 * x + y] += cnt[k];
    }
    fnn::dist_table_sums(t);
    d = 0.0;
    if (t.v == 0) return EMPTY;
    if (t.mism == 0) return FINITE;
    bool over = false;
    if (c.model == FNN_DIST_JC69) {
        if (fnn::dist_jc69_saturated(4, t.mism, t.v)) return SATURATED;
        d = fnn::dist_jc69(4, t.mism, t.v, c.shape, over);
        return over ? SATURATED : FINITE;
    }
    if (c.model == FNN_DIST_K2P) {
        const int64_t ts = t.ts1 + t.ts2;
        if (fnn::dist_k2p_saturated(ts, t.mism - ts, t.v)) return SATURATED;
        d = fnn::dist_k2p(ts, t.mism - ts, t.v, c.shape, over);
        return over ? SATURATED : FINITE;
    }
    const int32_t k = c.model == FNN_DIST_F81 ? fnn::dist_f81(t, d, c.shape) : c.model == FNN_DIST_F84 ? fnn::dist_f84(t, d, c.shape) : fnn::dist_tn93(t, d, c.shape);
    return k == fnn::DIST_KIND_DEGENERATE ? DEGENERATE : k == fnn::DIST_KIND_SATURATED ? SATURATED : FINITE;
}

static int run_case(const Case& c, uint64_t seed, int policy) {
    const int n = c.n, L = c.L, B = c.B;
    const double cap = 12.5;
    const int64_t lds = c.lds ? c.lds : L, ldc = c.ldc ? c.ldc : L, ld = c.ld ? c.ld : n, stride = c.stride ? c.stride : (int64_t)n * ld;
    const size_t seq_bytes = (size_t)((int64_t)(n - 1) * lds + L), cnt_elems = (size_t)((int64_t)(B - 1) * ldc + L);
    const size_t out_elems = (size_t)((int64_t)(B - 1) * stride + (int64_t)(n - 1) * ld + n);
    uint8_t* seq = (uint8_t*)std::malloc(seq_bytes);
    uint16_t* cnt = (uint16_t*)std::malloc(sizeof(uint16_t) * cnt_elems);
    uint64_t* out = (uint64_t*)std::malloc(8 * out_elems);   // (doubles, compared as 8-byte words)
    fnn_dist_model_rates* mr = make_rates(c.model, policy, cap, c.shape);
    if (!seq || !cnt || !out || !mr) return 1;
    uint64_t s = seed;
    for (size_t k = 0; k < seq_bytes; k++) seq[k] = (uint8_t)"ACGT"[splitmix64(s) & 3];   // padding that would change the result if read
    for (size_t k = 0; k < cnt_elems; k++) cnt[k] = 999;
    std::memset(out, 0xFF, 8 * out_elems);
    std::vector<uint8_t> base((size_t)L);
    for (int k = 0; k < L; k++) base[(size_t)k] = (uint8_t)"ACGT"[splitmix64(s) & 3];
    for (int i = 0; i < n; i++)
        for (int k = 0; k < L; k++) {
            uint8_t v = (int)(splitmix64(s) % 100) < c.diverge_pct ? (uint8_t)"ACGT"[splitmix64(s) & 3] : base[(size_t)k];
            if ((int)(splitmix64(s) % 100) < c.missing_pct) v = FNN_SITE_MISSING;
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
                const size_t at = (size_t)((int64_t)b * stride + (int64_t)i * ld + j);
                written[at] = 1;
                if (i == j) continue;
                double d = 0.0;
                int kind = pair_of(c, seq, lds, cnt + (int64_t)b * ldc, i < j ? i : j, i < j ? j : i, d);
                if (kind == DEGENERATE || kind == SATURATED) { any_capped = true; d = cap; }
                const bool fails = kind == EMPTY || (kind != FINITE && policy == FNN_DIST_SAT_FAIL);
                if (fails && i < j && first_kind == FINITE) { first_kind = kind; fb = b; fi = i; fj = j; }
                std::memcpy(&want[at], &d, 8);
            }
        capped_problems += any_capped ? 1 : 0;
    }

    if (c.chunk) setenv("FNN_BATCH_CHUNK", c.chunk, 1); else unsetenv("FNN_BATCH_CHUNK");
    fnn_dist_model_stats st{};
    const int32_t rc = (c.in_place ? emug_alignment_distances_model_batch_device_f64 : emug_alignment_distances_model_batch_f64)(
        seq, n, L, lds, cnt, B, ldc, &mr->base, 0, (double*)out, ld, stride, &st);
    int bad = 0;
    char tag[128];
    std::snprintf(tag, sizeof(tag), "model=%d shape=%g policy=%d n=%d L=%d B=%d", c.model, c.shape, policy, n, L, B);
    if (first_kind != FINITE) {
        char name[64];
        std::snprintf(name, sizeof(name), "(%d, %d, %d)", fb, fi, fj);
        const std::string msg = emug_last_error();
        if (rc != FNN_EINVAL || msg.find(name) == std::string::npos || msg.find(kind_word(first_kind)) == std::string::npos) {
            std::fprintf(stderr, "%s: status %d (%s), expected FNN_EINVAL naming %s as %s\n", tag, rc, msg.c_str(), name, kind_word(first_kind));
            bad = 1;
        }
        for (size_t k = 0; k < out_elems && !bad && !c.in_place; k++)
            if (out[k] != ~0ull) { std::fprintf(stderr, "%s: the output was written although the call failed\n", tag); bad = 1; }
    } else {
        if (rc != FNN_OK) { std::fprintf(stderr, "%s: status %d (%s)\n", tag, rc, emug_last_error()); bad = 1; }
        if (!bad && st.base.digit_passes != c.passes) { std::fprintf(stderr, "%s: %d digit passes, expected %d\n", tag, st.base.digit_passes, c.passes); bad = 1; }
        if (!bad && st.n_saturated_problems != (policy == FNN_DIST_SAT_CAP ? capped_problems : 0)) {
            std::fprintf(stderr, "%s: n_saturated_problems %lld, expected %lld\n", tag, (long long)st.n_saturated_problems, (long long)capped_problems);
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
    std::free(mr);
    return bad;
}

// the bootstrap entries with lead = 1 on both draw routes, host and in-place output: one set of words, and problem 0 is the
// counts entry on all ones
static int run_boot(int model, double shape, int n, int L, int B, uint64_t seed) {
    const size_t seq_bytes = (size_t)n * (size_t)L, out_elems = (size_t)B * (size_t)n * (size_t)n;
    uint8_t* seq = (uint8_t*)std::malloc(seq_bytes);
    uint16_t* ones = (uint16_t*)std::malloc(sizeof(uint16_t) * (size_t)L);
    uint64_t* first = (uint64_t*)std::malloc(8 * (size_t)n * (size_t)n);
    fnn_dist_model_rates* mr = make_rates(model, FNN_DIST_SAT_CAP, 12.5, shape);
    if (!seq || !ones || !first || !mr) return 1;
    uint64_t s = seed;
    std::vector<uint8_t> base((size_t)L);
    for (int k = 0; k < L; k++) base[(size_t)k] = (uint8_t)"ACGT"[splitmix64(s) & 3];
    for (size_t k = 0; k < seq_bytes; k++) {
        seq[k] = splitmix64(s) % 100 < 10 ? (uint8_t)"ACGT"[splitmix64(s) & 3] : base[k % (size_t)L];
        if (splitmix64(s) % 100 < 3) seq[k] = FNN_SITE_MISSING;
    }
    for (int k = 0; k < L; k++) ones[k] = 1;
    int bad = 0;
    if (emug_alignment_distances_model_batch_f64(seq, n, L, L, ones, 1, L, &mr->base, 0, (double*)first, n, (int64_t)n * n, nullptr) != FNN_OK) {
        std::fprintf(stderr, "boot model=%d: the counts entry failed (%s)\n", model, emug_last_error());
        bad = 1;
    }
    std::vector<uint64_t> ref;
    for (int variant = 0; variant < 4 && !bad; variant++) {
        uint64_t* out = (uint64_t*)std::malloc(8 * out_elems);
        if (!out) return 1;
        std::memset(out, 0xFF, 8 * out_elems);
        setenv("FNN_DRAW_ROUTE", variant & 1 ? "host" : "device", 1);
        fnn_boot_stats st{};
        const int32_t rc = (variant & 2 ? emug_bootstrap_distances_batch_device_f64 : emug_bootstrap_distances_batch_f64)(
            seq, n, L, L, B, 77, 1, &mr->base, 0, (double*)out, n, (int64_t)n * n, &st);
        if (rc != FNN_OK || st.draw_route != (variant & 1 ? FNN_DRAW_HOST : FNN_DRAW_DEVICE)) {
            std::fprintf(stderr, "boot model=%d variant=%d: status %d (%s), route %d\n", model, variant, rc, emug_last_error(), st.draw_route);
            bad = 1;
        }
        if (!bad && std::memcmp(out, first, 8 * (size_t)n * (size_t)n) != 0) { std::fprintf(stderr, "boot model=%d variant=%d: problem 0 differs\n", model, variant); bad = 1; }
        if (!bad && variant == 0) ref.assign(out, out + out_elems);
        if (!bad && std::memcmp(out, ref.data(), 8 * out_elems) != 0) { std::fprintf(stderr, "boot model=%d variant=%d: the routes differ\n", model, variant); bad = 1; }
        std::free(out);
    }
    unsetenv("FNN_DRAW_ROUTE");
    std::free(seq);
    std::free(ones);
    std::free(first);
    std::free(mr);
    return bad;
}

int main() {
    const int J = FNN_DIST_JC69, K = FNN_DIST_K2P, E = FNN_DIST_F81, F = FNN_DIST_F84, T = FNN_DIST_TN93;
    const Case cases[] = {
        // shape edges, without and with missing bytes (at few sites some of these have empty, degenerate or saturated pairs: named, or capped)
        {J, 0.5, 1, 1, 1, 127, 10, 0, 0, 0, 0, 0, false, nullptr, 1},     {K, 0.05, 2, 15, 15, 127, 10, 5, 0, 0, 0, 0, false, nullptr, 1},
        {E, 1.0, 3, 16, 16, 127, 10, 5, 0, 0, 0, 0, false, nullptr, 1},   {F, 4.0, 5, 17, 17, 127, 10, 0, 0, 0, 0, 0, false, nullptr, 1},
        {T, 0.5, 6, 63, 33, 127, 10, 0, 0, 0, 0, 0, false, nullptr, 1},   {J, 4.0, 7, 64, 1, 127, 10, 5, 0, 0, 0, 0, false, nullptr, 1},
        {K, 1.0, 17, 65, 15, 127, 10, 0, 0, 0, 0, 0, false, nullptr, 1},  {F, 0.05, 33, 130, 16, 127, 10, 5, 0, 0, 0, 0, false, nullptr, 1},
        {T, 0.05, 33, 130, 33, 127, 10, 5, 0, 0, 0, 0, false, nullptr, 1}, {E, 0.5, 17, 130, 33, 127, 10, 0, 0, 0, 0, 0, false, nullptr, 1},
        // digit planes, without and with missing bytes
        {K, 0.5, 7, 65, 17, 128, 10, 0, 0, 0, 0, 0, false, nullptr, 2},    {T, 0.5, 7, 65, 17, 128, 10, 10, 0, 0, 0, 0, false, nullptr, 2},
        {K, 0.5, 7, 65, 65, 16384, 10, 10, 0, 0, 0, 0, false, nullptr, 3}, {T, 0.5, 7, 65, 17, 16384, 10, 0, 0, 0, 0, 0, false, nullptr, 3},
        {J, 0.5, 7, 65, 17, 65535, 10, 10, 0, 0, 0, 0, false, nullptr, 3},
        // overflow of expm1': a shape so small that the divergent pairs' t passes 709.78...
        {J, 0.0005, 5, 64, 5, 127, 40, 0, 0, 0, 0, 0, false, nullptr, 1},  {K, 0.0005, 5, 64, 5, 127, 40, 0, 0, 0, 0, 0, false, nullptr, 1},
        {E, 0.0005, 5, 64, 5, 127, 40, 5, 0, 0, 0, 0, false, nullptr, 1},  {F, 0.0005, 5, 64, 5, 127, 40, 0, 0, 0, 0, 0, true, nullptr, 1},
        {T, 0.0005, 5, 64, 5, 127, 40, 0, 0, 0, 0, 0, false, nullptr, 1},  {T, 1e-300, 4, 64, 3, 127, 10, 0, 0, 0, 0, 0, false, nullptr, 1},
        // kinds: few sites, far apart, many bytes missing
        {F, 0.5, 4, 3, 5, 127, 60, 0, 0, 0, 0, 0, false, nullptr, 1},      {T, 0.5, 4, 6, 5, 127, 60, 30, 0, 0, 0, 0, false, nullptr, 1},
        {K, 0.5, 4, 6, 5, 127, 60, 30, 0, 0, 0, 0, true, nullptr, 1},      {E, 0.05, 6, 8, 40, 127, 40, 10, 0, 0, 0, 0, true, nullptr, 1},
        // layout, both entries, and chunking
        {T, 0.5, 7, 65, 7, 300, 10, 10, 70, 68, 9, 74, false, nullptr, 2}, {K, 0.5, 7, 65, 7, 300, 10, 10, 70, 68, 9, 74, true, nullptr, 2},
        {F, 1.0, 7, 65, 7, 300, 10, 10, 0, 0, 9, 70, false, "3", 2},       {J, 1.0, 7, 65, 7, 300, 10, 10, 0, 0, 9, 70, true, "3", 2},
    };
    int k = 0, runs = 0;
    for (const Case& c : cases) {
        for (int policy : {FNN_DIST_SAT_FAIL, FNN_DIST_SAT_CAP}) {
            if (run_case(c, 9000 + (uint64_t)k, policy)) return 1;
            runs++;
        }
        k++;
    }
    unsetenv("FNN_BATCH_CHUNK");
    for (int model : {J, K, E, F, T}) {
        if (run_boot(model, 0.5, 6, 130, 5, 9500 + (uint64_t)model)) return 1;
        runs++;
    }
    std::printf("ok: %d cases, %d runs\n", k, runs);
    return 0;
}

// fnn_draw_emu_main.cpp -- TEST INFRASTRUCTURE: stand-alone program over the CPU driver of the bootstrap entries that draw their
// replicates on the device (fnn_draw_emu.cpp), meant to be built with -fsanitize=address,undefined, as fnn_dist_model_emu_main.cpp
// is for the counts entries.
//
// The counts of every case come from a plain loop over the definition (SplitMix64 by its recurrence, the site by a 128-bit
// product).  The drawn planes (emu_bootstrap_draw_planes) must hold their digits, zero wherever the definition has nothing;
// the matrices of the bootstrap entries must be, byte for byte, those of the counts entries on these counts (what those are
// is fnn_dist_model_emu_main.cpp's business), padding untouched, under both draw routes, with forced digit planes and in
// chunks.  The caller's arrays are heap blocks of EXACTLY the declared sizes, filled with 0xFF bytes first; the driver does
// the same for the histogram (the launch's LDS bytes) and for every device buffer.  Exit status 0: all well.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fastnn.h"

extern "C" {
const char* emu_last_error(void);
int32_t emu_alignment_distances_model_batch_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch, int64_t ldc,
                                                const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                fnn_dist_model_stats* stats);
int32_t emu_bootstrap_distances_batch_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, int64_t batch, uint64_t seed, int64_t lead,
                                          const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride, fnn_boot_stats* stats);
int32_t emu_bootstrap_distances_batch_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, int64_t batch, uint64_t seed, int64_t lead,
                                                 const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                 fnn_boot_stats* stats);
int32_t emu_bootstrap_draw_planes(int64_t L, int64_t batch, int64_t first, int64_t lead, uint64_t seed, int32_t digits, int8_t* planes_out,
                                  int64_t* total_out, uint32_t* max_count_out);
int32_t emu_bootstrap_draw_max_sites(void);
}

static uint64_t splitmix64(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// the definition: `lead` rows of ones, then replicate r draws the outputs r L ... r L + L - 1 of the generator seeded with `seed`
static std::vector<uint16_t> definition(int64_t L, int64_t batch, uint64_t seed, int64_t lead) {
    std::vector<uint16_t> c((size_t)(batch * L), 0);
    uint64_t state = seed;
    for (int64_t b = 0; b < batch; b++)
        for (int64_t k = 0; k < L; k++) {
            if (b < lead) { c[(size_t)(b * L + k)] = 1; continue; }
            const uint64_t x = splitmix64(state);
            c[(size_t)(b * L + (int64_t)(uint64_t)(((unsigned __int128)x * (unsigned __int128)(uint64_t)L) >> 64))]++;
        }
    return c;
}

static int check_planes(int64_t L, int64_t batch, uint64_t seed, int64_t lead, int digits) {
    const int64_t lpad = (L + 63) / 64 * 64, rows = (batch + 63) / 64 * 64;
    const size_t plane = (size_t)(rows * lpad);
    int8_t* planes = (int8_t*)std::malloc(plane * (size_t)digits);
    int64_t* total = (int64_t*)std::malloc(sizeof(int64_t) * (size_t)rows);
    uint32_t most = 0;
    if (!planes || !total) return 1;
    std::memset(planes, 0xFF, plane * (size_t)digits);
    std::memset(total, 0xFF, sizeof(int64_t) * (size_t)rows);
    int bad = 0;
    if (emu_bootstrap_draw_planes(L, batch, 0, lead, seed, digits, planes, total, &most) != FNN_OK) {
        std::fprintf(stderr, "planes L=%lld: %s\n", (long long)L, emu_last_error());
        bad = 1;
    }
    const std::vector<uint16_t> c = definition(L, batch, seed, lead);
    uint32_t want_most = 0;
    for (int d = 0; d < digits && !bad; d++)
        for (int64_t b = 0; b < rows && !bad; b++)
            for (int64_t s = 0; s < lpad && !bad; s++) {
                const uint32_t count = b < batch && s < L ? c[(size_t)(b * L + s)] : 0;
                want_most = count > want_most ? count : want_most;
                if (planes[(size_t)d * plane + (size_t)(b * lpad + s)] != (int8_t)((count >> (7 * d)) & 127)) {
                    std::fprintf(stderr, "planes L=%lld batch=%lld: digit %d of (%lld, %lld) is wrong\n", (long long)L, (long long)batch, d, (long long)b, (long long)s);
                    bad = 1;
                }
            }
    for (int64_t b = 0; b < rows && !bad; b++)
        if (total[b] != (b < batch ? L : 0)) { std::fprintf(stderr, "planes L=%lld: total of row %lld\n", (long long)L, (long long)b); bad = 1; }
    if (!bad && most != want_most) { std::fprintf(stderr, "planes L=%lld: largest count %u, expected %u\n", (long long)L, most, want_most); bad = 1; }
    std::free(planes);
    std::free(total);
    return bad;
}

struct Case {
    int model, n, L, batch, lead, missing_pct;
    uint64_t seed;
    int64_t lds, ld, stride;  // 0: dense
    bool in_place;
    const char* chunk;   // FNN_BATCH_CHUNK or nullptr
    const char* digits;  // FNN_DIST_FORCE_DIGITS or nullptr
    const char* route;   // FNN_DRAW_ROUTE or nullptr
};

static void set_or_unset(const char* name, const char* value) {
    if (value) setenv(name, value, 1); else unsetenv(name);
}

static int run_case(const Case& c, uint64_t gen, int policy) {
    const int n = c.n, L = c.L, B = c.batch;
    const int64_t lds = c.lds ? c.lds : L, ld = c.ld ? c.ld : n, stride = c.stride ? c.stride : (int64_t)n * ld;
    const size_t seq_bytes = (size_t)((int64_t)(n - 1) * lds + L), out_elems = (size_t)((int64_t)(B - 1) * stride + (int64_t)(n - 1) * ld + n);
    uint8_t* seq = (uint8_t*)std::malloc(seq_bytes);
    double* out = (double*)std::malloc(sizeof(double) * out_elems);
    double* want = (double*)std::malloc(sizeof(double) * out_elems);
    if (!seq || !out || !want) return 1;
    uint64_t s = gen;
    for (size_t k = 0; k < seq_bytes; k++) seq[k] = (uint8_t)"ACGT"[splitmix64(s) & 3];  // (padding: states that would change the result if read)
    std::vector<uint8_t> base((size_t)L);
    for (int k = 0; k < L; k++) base[(size_t)k] = (uint8_t)"ACGT"[splitmix64(s) & 3];
    for (int i = 0; i < n; i++)
        for (int k = 0; k < L; k++) {
            uint8_t v = splitmix64(s) % 100 < 10 ? (uint8_t)"ACGT"[splitmix64(s) & 3] : base[(size_t)k];
            if ((int)(splitmix64(s) % 100) < c.missing_pct) v = FNN_SITE_MISSING;
            seq[(size_t)((int64_t)i * lds + k)] = v;
        }
    std::memset(out, 0xFF, sizeof(double) * out_elems);
    std::memset(want, 0xFF, sizeof(double) * out_elems);
    fnn_dist_model m{};
    m.model = c.model;
    m.states = 4;
    m.on_saturation = policy;
    m.cap = policy == FNN_DIST_SAT_CAP ? 12.5 : 0.0;
    // the counts entry on the definition's counts, into the same layout (in place: so that a failure leaves what it leaves)
    const std::vector<uint16_t> counts = definition(L, B, c.seed, c.lead);
    unsetenv("FNN_BATCH_CHUNK");
    unsetenv("FNN_DIST_FORCE_DIGITS");
    unsetenv("FNN_DRAW_ROUTE");
    fnn_dist_model_stats mst{};
    const int32_t rc_want = emu_alignment_distances_model_batch_f64(seq, n, L, lds, counts.data(), B, L, &m, 0, want, ld, stride, &mst);
    const std::string msg_want = emu_last_error();
    set_or_unset("FNN_BATCH_CHUNK", c.chunk);
    set_or_unset("FNN_DIST_FORCE_DIGITS", c.digits);
    set_or_unset("FNN_DRAW_ROUTE", c.route);
    fnn_boot_stats st{};
    const int32_t rc = (c.in_place ? emu_bootstrap_distances_batch_device_f64 : emu_bootstrap_distances_batch_f64)(seq, n, L, lds, B, c.seed, c.lead, &m, 0, out,
                                                                                                                   ld, stride, &st);
    const std::string msg = emu_last_error();
    int bad = 0;
    char tag[128];
    std::snprintf(tag, sizeof(tag), "model=%d policy=%d n=%d L=%d batch=%d lead=%d", c.model, policy, n, L, B, c.lead);
    if (rc != rc_want) { std::fprintf(stderr, "%s: status %d (%s), the counts entry's is %d (%s)\n", tag, rc, msg.c_str(), rc_want, msg_want.c_str()); bad = 1; }
    if (!bad && rc != FNN_OK) {
        // the same pair named (behind the entry's name), the host output untouched
        const size_t p0 = msg.find(": "), p1 = msg_want.find(": ");
        if (p0 == std::string::npos || p1 == std::string::npos || msg.substr(p0) != msg_want.substr(p1)) {
            std::fprintf(stderr, "%s: \"%s\" against \"%s\"\n", tag, msg.c_str(), msg_want.c_str());
            bad = 1;
        }
        for (size_t k = 0; k < out_elems && !bad && !c.in_place; k++) {
            uint64_t bits;
            std::memcpy(&bits, &out[k], 8);
            if (bits != ~0ull) { std::fprintf(stderr, "%s: the output was written although the call failed\n", tag); bad = 1; }
        }
    }
    if (!bad && rc == FNN_OK) {
        if (std::memcmp(out, want, sizeof(double) * out_elems) != 0) { std::fprintf(stderr, "%s: the matrices differ from the counts entry's\n", tag); bad = 1; }
        const int want_route = c.route ? (std::strcmp(c.route, "host") == 0 ? FNN_DRAW_HOST : FNN_DRAW_DEVICE) : FNN_DRAW_DEVICE;
        const int want_digits = c.digits ? std::atoi(c.digits) : 1;
        uint32_t most = 0;
        for (uint16_t x : counts) most = x > most ? x : most;
        if (st.draw_route != want_route || st.model.base.digit_passes != want_digits || st.max_count != (int32_t)most ||
            st.model.n_saturated_problems != mst.n_saturated_problems || st.model.base.has_missing != mst.base.has_missing) {
            std::fprintf(stderr, "%s: route %d, %d digit passes, largest count %d\n", tag, st.draw_route, st.model.base.digit_passes, st.max_count);
            bad = 1;
        }
    }
    std::free(seq);
    std::free(out);
    std::free(want);
    return bad;
}

int main() {
    const int P = FNN_DIST_P, J = FNN_DIST_JC69, K = FNN_DIST_K2P;
    const uint64_t M64 = ~0ull;
    if (emu_bootstrap_draw_max_sites() < 30000) { std::fprintf(stderr, "the site limit is below 30000\n"); return 1; }
    const struct { int64_t L, batch; uint64_t seed; int64_t lead; int digits; } planes[] = {
        {1, 1, 0, 0, 1}, {15, 15, 7, 0, 1}, {17, 16, M64, 1, 2}, {64, 64, 3, 0, 3}, {65, 65, 7, 1, 1}, {130, 70, 5, 0, 2}, {200, 63, 7, 1, 1},
        {4097, 3, 11, 1, 3}, {32768, 2, 7, 0, 1}};
    int np = 0;
    for (const auto& p : planes) {
        if (check_planes(p.L, p.batch, p.seed, p.lead, p.digits)) return 1;
        np++;
    }
    const Case cases[] = {
        // shape edges, every model, without and with missing bytes (at few sites some replicates have empty or saturated pairs:
        // named as the counts entry names them, or capped)
        {P, 1, 1, 1, 0, 0, 0, 0, 0, 0, false, nullptr, nullptr, nullptr},       {K, 2, 15, 15, 0, 5, 7, 0, 0, 0, false, nullptr, nullptr, nullptr},
        {J, 5, 16, 16, 1, 5, M64, 0, 0, 0, false, nullptr, nullptr, nullptr},   {K, 17, 17, 17, 0, 0, 0, 0, 0, 0, false, nullptr, nullptr, nullptr},
        {P, 33, 63, 63, 1, 5, 7, 0, 0, 0, false, nullptr, nullptr, nullptr},    {J, 2, 64, 64, 0, 0, M64, 0, 0, 0, false, nullptr, nullptr, nullptr},
        {K, 5, 65, 65, 1, 5, 0, 0, 0, 0, false, nullptr, nullptr, nullptr},     {J, 17, 130, 70, 0, 5, 7, 0, 0, 0, false, nullptr, nullptr, nullptr},
        {P, 33, 200, 1, 1, 0, M64, 0, 0, 0, false, nullptr, nullptr, nullptr},  {K, 3, 8, 40, 0, 30, 3, 0, 0, 0, false, nullptr, nullptr, nullptr},
        {J, 3, 4, 40, 1, 0, 4, 0, 0, 0, true, nullptr, nullptr, nullptr},
        // forced digit planes; K2P with three of them and missing bytes at 65 problems: two replicate tiles per wave
        {P, 7, 65, 17, 1, 5, 7, 0, 0, 0, false, nullptr, "2", nullptr},         {K, 7, 65, 65, 0, 10, 7, 0, 0, 0, false, nullptr, "3", nullptr},
        {J, 7, 65, 17, 1, 0, 7, 0, 0, 0, true, nullptr, "3", nullptr},
        // layout, both entries, chunks, the host route
        {K, 7, 65, 7, 1, 10, 5, 70, 9, 74, false, nullptr, nullptr, nullptr},   {K, 7, 65, 7, 1, 10, 5, 70, 9, 74, true, nullptr, nullptr, nullptr},
        {K, 7, 65, 7, 1, 10, 5, 0, 9, 70, false, "3", nullptr, nullptr},        {J, 7, 65, 7, 0, 10, 5, 0, 9, 70, true, "3", "2", nullptr},
        {P, 7, 65, 7, 1, 10, 5, 70, 9, 74, false, "3", nullptr, "host"},        {K, 5, 130, 9, 0, 5, 6, 0, 0, 0, true, nullptr, nullptr, "host"},
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
    unsetenv("FNN_DIST_FORCE_DIGITS");
    unsetenv("FNN_DRAW_ROUTE");
    std::printf("ok: %d plane cases, %d cases, %d runs\n", np, k, runs);
    return 0;
}

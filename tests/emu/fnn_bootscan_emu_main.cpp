// fnn_bootscan_emu_main.cpp -- TEST INFRASTRUCTURE: stand-alone program over the CPU driver of the bootscan entries
// (fnn_bootscan_emu.cpp), meant to be built with -fsanitize=address,undefined, as fnn_dist_ranges_emu_main.cpp is for the site
// ranges.
//
// Runs cases of tests/bootscan_common.py - every window boundary, column groups across 16 and 64 rows, window sets under every
// model without and with missing bytes, chunks that split windows, the host route and the forced second digit, failures.  Every
// bootscan call is compared with the driver's counts entry on the rows of emus_bootscan_counts: the same status, the same message
// behind the entry's name, the same words in the whole output array.  The caller's arrays are heap blocks of EXACTLY the declared
// sizes, the outputs filled with 0xFF bytes first; the output's padding - and after a failure of the host entry all of it - must
// still hold those bytes.  Exit status 0: all well.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/fastnn.h"

extern "C" {
const char* emus_last_error(void);
int32_t emus_bootscan_counts(int64_t L, const int64_t* starts, const int64_t* ends, int64_t windows, int64_t replicates, int64_t lead, uint64_t seed,
                             int64_t first, int64_t count, uint16_t* counts_out);
int32_t emus_bootscan_distances_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts, const int64_t* ends, int64_t windows,
                                    int64_t replicates, uint64_t seed, int64_t lead, const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld,
                                    int64_t stride, fnn_scan_stats* stats);
int32_t emus_bootscan_distances_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts, const int64_t* ends, int64_t windows,
                                           int64_t replicates, uint64_t seed, int64_t lead, const fnn_dist_model* m, int32_t device, double* D_out,
                                           int64_t ld, int64_t stride, fnn_scan_stats* stats);
int32_t emus_bootscan_pair_counts_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts, const int64_t* ends, int64_t windows,
                                      int64_t replicates, uint64_t seed, int64_t lead, const fnn_dist_model* m, int32_t device, int64_t* F_out, int64_t ld,
                                      int64_t stride, fnn_scan_stats* stats);
int32_t emus_bootscan_pair_counts_device_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts, const int64_t* ends,
                                             int64_t windows, int64_t replicates, uint64_t seed, int64_t lead, const fnn_dist_model* m, int32_t device,
                                             int64_t* F_out, int64_t ld, int64_t stride, fnn_scan_stats* stats);
int32_t emus_alignment_distances_model_batch_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch, int64_t ldc,
                                                 const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                 fnn_dist_model_stats* stats);
int32_t emus_alignment_distances_model_batch_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch,
                                                        int64_t ldc, const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                        fnn_dist_model_stats* stats);
int32_t emus_alignment_pair_counts_batch_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch, int64_t ldc,
                                             int32_t device, int64_t* F_out, int64_t ld, int64_t stride, fnn_dist_model_stats* stats);
int32_t emus_alignment_pair_counts_batch_device_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch,
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

// 4-state rows at about 10 % divergence, `missing` per mille of the bytes 255; (n - 1) * lds + L bytes
static std::vector<uint8_t> alignment(int n, int L, int64_t lds, uint64_t seed, int missing) {
    std::vector<uint8_t> b((size_t)((n - 1) * lds + L), (uint8_t)'T');
    std::vector<uint8_t> base((size_t)L);
    for (int s = 0; s < L; s++) base[(size_t)s] = (uint8_t)"ACGT"[splitmix64(seed) & 3];
    for (int i = 0; i < n; i++)
        for (int s = 0; s < L; s++) {
            uint8_t c = splitmix64(seed) % 10 == 0 ? (uint8_t)"ACGT"[splitmix64(seed) & 3] : base[(size_t)s];
            if ((int)(splitmix64(seed) % 1000) < missing) c = 255;
            b[(size_t)(i * lds + s)] = c;
        }
    return b;
}

template <class T>
static T* exact(const std::vector<T>& v) {  // a heap block of exactly the vector's bytes
    T* p = (T*)std::malloc(v.size() * sizeof(T) + (v.empty() ? 1 : 0));
    if (!v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

static int g_failed = 0, g_calls = 0;
static void expect(bool ok, const std::string& what) {
    if (!ok) { std::printf("FAILED: %s\n", what.c_str()); g_failed++; }
}
static std::string tail(const char* msg) {  // the message behind the entry's name
    const std::string s(msg ? msg : "");
    const size_t at = s.find(": ");
    return at == std::string::npos ? s : s.substr(at + 2);
}

struct Case {
    int n, L;
    int64_t lds, ld, pad;  // stride = cell * n * ld + pad
    Ranges ranges;
    int64_t R, lead;
    uint64_t seed;
    int model;
    double shape;
    int policy;
    double cap;
    int missing;
    bool in_place;
};

// one bootscan call against the counts entry on the rows of emus_bootscan_counts; returns the status
static int32_t run(const Case& c, const std::string& name, int64_t* host_chunks = nullptr) {
    g_calls++;
    const bool tables = c.model == TABLES;
    const int64_t W = (int64_t)c.ranges.size(), P = c.R + c.lead, B = W * P, cell = tables ? 16 : 1, stride = cell * c.n * c.ld + c.pad;
    std::vector<int64_t> s, e;
    for (const auto& r : c.ranges) { s.push_back(r.first); e.push_back(r.second); }
    uint8_t* seq = exact(alignment(c.n, c.L, c.lds, 4242 + (uint64_t)c.n, c.missing));
    int64_t *starts = exact(s), *ends = exact(e);
    const size_t words = (size_t)(B > 0 ? (B - 1) * stride + ((int64_t)(c.n - 1) * c.ld + c.n) * cell : 0);
    double* got = (double*)std::malloc(words * 8 + 1);
    double* want = (double*)std::malloc(words * 8 + 1);
    std::memset(got, 0xFF, words * 8);
    std::memset(want, 0xFF, words * 8);
    uint16_t* counts = (uint16_t*)std::malloc((size_t)(B * c.L) * 2 + 1);
    expect(emus_bootscan_counts(c.L, starts, ends, W, c.R, c.lead, c.seed, 0, B, counts) == 0, name + ": counts");
    fnn_dist_model_rates mr{};
    mr.base.model = tables ? 0 : c.model;
    mr.base.states = 4;
    mr.base.on_saturation = c.policy;
    mr.base.cap = c.cap;
    if (c.shape > 0.0) { mr.base.reserved = FNN_DIST_RATES_GAMMA; mr.shape = c.shape; }
    fnn_scan_stats st{};
    fnn_dist_model_stats cst{};
    int32_t rg, rw;
    if (tables) {
        rg = (c.in_place ? emus_bootscan_pair_counts_device_i64 : emus_bootscan_pair_counts_i64)(seq, c.n, c.L, c.lds, starts, ends, W, c.R, c.seed, c.lead, nullptr,
                                                                                               0, (int64_t*)got, c.ld, stride, &st);
        const std::string mg = tail(emus_last_error());
        rw = (c.in_place ? emus_alignment_pair_counts_batch_device_i64 : emus_alignment_pair_counts_batch_i64)(seq, c.n, c.L, c.lds, counts, B, c.L, 0,
                                                                                                             (int64_t*)want, c.ld, stride, &cst);
        expect(rg == rw && (rg == 0 || mg == tail(emus_last_error())), name + ": status or message");
    } else {
        rg = (c.in_place ? emus_bootscan_distances_device_f64 : emus_bootscan_distances_f64)(seq, c.n, c.L, c.lds, starts, ends, W, c.R, c.seed, c.lead, &mr.base, 0,
                                                                                           got, c.ld, stride, &st);
        const std::string mg = tail(emus_last_error());
        rw = (c.in_place ? emus_alignment_distances_model_batch_device_f64 : emus_alignment_distances_model_batch_f64)(seq, c.n, c.L, c.lds, counts, B, c.L,
                                                                                                                     &mr.base, 0, want, c.ld, stride, &cst);
        expect(rg == rw && (rg == 0 || mg == tail(emus_last_error())), name + ": status or message (" + mg + " / " + tail(emus_last_error()) + ")");
    }
    if (rg == 0 || !c.in_place) expect(std::memcmp(got, want, words * 8) == 0, name + ": output words");
    if (rg == 0) expect(st.n_windows == W && st.boot.model.base.n_problems == B, name + ": stats");
    if (host_chunks) *host_chunks = st.n_host_chunks;
    std::free(seq); std::free(starts); std::free(ends); std::free(got); std::free(want); std::free(counts);
    return rg;
}

int main() {
    const int P_ = FNN_DIST_P, JC69 = FNN_DIST_JC69, K2P = FNN_DIST_K2P, TN93 = FNN_DIST_TN93;
    // every window boundary
    Ranges every;
    for (int64_t s : {0, 1, 15, 16, 63, 64, 65})
        for (int64_t w : {1, 15, 16, 17, 63, 64, 65, 130}) every.push_back({s, s + w});
    every.push_back({190, 200});
    for (int model : {P_, TABLES}) run(Case{6, 200, 200, 6, 0, every, 3, 1, 7, model, 0.0, 0, 0.0, 0, false}, "boundaries");
    // column groups
    const Ranges two = {{3, 93}, {70, 200}};
    for (int64_t P : {1, 3, 16, 17, 64, 65, 66})
        for (int64_t lead : {0, 1})
            for (int model : {P_, K2P, TABLES}) run(Case{3, 200, 205, 5, 5, two, P - lead, lead, 11, model, 0.0, 0, 0.0, 0, lead == 1}, "groups");
    // window sets under every model
    const std::vector<Ranges> sets = {{{0, 64}, {40, 104}, {80, 144}, {120, 184}, {136, 200}}, {{1, 131}, {15, 80}, {63, 128}, {65, 195}, {16, 200}},
                                      {{0, 200}, {50, 150}, {50, 150}, {100, 164}}};
    const std::pair<int, double> models[] = {{P_, 0.0}, {FNN_DIST_JC69, 0.0}, {K2P, 0.0}, {FNN_DIST_F81, 0.0}, {FNN_DIST_F84, 0.0}, {TN93, 0.0},
                                             {FNN_DIST_LOGDET, 0.0}, {K2P, 0.5}, {TN93, 0.5}, {TABLES, 0.0}};
    for (const Ranges& set : sets)
        for (int missing : {0, 20})
            for (const auto& m : models)
                if (missing || m.first == P_ || m.first == K2P || m.first == TABLES)  // (without missing bytes: one kernel of each kind)
                    run(Case{6, 200, 203, 7, 3, set, 5, 1, 0x8000000000000005ULL, m.first, m.second, 1, 9.5, missing, missing != 0}, "grid");
    // chunks that split windows; the host route; a forced second digit
    for (int model : {K2P, TN93, TABLES})
        for (bool in_place : {false, true}) {
            const Case c{6, 200, 207, 9, 7, sets[2], 4, 1, 3, model, 0.0, 1, 9.5, 20, in_place};
            setenv("FNN_BATCH_CHUNK", "3", 1);
            run(c, "chunks");
            setenv("FNN_DIST_FORCE_DIGITS", "2", 1);
            int64_t hc = 0;
            run(c, "chunks, forced digits", &hc);
            expect(hc == 7, "forced digits: n_host_chunks");
            unsetenv("FNN_DIST_FORCE_DIGITS");
            unsetenv("FNN_BATCH_CHUNK");
            setenv("FNN_DRAW_ROUTE", "host", 1);
            run(c, "host route");
            unsetenv("FNN_DRAW_ROUTE");
        }
    // failures: an empty window below a non-empty one, without and with missing bytes
    const Ranges holes = {{0, 100}, {50, 50}, {100, 200}, {64, 64}};
    for (int missing : {0, 20})
        for (int model : {P_, K2P, TN93})
            for (bool in_place : {false, true})
                expect(run(Case{4, 200, 200, 4, 0, holes, 2, 1, 5, model, 0.0, 0, 0.0, missing, in_place}, "empty window") == FNN_EINVAL, "empty window: status");
    expect(run(Case{4, 200, 200, 4, 0, holes, 2, 1, 5, TABLES, 0.0, 0, 0.0, 20, false}, "empty window, tables") == 0, "empty window, tables: status");
    // tiny windows: saturated and empty pairs of single replicates, under both policies
    const Ranges tiny = {{0, 8}, {8, 16}, {16, 24}, {3, 5}};
    for (uint64_t seed = 0; seed < 6; seed++)
        for (int model : {JC69, K2P, TN93})
            for (int policy : {0, 1}) run(Case{3, 24, 24, 3, 0, tiny, 6, 1, seed, model, 0.0, policy, 7.5, 100, false}, "tiny windows");
    if (g_failed) { std::printf("%d of %d calls failed\n", g_failed, g_calls); return 1; }
    std::printf("ok: %d calls\n", g_calls);
    return 0;
}

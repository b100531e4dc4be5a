// fnn_support_emu_main.cpp -- TEST INFRASTRUCTURE: stand-alone program over the CPU driver of the split-support stage
// (fnn_support_emu.cpp), meant to be built with -fsanitize=address,undefined: an index past a record, table, row or segment
// buffer is silent on the GPU, here it ends the program.
//
// Runs word-edge shapes on generated inputs - rotations and reflections of one circular order, sparse positive weights -
// through both entries, in chunks, with a hash cut to a few bits and with the workgroups of every launch reversed, and
// compares every byte of the table with a plain loop over the definition (taxon sets as byte vectors, rows in a vector
// searched linearly).  The caller's arrays are heap blocks of EXACTLY the declared sizes: B (n + 1) ints, B n(n-1)/2 doubles,
// S rows of output.  Exit status 0: all well.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/fastnn.h"

extern "C" {
const char* emu_last_error(void);
void emu_support_set_reverse(int32_t on);
int32_t emu_split_support_f64(int32_t n, int64_t batch, const int32_t* orderings, const double* weights, double threshold, int64_t lead, int32_t device,
                              uint64_t* keys_out, int64_t* first_b_out, int64_t* first_k_out, int64_t* counts_out, double* weight_sum_out,
                              int64_t capacity, int64_t* count_out, fnn_support_stats* stats);
int32_t emu_split_support_device_f64(int32_t n, int64_t batch, const int32_t* orderings, const double* d_weights, double threshold, int64_t lead,
                                     int32_t device, uint64_t* keys_out, int64_t* first_b_out, int64_t* first_k_out, int64_t* counts_out,
                                     double* weight_sum_out, int64_t capacity, int64_t* count_out, fnn_support_stats* stats);
}

static uint64_t splitmix64(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

struct Case {
    int n, B, lead;
    bool in_place, reverse;
    const char *chunk, *bits;  // FNN_BATCH_CHUNK, FNN_SUPPORT_HASH_BITS or nullptr
    int route, retries;        // expected
};

struct RefRow { std::vector<uint8_t> set; int64_t b, k, count; double sum; };

static int run_case(const Case& c, uint64_t seed) {
    const int n = c.n, B = c.B, words = (n + 63) / 64;
    const int64_t K = (int64_t)n * (n - 1) / 2;
    int32_t* ord = (int32_t*)std::malloc(sizeof(int32_t) * (size_t)B * (size_t)(n + 1));
    double* w = (double*)std::malloc(sizeof(double) * (size_t)B * (size_t)K);
    if (!ord || !w) return 1;
    uint64_t s = seed;
    std::vector<int32_t> base((size_t)n);
    for (int t = 0; t < n; t++) base[(size_t)t] = t + 1;
    for (int t = n - 1; t > 0; t--) { const int u = (int)(splitmix64(s) % (uint64_t)(t + 1)); const int32_t x = base[(size_t)t]; base[(size_t)t] = base[(size_t)u]; base[(size_t)u] = x; }
    for (int b = 0; b < B; b++) {
        const int rot = (int)(splitmix64(s) % (uint64_t)n);
        const bool refl = splitmix64(s) & 1;
        ord[(size_t)b * (size_t)(n + 1)] = 0;
        for (int p = 0; p < n; p++) ord[(size_t)b * (size_t)(n + 1) + 1 + (size_t)(refl ? n - 1 - p : p)] = base[(size_t)((p + rot) % n)];
        for (int64_t k = 0; k < K; k++) w[(size_t)b * (size_t)K + (size_t)k] = 0.0;
        const int cnt = 3 * n < K ? 3 * n : (int)K;
        for (int q = 0; q < cnt; q++) w[(size_t)b * (size_t)K + (size_t)(splitmix64(s) % (uint64_t)K)] = 0.01 + (double)(splitmix64(s) >> 11) * 0x1.0p-53;
        if (K >= 4) w[(size_t)b * (size_t)K + (size_t)(splitmix64(s) % (uint64_t)K)] = -1.0;
    }
    // the definition
    std::vector<RefRow> ref;
    std::vector<uint8_t> set((size_t)n);
    for (int b = 0; b < B; b++) {
        int64_t k = 0;
        for (int i = 0; i < n - 1; i++)
            for (int j = i + 1; j < n; j++, k++) {
                const double x = w[(size_t)b * (size_t)K + (size_t)k];
                if (!(x > 1e-6)) continue;
                std::fill(set.begin(), set.end(), (uint8_t)0);
                for (int p = i + 1; p <= j; p++) set[(size_t)(ord[(size_t)b * (size_t)(n + 1) + (size_t)p] - 1)] = 1;
                if (set[0]) for (int t = 0; t < n; t++) set[(size_t)t] ^= 1;
                size_t r = 0;
                while (r < ref.size() && ref[r].set != set) r++;
                if (r == ref.size()) ref.push_back(RefRow{set, b, k, 0, 0.0});
                if (b >= c.lead) { ref[r].count++; ref[r].sum = ref[r].sum + x; }
            }
    }
    const int64_t S = (int64_t)ref.size();
    uint64_t* keys = (uint64_t*)std::malloc(8 * (size_t)S * (size_t)words);
    int64_t* fb = (int64_t*)std::malloc(8 * (size_t)S);
    int64_t* fk = (int64_t*)std::malloc(8 * (size_t)S);
    int64_t* cn = (int64_t*)std::malloc(8 * (size_t)S);
    double* sm = (double*)std::malloc(8 * (size_t)S);
    if (!keys || !fb || !fk || !cn || !sm) return 1;
    if (c.chunk) setenv("FNN_BATCH_CHUNK", c.chunk, 1); else unsetenv("FNN_BATCH_CHUNK");
    if (c.bits) setenv("FNN_SUPPORT_HASH_BITS", c.bits, 1); else unsetenv("FNN_SUPPORT_HASH_BITS");
    setenv("FNN_SUPPORT_ROUTE", "kernel", 1);
    emu_support_set_reverse(c.reverse ? 1 : 0);
    fnn_support_stats st{};
    int64_t got = -1;
    const int32_t rc = (c.in_place ? emu_split_support_device_f64 : emu_split_support_f64)(n, B, ord, w, 1e-6, c.lead, 0, keys, fb, fk, cn, sm, S, &got, &st);
    int bad = 0;
    if (rc != FNN_OK) { std::fprintf(stderr, "n=%d B=%d: status %d (%s)\n", n, B, rc, emu_last_error()); bad = 1; }
    if (!bad && (got != S || st.n_splits != S)) { std::fprintf(stderr, "n=%d B=%d: %lld rows, expected %lld\n", n, B, (long long)got, (long long)S); bad = 1; }
    if (!bad && (st.route != c.route || st.hash_retries != c.retries)) {
        std::fprintf(stderr, "n=%d B=%d: route %d after %d repeats, expected %d after %d\n", n, B, st.route, st.hash_retries, c.route, c.retries);
        bad = 1;
    }
    for (int64_t r = 0; r < S && !bad; r++) {
        const RefRow& R = ref[(size_t)r];
        for (int t = 0; t < words * 64 && !bad; t++) {
            const int bit = (int)((keys[(size_t)r * (size_t)words + (size_t)(t / 64)] >> (t % 64)) & 1);
            if (bit != (t < n ? (int)R.set[(size_t)t] : 0)) { std::fprintf(stderr, "n=%d B=%d: row %lld, key bit %d\n", n, B, (long long)r, t); bad = 1; }
        }
        if (!bad && (fb[r] != R.b || fk[r] != R.k || cn[r] != R.count || std::memcmp(&sm[r], &R.sum, 8) != 0)) {
            std::fprintf(stderr, "n=%d B=%d: row %lld is (%lld, %lld, %lld, %.17g), expected (%lld, %lld, %lld, %.17g)\n", n, B, (long long)r,
                         (long long)fb[r], (long long)fk[r], (long long)cn[r], sm[r], (long long)R.b, (long long)R.k, (long long)R.count, R.sum);
            bad = 1;
        }
    }
    std::free(ord); std::free(w); std::free(keys); std::free(fb); std::free(fk); std::free(cn); std::free(sm);
    return bad;
}

int main() {
    const Case cases[] = {
        // word edges, both entries
        {2, 1, 0, false, false, nullptr, nullptr, 0, 0},   {3, 2, 0, true, false, nullptr, nullptr, 0, 0},
        {5, 17, 0, false, false, nullptr, nullptr, 0, 0},  {63, 2, 0, true, false, nullptr, nullptr, 0, 0},
        {64, 17, 1, false, false, nullptr, nullptr, 0, 0}, {65, 2, 0, true, false, nullptr, nullptr, 0, 0},
        {128, 2, 0, false, false, nullptr, nullptr, 0, 0}, {129, 3, 1, true, false, nullptr, nullptr, 0, 0},
        {140, 5, 0, false, false, nullptr, nullptr, 0, 0}, {141, 2, 2, true, false, nullptr, nullptr, 0, 0},
        {1024, 2, 0, false, false, nullptr, nullptr, 0, 0},
        // chunks and the carry, reversed workgroups, a hash of 3 bits (every seed collides: the host route) and of 64
        {65, 7, 1, false, false, "3", nullptr, 0, 0},      {65, 7, 1, true, true, "3", nullptr, 0, 0},
        {33, 7, 0, false, true, "1", nullptr, 0, 0},       {140, 5, 0, false, true, nullptr, nullptr, 0, 0},
        {33, 5, 0, false, false, nullptr, "3", 1, 3},      {33, 5, 0, true, true, "2", "3", 1, 3},
        {33, 5, 0, false, false, nullptr, "64", 0, 0},
    };
    int k = 0;
    for (const Case& c : cases)
        if (run_case(c, 5000 + (uint64_t)(k++))) return 1;
    std::printf("ok: %d cases\n", k);
    return 0;
}

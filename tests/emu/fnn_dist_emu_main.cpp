// fnn_dist_emu_main.cpp -- TEST INFRASTRUCTURE: stand-alone program over the CPU driver of the alignment-distance path
// (fnn_dist_emu.cpp), meant to be built with -fsanitize=address,undefined: a 16-byte operand load that leaves its buffer is
// silent on the GPU, here it ends the program.
//
// Runs the shape, digit-plane, missing-data and layout cases of tests/dist_common.py on generated inputs and compares every
// entry with a plain loop over the definition.  The caller's arrays are heap blocks of EXACTLY the declared sizes -
// (n - 1) lds + L bytes, (B - 1) ldc + L counts, (B - 1) stride + (n - 1) ld + n doubles -, filled with 0xFF bytes first: a read
// or a write past the last element is an error, and the output's padding must still hold those bytes afterwards.
// Exit status 0: all well.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/fastnn.h"

extern "C" {
const char* emu_last_error(void);
int32_t emu_alignment_distances_batch_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch, int64_t ldc,
                                          int32_t model, int32_t device, double* D_out, int64_t ld, int64_t stride, fnn_dist_stats* stats);
int32_t emu_alignment_distances_batch_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch,
                                                 int64_t ldc, int32_t model, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                 fnn_dist_stats* stats);
}

static uint64_t splitmix64(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

struct Case {
    int n, L, B, cmax, missing_pct;  // missing_pct: per cent of bytes 255
    int64_t lds, ldc, ld, stride;    // 0: dense
    bool in_place;
    const char* chunk;               // FNN_BATCH_CHUNK or nullptr
    int passes;                      // expected digit_passes
};

static int run_case(const Case& c, uint64_t seed) {
    const int n = c.n, L = c.L, B = c.B;
    const int64_t lds = c.lds ? c.lds : L, ldc = c.ldc ? c.ldc : L, ld = c.ld ? c.ld : n, stride = c.stride ? c.stride : (int64_t)n * ld;
    const size_t seq_bytes = (size_t)((int64_t)(n - 1) * lds + L), cnt_elems = (size_t)((int64_t)(B - 1) * ldc + L);
    const size_t out_elems = (size_t)((int64_t)(B - 1) * stride + (int64_t)(n - 1) * ld + n);
    uint8_t* seq = (uint8_t*)std::malloc(seq_bytes);
    uint16_t* cnt = (uint16_t*)std::malloc(sizeof(uint16_t) * cnt_elems);
    double* out = (double*)std::malloc(sizeof(double) * out_elems);
    if (!seq || !cnt || !out) return 1;
    uint64_t s = seed;
    // padding: states and counts that would change the result if read
    for (size_t k = 0; k < seq_bytes; k++) seq[k] = (uint8_t)"ACGT"[splitmix64(s) & 3];
    for (size_t k = 0; k < cnt_elems; k++) cnt[k] = 999;
    std::memset(out, 0xFF, sizeof(double) * out_elems);
    std::vector<uint8_t> base((size_t)L);
    for (int k = 0; k < L; k++) base[(size_t)k] = (uint8_t)"ACGT"[splitmix64(s) & 3];
    for (int i = 0; i < n; i++)
        for (int k = 0; k < L; k++) {
            uint8_t v = splitmix64(s) % 10 == 0 ? (uint8_t)"ACGT"[splitmix64(s) & 3] : base[(size_t)k];
            if ((int)(splitmix64(s) % 100) < c.missing_pct) v = FNN_SITE_MISSING;
            seq[(size_t)((int64_t)i * lds + k)] = v;
        }
    for (int b = 0; b < B; b++)
        for (int k = 0; k < L; k++) cnt[(size_t)((int64_t)b * ldc + k)] = (uint16_t)(1 + splitmix64(s) % (uint64_t)c.cmax);
    cnt[(size_t)((int64_t)(B / 2) * ldc + L / 2)] = (uint16_t)c.cmax;
    if (c.chunk) setenv("FNN_BATCH_CHUNK", c.chunk, 1); else unsetenv("FNN_BATCH_CHUNK");
    fnn_dist_stats st{};
    const int32_t rc = (c.in_place ? emu_alignment_distances_batch_device_f64 : emu_alignment_distances_batch_f64)(
        seq, n, L, lds, cnt, B, ldc, FNN_DIST_P, 0, out, ld, stride, &st);
    int bad = 0;
    if (rc != FNN_OK) { std::fprintf(stderr, "n=%d L=%d B=%d: status %d (%s)\n", n, L, B, rc, emu_last_error()); bad = 1; }
    if (!bad && st.digit_passes != c.passes) { std::fprintf(stderr, "n=%d L=%d B=%d: %d digit passes, expected %d\n", n, L, B, st.digit_passes, c.passes); bad = 1; }
    std::vector<char> written(out_elems, 0);
    for (int b = 0; b < B && !bad; b++)
        for (int i = 0; i < n && !bad; i++)
            for (int j = 0; j < n && !bad; j++) {
                int64_t mism = 0, valid = 0;
                for (int k = 0; k < L; k++) {
                    const uint8_t x = seq[(size_t)((int64_t)i * lds + k)], y = seq[(size_t)((int64_t)j * lds + k)];
                    if (x == FNN_SITE_MISSING || y == FNN_SITE_MISSING) continue;
                    valid += cnt[(size_t)((int64_t)b * ldc + k)];
                    if (x != y) mism += cnt[(size_t)((int64_t)b * ldc + k)];
                }
                const double want = i == j ? 0.0 : (double)mism / (double)(valid ? valid : 1);
                const size_t at = (size_t)((int64_t)b * stride + (int64_t)i * ld + j);
                written[at] = 1;
                if (i != j && valid == 0) { std::fprintf(stderr, "n=%d L=%d B=%d: the generated case has an empty pair\n", n, L, B); bad = 1; }
                else if (std::memcmp(&out[at], &want, 8) != 0) {
                    std::fprintf(stderr, "n=%d L=%d B=%d: entry (%d, %d, %d) is %.17g, expected %.17g\n", n, L, B, b, i, j, out[at], want);
                    bad = 1;
                }
            }
    for (size_t k = 0; k < out_elems && !bad; k++) {
        uint64_t bits;
        std::memcpy(&bits, &out[k], 8);
        if (!written[k] && bits != ~0ull) { std::fprintf(stderr, "n=%d L=%d B=%d: output padding at %zu was written\n", n, L, B, k); bad = 1; }
    }
    std::free(seq);
    std::free(cnt);
    std::free(out);
    return bad;
}

int main() {
    const Case cases[] = {
        // shape edges (tests/dist_common.py SHAPES), every other long one with missing bytes
        {1, 1, 1, 127, 0, 0, 0, 0, 0, false, nullptr, 1},    {2, 15, 15, 127, 0, 0, 0, 0, 0, false, nullptr, 1},
        {3, 16, 16, 127, 0, 0, 0, 0, 0, false, nullptr, 1},  {5, 17, 17, 127, 0, 0, 0, 0, 0, false, nullptr, 1},
        {6, 63, 33, 127, 0, 0, 0, 0, 0, false, nullptr, 1},  {7, 64, 1, 127, 10, 0, 0, 0, 0, false, nullptr, 1},
        {17, 65, 15, 127, 0, 0, 0, 0, 0, false, nullptr, 1}, {33, 130, 16, 127, 10, 0, 0, 0, 0, false, nullptr, 1},
        {65, 1, 17, 127, 0, 0, 0, 0, 0, false, nullptr, 1},  {1, 130, 33, 127, 10, 0, 0, 0, 0, false, nullptr, 1},
        {2, 64, 17, 127, 0, 0, 0, 0, 0, false, nullptr, 1},  {3, 65, 1, 127, 10, 0, 0, 0, 0, false, nullptr, 1},
        {5, 63, 16, 127, 0, 0, 0, 0, 0, false, nullptr, 1},  {6, 16, 15, 127, 0, 0, 0, 0, 0, false, nullptr, 1},
        {7, 17, 33, 127, 0, 0, 0, 0, 0, false, nullptr, 1},  {17, 15, 1, 127, 0, 0, 0, 0, 0, false, nullptr, 1},
        {33, 1, 15, 127, 0, 0, 0, 0, 0, false, nullptr, 1},  {65, 130, 33, 127, 10, 0, 0, 0, 0, false, nullptr, 1},
        // digit planes, without and with missing bytes
        {7, 65, 17, 1, 0, 0, 0, 0, 0, false, nullptr, 1},      {7, 65, 17, 127, 10, 0, 0, 0, 0, false, nullptr, 1},
        {7, 65, 17, 128, 0, 0, 0, 0, 0, false, nullptr, 2},    {7, 65, 17, 16383, 10, 0, 0, 0, 0, false, nullptr, 2},
        {7, 65, 17, 16384, 0, 0, 0, 0, 0, false, nullptr, 3},  {7, 65, 17, 65535, 10, 0, 0, 0, 0, false, nullptr, 3},
        {7, 65, 17, 65535, 0, 0, 0, 0, 0, false, nullptr, 3},
        // missing data
        {9, 130, 5, 127, 10, 0, 0, 0, 0, false, nullptr, 1},
        // layout, both entries, and chunking
        {7, 65, 7, 300, 10, 70, 68, 9, 74, false, nullptr, 2}, {7, 65, 7, 300, 10, 70, 68, 9, 74, true, nullptr, 2},
        {7, 65, 7, 300, 0, 65, 66, 7, 50, false, nullptr, 2},  {7, 65, 7, 300, 0, 81, 65, 8, 56, true, nullptr, 2},
        {7, 65, 7, 300, 10, 0, 0, 9, 70, false, "3", 2},       {7, 65, 7, 300, 10, 0, 0, 9, 70, true, "3", 2},
    };
    int k = 0;
    for (const Case& c : cases)
        if (run_case(c, 4000 + (uint64_t)(k++))) return 1;
    unsetenv("FNN_BATCH_CHUNK");
    std::printf("ok: %d cases\n", k);
    return 0;
}

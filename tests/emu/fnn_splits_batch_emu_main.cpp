// fnn_splits_batch_emu_main.cpp -- TEST INFRASTRUCTURE: stand-alone program over the CPU driver of the batched circular split
// weights (fnn_splits_batch_emu.cpp), meant to be built with -fsanitize=address,undefined: an index past the LDS image or
// past a problem's workspace slice is silent on the GPU (or takes the machine down), here it ends the program.
//
//   fnn_splits_batch_emu_main [n ...]   (default sizes: 4 33 64 and the limit)  per size a batch of generated matrices
//                                 (uniform, ties to 4 decimals, a third negative, a dyadic ultrametric, a circular metric
//                                 of all splits with weight 1) under generated circular orders (the identity, a rotation-free
//                                 shuffle), by the host entry on dense problems and by both entries through a caller's layout
//                                 (padded rows, problems five doubles apart) in a heap block of exactly the size the contract
//                                 asks for, padding NaN.  Every problem must come back certified with weights >= 0, the
//                                 layouts must give the bits of the dense run, the circular metric must take the closed form
//                                 and give weight 1 everywhere, and the caller's block must be unchanged.
// Exit status 0: all well.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/fastnn.h"

extern "C" {
const char* emu_last_error(void);
int32_t emu_split_weights_batch_max_n(void);
int32_t emu_split_weights_batch_f64(const double* D, int32_t n, int64_t ld, int64_t stride, int64_t batch, const int32_t* orderings, int32_t device,
                                    double* weights_out, fnn_sw_stats* stats_out, fnn_sw_batch_stats* stats);
int32_t emu_split_weights_batch_device_f64(const double* D, int32_t n, int64_t ld, int64_t stride, int64_t batch, const int32_t* orderings,
                                           int32_t device, double* weights_out, fnn_sw_stats* stats_out, fnn_sw_batch_stats* stats);
}

static uint64_t splitmix64(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

constexpr int NCLS = 5;

// class 4: the circular metric of the identity order in which every split weighs 1: d(i, j) = (j - i) (n - (j - i))
static void generate(std::vector<double>& D, int n, int cls, uint64_t seed) {
    D.assign((size_t)n * n, 0.0);
    uint64_t s = seed;
    for (int i = 0; i < n; i++)
        for (int j = i + 1; j < n; j++) {
            const double u = (double)(splitmix64(s) >> 11) * 0x1.0p-53;
            double d = u + 0x1.0p-10;
            if (cls == 1) d = (double)((int64_t)(u * 1e4) + 1) / 1e4;
            if (cls == 2) d = u - 0.25;
            if (cls == 3) { int h = 0; for (int x = i ^ j; x; x >>= 1) h++; d = (double)h / 64.0; }
            if (cls == 4) d = (double)(j - i) * (double)(n - (j - i));
            D[(size_t)i * n + j] = D[(size_t)j * n + i] = d;
        }
}

static void make_order(std::vector<int32_t>& o, int n, int cls, uint64_t seed) {
    o.assign((size_t)n + 1, 0);
    for (int i = 1; i <= n; i++) o[(size_t)i] = i;
    if (cls == 4 || cls == 0) return;  // the identity
    uint64_t s = seed;
    for (int i = n; i > 2; i--) {      // positions 2 ... n shuffled, position 1 stays taxon 1
        const int j = 2 + (int)(splitmix64(s) % (uint64_t)(i - 1));
        const int32_t t = o[(size_t)i]; o[(size_t)i] = o[(size_t)j]; o[(size_t)j] = t;
    }
}

static int check(const std::vector<double>& w, const std::vector<fnn_sw_stats>& sw, const fnn_sw_batch_stats& st, int n, int B, const char* what) {
    const size_t N = (size_t)n * (n - 1) / 2;
    if (st.n_problems != B || st.n_fallback != 0 || st.n_kernel + st.n_closed_form != B) { std::fprintf(stderr, "%s: n=%d: wrong route\n", what, n); return 1; }
    for (int b = 0; b < B; b++) {
        if (!sw[(size_t)b].certified || !(sw[(size_t)b].kkt_violation <= 1e-9)) { std::fprintf(stderr, "%s: n=%d problem %d: not certified\n", what, n, b); return 1; }
        for (size_t k = 0; k < N; k++)
            if (!(w[(size_t)b * N + k] >= 0.0)) { std::fprintf(stderr, "%s: n=%d problem %d: weight %d is negative or NaN\n", what, n, b, (int)k); return 1; }
    }
    const int b = 4;  // the circular metric
    if (sw[(size_t)b].route != FNN_SW_ROUTE_CLOSED_FORM) { std::fprintf(stderr, "%s: n=%d: the circular metric did not take the closed form\n", what, n); return 1; }
    for (size_t k = 0; k < N; k++)
        if (std::fabs(w[(size_t)b * N + k] - 1.0) > 1e-9) { std::fprintf(stderr, "%s: n=%d: circular metric, weight %d is %.17g\n", what, n, (int)k, w[(size_t)b * N + k]); return 1; }
    return 0;
}

static int run_size(int n) {
    const int B = NCLS;
    const size_t N = (size_t)n * (n - 1) / 2;
    std::vector<double> all, one;
    std::vector<int32_t> orders, o;
    for (int cls = 0; cls < NCLS; cls++) {
        generate(one, n, cls, 2000 + (uint64_t)n * 8 + (uint64_t)cls);
        make_order(o, n, cls, 77 + (uint64_t)n + (uint64_t)cls);
        all.insert(all.end(), one.begin(), one.end());
        orders.insert(orders.end(), o.begin(), o.end());
    }
    std::vector<double> w(B * N, -7.0);
    std::vector<fnn_sw_stats> sw((size_t)B);
    fnn_sw_batch_stats st{};
    int32_t rc = emu_split_weights_batch_f64(all.data(), n, n, (int64_t)n * n, B, orders.data(), 0, w.data(), sw.data(), &st);
    if (rc != FNN_OK) { std::fprintf(stderr, "dense: n=%d: status %d (%s)\n", n, rc, emu_last_error()); return 1; }
    if (check(w, sw, st, n, B, "dense")) return 1;
    // the caller's layout in a block of EXACTLY the size the contract asks for: (B - 1) * stride + (n - 1) * ld + n doubles
    const int64_t ld = n + 1, stride = (int64_t)n * ld + 5;
    const size_t need = (size_t)((B - 1) * stride + (int64_t)(n - 1) * ld + n);
    double* buf = (double*)std::malloc(sizeof(double) * need);
    if (!buf) return 1;
    for (size_t k = 0; k < need; k++) buf[k] = std::nan("");
    for (int b = 0; b < B; b++)
        for (int r = 0; r < n; r++)
            for (int c = 0; c < n; c++) buf[(size_t)(b * stride + r * ld + c)] = all[((size_t)b * n + r) * n + c];
    std::vector<unsigned char> before((const unsigned char*)buf, (const unsigned char*)buf + sizeof(double) * need);
    int bad = 0;
    for (int k = 0; k < 2 && !bad; k++) {
        std::vector<double> w2(B * N, -7.0);
        std::vector<fnn_sw_stats> sw2((size_t)B);
        fnn_sw_batch_stats st2{};
        rc = (k == 0 ? emu_split_weights_batch_f64 : emu_split_weights_batch_device_f64)(buf, n, ld, stride, B, orders.data(), 0, w2.data(), sw2.data(), &st2);
        if (rc != FNN_OK) { std::fprintf(stderr, "layout: n=%d entry %d: status %d (%s)\n", n, k, rc, emu_last_error()); bad = 1; break; }
        if (check(w2, sw2, st2, n, B, "layout")) bad = 1;
        else if (std::memcmp(w.data(), w2.data(), sizeof(double) * w.size()) != 0) { std::fprintf(stderr, "layout: n=%d entry %d: other bits than the dense run\n", n, k); bad = 1; }
        else if (std::memcmp(before.data(), buf, before.size()) != 0) { std::fprintf(stderr, "layout: n=%d entry %d: the caller's block was written\n", n, k); bad = 1; }
    }
    std::free(buf);
    return bad;
}

int main(int argc, char** argv) {
    std::vector<int> sizes;
    for (int i = 1; i < argc; i++) sizes.push_back(std::atoi(argv[i]));
    if (sizes.empty()) sizes = {4, 33, 64, emu_split_weights_batch_max_n()};
    int cases = 0;
    for (int n : sizes) {
        if (n < 2 || n > emu_split_weights_batch_max_n()) { std::fprintf(stderr, "size %d is outside 2 ... %d\n", n, emu_split_weights_batch_max_n()); return 1; }
        if (run_size(n)) return 1;
        cases += NCLS;
    }
    std::printf("ok: %d problems\n", cases);
    return 0;
}

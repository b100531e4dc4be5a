// fnn_batch_global_emu_main.cpp -- TEST INFRASTRUCTURE: stand-alone program over the CPU driver of the batched path above the LDS limit
// (fnn_batch_global_emu.cpp), meant to be built with -fsanitize=address,undefined: an index past the LDS image or past a
// problem's working matrix is silent on the GPU (or takes the machine down), here it ends the program.  The program sets
// FNN_BATCH_ROUTE=global itself, so every size takes the route.
//
//   fnn_batch_global_emu_main     runs a fixed list of generated matrices (uniform, ties to 4 decimals, a third negative,
//                                 every taxon four times, a dyadic ultrametric) at the sizes below and checks that every
//                                 result is a circular order; each batch again through three caller layouts (problem stride
//                                 n*n + 1, padded rows, both) in heap blocks of exactly the size the contract asks for, by
//                                 the host entry and twice by the in-place ("device") entry, after which the block must
//                                 be unchanged
//   fnn_batch_global_emu_main FILE      also runs the cases of FILE and compares the orders with the ones recorded in it:
//                                 int32 ncases, then per case int32 n, int32 B, B*n*n doubles, B*(n+1) int32 orders
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
int32_t emu_batch_lds_max_n(void);
int32_t emu_batch_global_max_n(void);
int32_t emu_canonical_order_batch_device_f64(const double* D, int32_t n, int64_t ld, int64_t stride, int64_t batch, const fnn_opts* opts,
                                             int32_t* orders_out, fnn_event* events_out, int32_t* nevents_out, fnn_batch_stats* stats);
int32_t emu_canonical_order_batch_f64(const double* D, int32_t n, int64_t ld, int64_t stride, int64_t batch, const fnn_opts* opts,
                                      int32_t* orders_out, fnn_event* events_out, int32_t* nevents_out, fnn_batch_stats* stats);
}

static uint64_t splitmix64(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

static void generate(std::vector<double>& D, int n, int cls, uint64_t seed) {
    D.assign((size_t)n * n, 0.0);
    uint64_t s = seed;
    const int g = cls == 3 ? (n + 3) / 4 : n;  // class 3: taxon i is a copy of taxon i / 4
    std::vector<double> base((size_t)g * g, 0.0);
    for (int i = 0; i < g; i++)
        for (int j = i + 1; j < g; j++) {
            const double u = (double)(splitmix64(s) >> 11) * 0x1.0p-53;
            double d = u + 0x1.0p-10;
            if (cls == 1) d = (double)((int64_t)(u * 1e4) + 1) / 1e4;
            if (cls == 2) d = u - 0.25;
            if (cls == 4) { int h = 0; for (int x = i ^ j; x; x >>= 1) h++; d = (double)h / 64.0; }
            base[(size_t)i * g + j] = base[(size_t)j * g + i] = d;
        }
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) D[(size_t)i * n + j] = cls == 3 ? base[(size_t)(i / 4) * g + j / 4] : base[(size_t)i * g + j];
}

static int check_orders(const std::vector<int32_t>& orders, const std::vector<int32_t>& nev, int n, int B, const char* what) {
    for (int b = 0; b < B; b++) {
        const int32_t* o = &orders[(size_t)b * (n + 1)];
        std::vector<int> seen((size_t)n + 1, 0);
        bool ok = o[0] == 0 && o[1] == 1 && nev[(size_t)b] >= 1 && nev[(size_t)b] < n;
        for (int i = 1; i <= n && ok; i++) ok = o[i] >= 1 && o[i] <= n && !seen[(size_t)o[i]]++;
        if (!ok) { std::fprintf(stderr, "%s: n=%d problem %d: not a circular order\n", what, n, b); return 1; }
    }
    return 0;
}

// The same problems through a caller's layout (row stride ld, problem stride `stride`) in a heap block of EXACTLY the size the
// contract asks for - (B - 1) * stride + (n - 1) * ld + n doubles, padding NaN: a read past the last problem's last element is an
// error here.  The orders must be those of the dense run.
static int run_layout(const std::vector<double>& D, int n, int B, int64_t ld, int64_t stride, const std::vector<int32_t>& dense_orders) {
    const size_t need = (size_t)((B - 1) * stride + (int64_t)(n - 1) * ld + n);
    double* buf = (double*)std::malloc(sizeof(double) * need);
    if (!buf) return 1;
    for (size_t k = 0; k < need; k++) buf[k] = std::nan("");
    for (int b = 0; b < B; b++)
        for (int r = 0; r < n; r++)
            for (int c = 0; c < n; c++) buf[(size_t)(b * stride + r * ld + c)] = D[((size_t)b * n + r) * n + c];
    std::vector<int32_t> orders((size_t)B * (n + 1), -7);
    fnn_opts opts{};
    opts.validate = 1;
    int32_t rc = emu_canonical_order_batch_f64(buf, n, ld, stride, B, &opts, orders.data(), nullptr, nullptr, nullptr);
    // the in-place entry, twice on the same block: it must not write to it (the bytes are compared: the padding is NaN)
    std::vector<unsigned char> before((const unsigned char*)buf, (const unsigned char*)buf + sizeof(double) * need);
    for (int k = 0; k < 2 && rc == FNN_OK; k++) {
        std::vector<int32_t> again((size_t)B * (n + 1), -7);
        rc = emu_canonical_order_batch_device_f64(buf, n, ld, stride, B, &opts, again.data(), nullptr, nullptr, nullptr);
        if (rc == FNN_OK && (again != orders || std::memcmp(before.data(), buf, before.size()) != 0)) {
            std::fprintf(stderr, "layout ld=%d stride=%d: n=%d: in-place run %d wrote to the caller's block or gave other orders\n", (int)ld, (int)stride, n, k);
            std::free(buf);
            return 1;
        }
    }
    std::free(buf);
    if (rc != FNN_OK) { std::fprintf(stderr, "layout ld=%d stride=%d: n=%d: status %d (%s)\n", (int)ld, (int)stride, n, rc, emu_last_error()); return 1; }
    if (orders != dense_orders) { std::fprintf(stderr, "layout ld=%d stride=%d: n=%d: orders differ from the dense run\n", (int)ld, (int)stride, n); return 1; }
    return 0;
}

static int run_case(const std::vector<double>& D, int n, int B, const int32_t* expect, const char* what) {
    std::vector<int32_t> orders((size_t)B * (n + 1), -7), nev((size_t)B, -7);
    std::vector<fnn_event> ev((size_t)B * n);
    fnn_opts opts{};
    opts.validate = 1;
    fnn_batch_stats st{};
    const int32_t rc = emu_canonical_order_batch_f64(D.data(), n, n, (int64_t)n * n, B, &opts, orders.data(), ev.data(), nev.data(), &st);
    if (rc != FNN_OK) { std::fprintf(stderr, "%s: n=%d: status %d (%s)\n", what, n, rc, emu_last_error()); return 1; }
    if (st.n_global != B || st.n_lds != 0 || st.n_fallback != 0 || st.lds_bytes > 163840) { std::fprintf(stderr, "%s: n=%d: wrong route\n", what, n); return 1; }
    if (check_orders(orders, nev, n, B, what)) return 1;
    // caller layouts on exact-size buffers: a padded row stride with problems five doubles apart; up to 65 taxa also
    // problems one double apart and a padded row stride alone
    if (run_layout(D, n, B, n + 1, (int64_t)n * (n + 1) + 5, orders)) return 1;
    if (n <= 65 && (run_layout(D, n, B, n, (int64_t)n * n + 1, orders) || run_layout(D, n, B, n + 3, (int64_t)n * (n + 3), orders))) return 1;
    if (expect)
        for (size_t k = 0; k < orders.size(); k++)
            if (orders[k] != expect[k]) { std::fprintf(stderr, "%s: n=%d problem %d: order differs from the recorded one\n", what, n, (int)(k / (n + 1))); return 1; }
    return 0;
}

int main(int argc, char** argv) {
    setenv("FNN_BATCH_ROUTE", "global", 1);
    const int nmax = emu_batch_lds_max_n();
    if (emu_batch_global_max_n() <= nmax) { std::fprintf(stderr, "global_max_n = %d <= lds_max_n\n", emu_batch_global_max_n()); return 1; }
    const int sizes[] = {4, 5, 6, 7, 8, 9, 16, 33, 63, 64, 65, nmax + 1, 257};
    int cases = 0;
    for (int n : sizes) {
        const int ncls = 5;
        std::vector<double> all, one;
        for (int cls = 0; cls < ncls; cls++) {
            generate(one, n, cls, 1000 + (uint64_t)n * 8 + (uint64_t)cls);
            all.insert(all.end(), one.begin(), one.end());
        }
        if (run_case(all, n, ncls, nullptr, "generated")) return 1;
        cases += ncls;
    }
    if (argc > 1) {
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
        int32_t ncases = 0;
        if (std::fread(&ncases, 4, 1, f) != 1) { std::fclose(f); return 1; }
        for (int k = 0; k < ncases; k++) {
            int32_t hdr[2];
            if (std::fread(hdr, 4, 2, f) != 2 || hdr[0] < 1 || hdr[1] < 1) { std::fclose(f); std::fprintf(stderr, "bad case file\n"); return 1; }
            const int n = hdr[0], B = hdr[1];
            std::vector<double> D((size_t)B * n * n);
            std::vector<int32_t> expect((size_t)B * (n + 1));
            if (std::fread(D.data(), 8, D.size(), f) != D.size() || std::fread(expect.data(), 4, expect.size(), f) != expect.size()) {
                std::fclose(f); std::fprintf(stderr, "short case file\n"); return 1;
            }
            if (run_case(D, n, B, expect.data(), "recorded")) { std::fclose(f); return 1; }
            cases += B;
        }
        std::fclose(f);
    }
    std::printf("ok: %d problems\n", cases);
    return 0;
}

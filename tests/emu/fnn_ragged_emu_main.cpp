// fnn_ragged_emu_main.cpp -- TEST INFRASTRUCTURE: stand-alone program over the CPU driver of the ragged batch calls
// (fnn_ragged_emu.cpp), meant to be built with -fsanitize=address,undefined: an index past a problem's LDS layout, its
// workspace slice or its slice of a concatenated output is silent on the GPU, here it ends the program.
//
//   fnn_ragged_emu_main FILE      int32 B, then per problem int32 n, n*n doubles, n+1 int32 (the expected order).  Every matrix
//                                 goes into a heap block of its own of EXACTLY the size the contract asks for - (n - 1) * ld + n
//                                 doubles, every third with ld = n + 3, padding NaN -, so a read past a problem's last
//                                 element is an error here; one block starts one double late, so that its problem lies at an
//                                 odd offset.  All problems run in ONE call per entry (host, in place), once in one chunk and
//                                 once three problems per chunk; the orders must be the recorded ones.  Then the weights of
//                                 those orders for the problems of two taxa and more, through both entries: certified,
//                                 finite, non-negative, the same bits from both.
// Exit status 0: all well.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/fastnn.h"

extern "C" {
const char* emu_last_error(void);
int32_t emu_canonical_order_ragged_f64(const double* D, const int64_t* offsets, const int32_t* n, const int64_t* ld, int64_t batch, const fnn_opts* opts,
                                       int32_t* orders_out, fnn_event* events_out, int32_t* nevents_out, fnn_batch_stats* stats);
int32_t emu_canonical_order_ragged_device_f64(const double* D, const int64_t* offsets, const int32_t* n, const int64_t* ld, int64_t batch,
                                              const fnn_opts* opts, int32_t* orders_out, fnn_event* events_out, int32_t* nevents_out,
                                              fnn_batch_stats* stats);
int32_t emu_split_weights_ragged_f64(const double* D, const int64_t* offsets, const int32_t* n, const int64_t* ld, int64_t batch, const int32_t* orderings,
                                     int32_t device, double* weights_out, fnn_sw_stats* stats_out, fnn_sw_batch_stats* stats);
int32_t emu_split_weights_ragged_device_f64(const double* D, const int64_t* offsets, const int32_t* n, const int64_t* ld, int64_t batch,
                                            const int32_t* orderings, int32_t device, double* weights_out, fnn_sw_stats* stats_out,
                                            fnn_sw_batch_stats* stats);
}

struct Problems {
    std::vector<double*> blocks;  // what to free
    std::vector<const double*> at;
    std::vector<int32_t> n;
    std::vector<int64_t> ld, off;
    std::vector<int32_t> expect;  // concatenated
    ~Problems() { for (double* p : blocks) std::free(p); }
};

static int run_orders(const Problems& P, const double* base, bool in_place, const char* what) {
    const int64_t B = (int64_t)P.n.size();
    int64_t ne = 0;
    for (int32_t n : P.n) ne += n;
    std::vector<int32_t> orders(P.expect.size(), -7), nev((size_t)B, -7);
    std::vector<fnn_event> ev((size_t)ne + 1);
    fnn_opts opts{};
    opts.validate = 1;
    fnn_batch_stats st{};
    const int32_t rc = (in_place ? emu_canonical_order_ragged_device_f64 : emu_canonical_order_ragged_f64)(
        base, P.off.data(), P.n.data(), P.ld.data(), B, &opts, orders.data(), ev.data(), nev.data(), &st);
    if (rc != FNN_OK) { std::fprintf(stderr, "%s: status %d (%s)\n", what, rc, emu_last_error()); return 1; }
    if (orders != P.expect) { std::fprintf(stderr, "%s: the orders differ from the recorded ones\n", what); return 1; }
    for (int64_t b = 0; b < B; b++)
        if (nev[(size_t)b] < 0 || nev[(size_t)b] >= (P.n[(size_t)b] > 0 ? P.n[(size_t)b] : 1)) { std::fprintf(stderr, "%s: problem %d: event count\n", what, (int)b); return 1; }
    if (st.n_fallback != 0 || st.chunks < 1 || st.chunks > 64) { std::fprintf(stderr, "%s: wrong route\n", what); return 1; }
    return 0;
}

static int run_weights(const Problems& P, const double* base) {
    std::vector<int32_t> n, ords;
    std::vector<int64_t> ld, off;
    size_t o = 0, nw = 0;
    for (size_t b = 0; b < P.n.size(); o += (size_t)P.n[b] + 1, b++) {
        if (P.n[b] < 2) continue;
        n.push_back(P.n[b]); ld.push_back(P.ld[b]); off.push_back(P.off[b]);
        ords.insert(ords.end(), P.expect.begin() + (long)o, P.expect.begin() + (long)(o + (size_t)P.n[b] + 1));
        nw += (size_t)P.n[b] * (size_t)(P.n[b] - 1) / 2;
    }
    const int64_t B = (int64_t)n.size();
    std::vector<double> w[2];
    for (int in_place = 0; in_place < 2; in_place++) {
        w[in_place].assign(nw, -7.0);
        std::vector<fnn_sw_stats> sw((size_t)B);
        fnn_sw_batch_stats st{};
        const int32_t rc = (in_place ? emu_split_weights_ragged_device_f64 : emu_split_weights_ragged_f64)(
            base, off.data(), n.data(), ld.data(), B, ords.data(), 0, w[in_place].data(), sw.data(), &st);
        if (rc != FNN_OK) { std::fprintf(stderr, "weights (%d): status %d (%s)\n", in_place, rc, emu_last_error()); return 1; }
        if (st.n_fallback != 0 || st.n_kernel + st.n_closed_form != B) { std::fprintf(stderr, "weights (%d): wrong route\n", in_place); return 1; }
        for (int64_t b = 0; b < B; b++)
            if (!sw[(size_t)b].certified || !(sw[(size_t)b].kkt_violation <= 1e-9)) { std::fprintf(stderr, "weights (%d): problem %d is not certified\n", in_place, (int)b); return 1; }
        for (double v : w[in_place])
            if (!(v >= 0.0) || !std::isfinite(v)) { std::fprintf(stderr, "weights (%d): a weight is negative or not finite\n", in_place); return 1; }
    }
    if (w[0] != w[1]) { std::fprintf(stderr, "weights: the two entries differ\n"); return 1; }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s FILE\n", argv[0]); return 1; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
    Problems P;
    int32_t B = 0;
    if (std::fread(&B, 4, 1, f) != 1 || B < 1) { std::fclose(f); std::fprintf(stderr, "bad case file\n"); return 1; }
    bool shifted = false;
    for (int b = 0; b < B; b++) {
        int32_t n = 0;
        if (std::fread(&n, 4, 1, f) != 1 || n < 0) { std::fclose(f); std::fprintf(stderr, "bad case file\n"); return 1; }
        std::vector<double> D((size_t)n * n);
        std::vector<int32_t> o((size_t)n + 1);
        if (std::fread(D.data(), 8, D.size(), f) != D.size() || std::fread(o.data(), 4, o.size(), f) != o.size()) {
            std::fclose(f); std::fprintf(stderr, "short case file\n"); return 1;
        }
        const int64_t ld = b % 3 == 1 ? n + 3 : n;
        const bool shift = !shifted && ld == n && n >= 8;  // this problem one double into its block: an odd offset
        shifted = shifted || shift;
        const size_t need = (n > 0 ? (size_t)((int64_t)(n - 1) * ld + n) : 1) + (shift ? 1 : 0);
        double* blk = (double*)std::malloc(sizeof(double) * need);
        if (!blk) { std::fclose(f); return 1; }
        for (size_t k = 0; k < need; k++) blk[k] = std::nan("");
        double* at = blk + (shift ? 1 : 0);
        for (int r = 0; r < n; r++)
            for (int c = 0; c < n; c++) at[(int64_t)r * ld + c] = D[(size_t)r * n + c];
        P.blocks.push_back(blk);
        P.at.push_back(at);
        P.n.push_back(n);
        P.ld.push_back(ld);
        P.expect.insert(P.expect.end(), o.begin(), o.end());
    }
    std::fclose(f);
    uintptr_t lo = UINTPTR_MAX;
    for (const double* p : P.at) lo = reinterpret_cast<uintptr_t>(p) < lo ? reinterpret_cast<uintptr_t>(p) : lo;
    for (const double* p : P.at) P.off.push_back((int64_t)((reinterpret_cast<uintptr_t>(p) - lo) / sizeof(double)));
    const double* base = reinterpret_cast<const double*>(lo);
    if (setenv("FNN_SW_BATCH_ROUTE", "kernel", 1)) return 1;
    if (run_orders(P, base, false, "host entry") || run_orders(P, base, true, "in-place entry") || run_weights(P, base)) return 1;
    if (setenv("FNN_BATCH_CHUNK", "3", 1)) return 1;
    if (run_orders(P, base, false, "host entry, chunked") || run_orders(P, base, true, "in-place entry, chunked") || run_weights(P, base)) return 1;
    std::printf("ok: %d problems\n", (int)B);
    return 0;
}

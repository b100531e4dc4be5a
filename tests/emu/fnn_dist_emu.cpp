// fnn_dist_emu.cpp -- TEST INFRASTRUCTURE: CPU driver of the alignment-distance path.
//
// Runs the per-lane steps of fastneighbornet_amd/csrc/fnn_dist.h for lane = 0 ... 63 of every wave of k_dist's grid, with the
// tile product as loops written from the stated lane maps (dist_tile_product), under the same host logic as the product
// (dist_batch<B>): argument checks, padding, digit planes, chunking, collection, error naming.  "Device memory" is the
// heap: every buffer has exactly the size the host logic asks for and is filled with 0xFF bytes first
// (fnn_small_emu.h), so under AddressSanitizer a 16-byte load that leaves its buffer is an error.
//
// Build: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off (tests/dist_common.py).  Same signatures as include/fastnn.h
// with the prefix emu_.
#include "../../fastneighbornet_amd/csrc/fnn_dist.h"
#include "fnn_small_emu.h"

namespace {

using namespace fnn;

template <int P, bool MISSING>
void emu_wave(const DistArgs& a, const DistTile& t, int64_t b0) {
    DistAcc am[DIST_RT][P][64], av[DIST_RT][P][64];
    std::memset(am, 0, sizeof(am));
    std::memset(av, 0, sizeof(av));
    DistFrag fm[64], fv[64], fb[64];
    std::memset(fv, 0xFF, sizeof(fv));
    for (int64_t s = 0; s < a.lpad; s += DIST_K) {
        for (int lane = 0; lane < 64; lane++) dist_lane_a<MISSING>(a, t, lane, s, fm[lane], fv[lane]);
        for (int rt = 0; rt < DIST_RT; rt++)
            for (int d = 0; d < P; d++) {
                for (int lane = 0; lane < 64; lane++) fb[lane] = dist_lane_b(a, b0, rt, d, lane, s);
                dist_tile_product(fm, fb, am[rt][d]);
                if (MISSING) dist_tile_product(fv, fb, av[rt][d]);
            }
    }
    for (int rt = 0; rt < DIST_RT; rt++)
        for (int lane = 0; lane < 64; lane++) {
            DistAcc m[P], v[P];
            for (int d = 0; d < P; d++) { m[d] = am[rt][d][lane]; v[d] = av[rt][d][lane]; }
            dist_lane_store<P, MISSING>(a, t, b0 + DIST_TILE * rt, lane, m, v);
        }
}

struct EmuDistBackend : EmuHeapBackend {
    template <int P, bool MISSING>
    void grid(const DistArgs& a, int64_t tile_groups, int64_t rep_groups) {
        for (int64_t blk = 0; blk < tile_groups * rep_groups; blk++) {
            const int64_t rg = blk / tile_groups, tg = blk - rg * tile_groups;
            for (int wave = 0; wave < DIST_WAVES; wave++) emu_wave<P, MISSING>(a, a.tiles[tg * DIST_WAVES + wave], rg * DIST_REPS);
        }
    }
    int32_t run(int32_t P, bool missing, const DistArgs& a, int64_t tile_groups, int64_t rep_groups, double* t_kernel_s) {
        const double t0 = now_s();
        switch (P * 2 + (missing ? 1 : 0)) {
            case 2: grid<1, false>(a, tile_groups, rep_groups); break;
            case 3: grid<1, true>(a, tile_groups, rep_groups); break;
            case 4: grid<2, false>(a, tile_groups, rep_groups); break;
            case 5: grid<2, true>(a, tile_groups, rep_groups); break;
            case 6: grid<3, false>(a, tile_groups, rep_groups); break;
            case 7: grid<3, true>(a, tile_groups, rep_groups); break;
            default: last = "no kernel for " + std::to_string(P) + " digits"; return FNN_EHIP;
        }
        *t_kernel_s = now_s() - t0;
        return FNN_OK;
    }
};

}  // namespace

extern "C" {

const char* emu_last_error(void) { return fnn::g_last_error.c_str(); }

int32_t emu_alignment_distances_batch_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch, int64_t ldc,
                                          int32_t model, int32_t device, double* D_out, int64_t ld, int64_t stride, fnn_dist_stats* stats) {
    try {
        EmuDistBackend be;
        return fnn::dist_batch(be, "emu_alignment_distances_batch_f64", seq, n, L, lds, counts, batch, ldc, model, device, D_out, false, ld, stride, stats);
    } catch (const std::exception& e) {
        return fnn::fail(FNN_ESTATE, std::string("exception: ") + e.what());
    }
}

// (the "device" pointer is host memory here: the matrices are written in place, through ld and stride)
int32_t emu_alignment_distances_batch_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch,
                                                 int64_t ldc, int32_t model, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                 fnn_dist_stats* stats) {
    try {
        EmuDistBackend be;
        return fnn::dist_batch(be, "emu_alignment_distances_batch_device_f64", seq, n, L, lds, counts, batch, ldc, model, device, D_out, true, ld, stride, stats);
    } catch (const std::exception& e) {
        return fnn::fail(FNN_ESTATE, std::string("exception: ") + e.what());
    }
}

int32_t emu_bootstrap_counts(int64_t L, int64_t batch, uint64_t seed, uint16_t* counts_out) {
    try {
        return fnn::dist_bootstrap_counts("emu_bootstrap_counts", L, batch, seed, counts_out);
    } catch (const std::exception& e) {
        return fnn::fail(FNN_ESTATE, std::string("exception: ") + e.what());
    }
}

}  // extern "C"

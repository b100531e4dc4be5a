// fnn_dist_gamma_emu.cpp -- TEST INFRASTRUCTURE: CPU driver of the alignment-distance path with gamma-distributed rates
// (DESIGN.md section 19).
//
// The gamma correction is a field of DistModel / DistPairs that the epilogues of fnn_dist.h and fnn_dist_pairs.h read, and the
// host template dist_batch_source<B> fills it from a fnn_dist_model_rates: the backend of fnn_dist_pairs_emu.cpp - the
// per-lane steps for lane = 0 ... 63 of every wave of the kernels' grids, k_draw's among them, on heap blocks of exactly the
// sizes the host logic asks for - runs it as it stands.  This file adds the entries with the prefix emug_ (so that one library
// holds what tests/dist_gamma_common.py binds) and emug_dist_expm1.
//
// Build: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off (tests/dist_gamma_common.py).
#include "fnn_dist_pairs_emu.cpp"  // EmuDistPairsBackend, emup_try

extern "C" {

const char* emug_last_error(void) { return fnn::g_last_error.c_str(); }

double emug_dist_expm1(double x) { return fnn::dist_expm1(x); }

int32_t emug_alignment_distances_model_batch_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch, int64_t ldc,
                                                 const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                 fnn_dist_model_stats* stats) {
    return emup_try([&] {
        EmuDistPairsBackend be;
        return fnn::dist_batch_model(be, "emug_alignment_distances_model_batch_f64", seq, n, L, lds, counts, batch, ldc, m, device, D_out, false, ld, stride,
                                     stats);
    });
}

// (the "device" pointers are host memory here: the output is written in place, through ld and stride)
int32_t emug_alignment_distances_model_batch_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts, int64_t batch,
                                                        int64_t ldc, const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                        fnn_dist_model_stats* stats) {
    return emup_try([&] {
        EmuDistPairsBackend be;
        return fnn::dist_batch_model(be, "emug_alignment_distances_model_batch_device_f64", seq, n, L, lds, counts, batch, ldc, m, device, D_out, true, ld,
                                     stride, stats);
    });
}

int32_t emug_bootstrap_draw_max_sites(void) { return fnn::DRAW_MAX_SITES; }

int32_t emug_bootstrap_distances_batch_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, int64_t batch, uint64_t seed, int64_t lead,
                                           const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride, fnn_boot_stats* stats) {
    return emup_try([&] {
        EmuDistPairsBackend be;
        return fnn::dist_bootstrap_batch(be, "emug_bootstrap_distances_batch_f64", seq, n, L, lds, batch, seed, lead, m, device, D_out, false, ld, stride,
                                         stats);
    });
}

int32_t emug_bootstrap_distances_batch_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, int64_t batch, uint64_t seed, int64_t lead,
                                                  const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                  fnn_boot_stats* stats) {
    return emup_try([&] {
        EmuDistPairsBackend be;
        return fnn::dist_bootstrap_batch(be, "emug_bootstrap_distances_batch_device_f64", seq, n, L, lds, batch, seed, lead, m, device, D_out, true, ld,
                                         stride, stats);
    });
}

}  // extern "C"

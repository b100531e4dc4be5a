// fnn_splits_plan.h -- the host arithmetic of the circular split-weight solver's block method (fnn_splits.hip) that touches
// no device: the switches of a call, the capacity plan of the factor, the host part of Lawson & Hanson's ratio step, the
// compaction and revival lists and the objective.  Plain C++ on host vectors - no HIP, no rocBLAS - so that
// tests/emu/fnn_splits_plan_main.cpp runs the very lines the solver runs, on the CPU and under the sanitizers.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace fnnsw {

// ---------------------------------------------------------------- the FNN_SW_* switches, read once per call
struct Knobs {
    bool log = false;                // FNN_SW_LOG: the method's progress and phase times on stderr
    double kfrac = 0.20;             // FNN_SW_KFRAC: a block is this share of the splits that are in
    double rfrac = 0.15;             // FNN_SW_RFRAC: the share of departed splits in the factor at which it is rebuilt
    int nms = 3;                     // FNN_SW_NMS: radius of the candidates' local-maximum test
    int revive = 2;                  // FNN_SW_REVIVE: 0 = departed splits only come back through a rebuild (round 3), 1 = at the start of
                                     // every step, 2 = only when no candidate is left (the case that used to force a rebuild "to look again")
    int64_t panel = 0;               // FNN_SW_PANEL: panel width of the factor's storage (>= 64; else the plan's own)
    double cap = 0.0;                // FNN_SW_CAP: the factor's capacity as a multiple of n (> 0; else the plan's own) ...
    bool cap_set = false;            // ... and its mere presence pins the capacity: no retry with a larger factor
    bool reference_method = false;   // FNN_SW_REFERENCE_METHOD: the reference's active-set / conjugate-gradient method from the start
    int64_t reference_max_n = 1024;  // FNN_SW_REFERENCE_MAX_N: up to this size the reference's route follows a give-up by itself
    bool allow_reference = false;    // FNN_SW_ALLOW_REFERENCE_ROUTE: ... and with this at every size
    bool no_reference = false;       // FNN_SW_NO_REFERENCE_ROUTE: ... and with this never
    bool fault_perturb = false;      // FNN_SW_FAULT_PERTURB: test hook (k_fault_perturb)

    static Knobs from_env() {
        auto envd = [](const char* k, double dflt) { const char* e = std::getenv(k); return e ? std::atof(e) : dflt; };
        auto set = [](const char* k) { return std::getenv(k) != nullptr; };
        Knobs kn;
        kn.log = set("FNN_SW_LOG");
        kn.kfrac = envd("FNN_SW_KFRAC", 0.20);
        kn.rfrac = envd("FNN_SW_RFRAC", 0.15);
        kn.nms = (int)envd("FNN_SW_NMS", 3);
        kn.revive = (int)envd("FNN_SW_REVIVE", 2.0);
        if (const char* e = std::getenv("FNN_SW_PANEL")) kn.panel = std::atoll(e);
        kn.cap = envd("FNN_SW_CAP", 0.0);
        kn.cap_set = set("FNN_SW_CAP");
        kn.reference_method = set("FNN_SW_REFERENCE_METHOD");
        if (const char* e = std::getenv("FNN_SW_REFERENCE_MAX_N")) kn.reference_max_n = std::atoll(e);
        kn.allow_reference = set("FNN_SW_ALLOW_REFERENCE_ROUTE");
        kn.no_reference = set("FNN_SW_NO_REFERENCE_ROUTE");
        kn.fault_perturb = set("FNN_SW_FAULT_PERTURB");
        return kn;
    }
};

// ---------------------------------------------------------------- the capacity plan
inline int64_t up64(int64_t v) { return (v + 63) / 64 * 64; }
// doubles of a lower-triangular factor of `cap` columns stored as column panels of width pw (TriStore in fnn_splits.hip)
inline int64_t tri_elems(int64_t cap, int64_t pw) {
    int64_t tot = 0;
    for (int64_t q0 = 0; q0 < cap; q0 += pw) tot += std::min(pw, cap - q0) * (cap - q0);
    return tot;
}
// {capacity / n, block = capacity / kdiv, departed columns = capacity / rdiv}
struct FactorShape { double f; int kdiv, rdiv; };
struct CapacityPlan {
    int64_t cap = 0, kmax = 0, rcap = 0, pw = 0;  // the factor's capacity, the largest block, room for departed columns, panel width
    FactorShape pick{0.0, 0, 0};
    double bytes = 0.0;    // what the buffers of that shape take (an estimate: some small vectors are not counted, the budget's 0.92 absorbs them)
    bool fits = false;     // bytes <= budget.  A first attempt that does not fit still gets the last shape (the allocation then fails)
    int64_t cap_want = 0;  // the retry's wanted capacity after the plan shrank it to what fits
};
// Capacity of the factor (splits that are in + the departed ones still inside + the entering block): random distances end
// with ~2.4 n positive splits, tree-like ones with more (tree + 5 % noise: 3.8 n) - as many as device memory allows, up
// to 6 n: the factor takes cap^2 doubles, the block buffers, the departed columns and their Gram matrices 0.61 cap^2 more.
// cap_want > 0: the factor's capacity for this attempt (a retry after FNN_SW_GIVEUP_CAPACITY), else the default for n.
inline CapacityPlan plan_capacity(int n, double budget, int64_t cap_want, const Knobs& kn) {
    const int64_t N = (int64_t)n * (n - 1) / 2;
    CapacityPlan b;
    auto sized = [&](double factor, int kdiv, int rdiv) {
        b.cap = up64(std::min<int64_t>(N, std::max<int64_t>({(int64_t)(factor * n) + 1024, std::min<int64_t>(8 * (int64_t)n + 64, 20000), 512})));
        if (cap_want > 0) b.cap = up64(std::min<int64_t>(N, cap_want));
        b.kmax = std::min<int64_t>({b.cap, std::max<int64_t>(64, up64(b.cap / kdiv)), (int64_t)8192});  // (a block costs 4 k^2 f beside its 4 k f^2: keep k / f small)
        b.rcap = std::min<int64_t>(b.cap, up64(b.cap / rdiv) + 64);
        b.pw = std::max<int64_t>(1024, up64(b.cap / 8));
        if (kn.panel >= 64) b.pw = up64(kn.panel);
        return 8.0 * ((double)tri_elems(b.cap, b.pw) + 3.0 * (double)b.cap * b.kmax + (double)b.cap * b.rcap + 4.0 * (double)b.rcap * b.rcap + 3.0 * (double)b.kmax * b.kmax +
                      0.5 * (double)std::max(b.rcap, b.kmax) * std::max(b.rcap, b.kmax)) + 64.0 * (double)b.cap + 48.0 * (double)std::max<int64_t>(1 << 16, N / 16 + 1024);
    };
    // the roomy shapes first; where memory is short (32768 taxa) a shape with smaller side buffers buys capacity (4 n instead of 3.5 n)
    const FactorShape shapes[] = {{6.0, 12, 5}, {5.0, 12, 5}, {4.5, 12, 5}, {4.0, 12, 5}, {4.0, 16, 8}, {3.5, 12, 5}, {3.25, 12, 5}};
    b.pick = shapes[6];
    if (cap_want > 0) {
        // a retry with a larger factor: the wanted capacity with the roomiest side buffers that fit, else as much as fits
        const FactorShape tries[] = {{0.0, 12, 5}, {0.0, 16, 8}, {0.0, 24, 12}};
        for (int round = 0; round < 40 && !b.fits; round++) {
            for (const FactorShape& sh : tries) { b.pick = sh; if ((b.bytes = sized(0.0, sh.kdiv, sh.rdiv)) <= budget) { b.fits = true; break; } }
            if (!b.fits) cap_want = (int64_t)(0.9 * (double)cap_want);
        }
        b.cap_want = cap_want;
        if (!b.fits) return b;
    } else {
        for (const FactorShape& sh : shapes) {
            b.pick = sh;
            if (kn.cap > 0.0) { b.pick.f = kn.cap; break; }
            if (sized(sh.f, sh.kdiv, sh.rdiv) <= budget) break;
        }
    }
    b.bytes = sized(b.pick.f, b.pick.kdiv, b.pick.rdiv);
    b.fits = b.bytes <= budget;
    return b;
}

// ---------------------------------------------------------------- Lawson & Hanson's ratio step, host part
// From the point xcur towards the sub-problem's minimiser s as far as feasibility allows: alpha is the smallest x / (x - s)
// over the members whose s is not positive (2 if there is none; `!(s > 0)` takes a NaN as not positive, and std::min(alpha, q)
// keeps alpha when q is NaN).  alpha > 1: the minimiser is feasible, nothing changes.  Else xcur moves by alpha, and the
// members that reach zero - `!(q > alpha)`: 0 / 0 counts as a hit - or do not stay positive are listed in `out`: they leave.
inline double ratio_step(std::vector<double>& xcur, const std::vector<double>& s, const std::vector<uint8_t>& dead, std::vector<int32_t>& out) {
    out.clear();
    double alpha = 2.0;
    for (size_t p = 0; p < s.size(); p++)
        if (!dead[p] && !(s[p] > 0.0)) alpha = std::min(alpha, xcur[p] / (xcur[p] - s[p]));
    if (alpha > 1.0) return alpha;
    for (size_t p = 0; p < s.size(); p++) {
        if (dead[p]) continue;
        const bool neg = !(s[p] > 0.0);
        const bool hit = neg && !(xcur[p] / (xcur[p] - s[p]) > alpha);  // (0 / 0 counts as a hit)
        xcur[p] = hit ? 0.0 : xcur[p] + alpha * (s[p] - xcur[p]);
        if (hit || (neg && !(xcur[p] > 0.0))) out.push_back((int32_t)p);
    }
    return alpha;
}

// ---------------------------------------------------------------- compaction and revival lists
// A rebuild keeps the splits that are still in, in order: F, xw, cF close ranks, `gone` receives the splits that had left
template <class Split>
inline void compact_live(std::vector<Split>& F, std::vector<double>& xw, std::vector<double>& cF, std::vector<uint8_t>& dead, std::vector<int32_t>& deadlist,
                         std::vector<Split>& gone) {
    gone.clear();
    size_t q = 0;
    for (size_t p = 0; p < F.size(); p++) {
        if (dead[p]) { gone.push_back(F[p]); continue; }
        F[q] = F[p]; xw[q] = xw[p]; cF[q] = cF[p]; q++;
    }
    F.resize(q); xw.resize(q); cF.resize(q); dead.assign(q, 0); deadlist.clear();
}
// The departed splits at the factor positions `rev` come back (dead is cleared there): keepcols = the columns of Y (indices into
// deadlist) that stay, newdead = their factor positions, both in the order of Y's columns
inline void revival_lists(const std::vector<int32_t>& rev, int64_t f, std::vector<uint8_t>& dead, const std::vector<int32_t>& deadlist,
                          std::vector<int32_t>& keepcols, std::vector<int32_t>& newdead) {
    keepcols.clear(); newdead.clear();
    std::vector<uint8_t> back((size_t)f, 0);
    for (int32_t p : rev) { back[(size_t)p] = 1; dead[(size_t)p] = 0; }
    for (int64_t q = 0; q < (int64_t)deadlist.size(); q++)
        if (!back[(size_t)deadlist[(size_t)q]]) { keepcols.push_back((int32_t)q); newdead.push_back(deadlist[(size_t)q]); }
}

// objective - c_F . x_F / 2 of a sub-problem's exact minimiser xs
inline double objective(const std::vector<double>& xs, const std::vector<double>& cF, const std::vector<uint8_t>& dead) {
    double acc = 0.0;
    for (size_t p = 0; p < xs.size(); p++) if (!dead[p]) acc += cF[p] * xs[p];
    return -0.5 * acc;
}

}  // namespace fnnsw

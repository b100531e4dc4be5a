// fnn_splits_phase_main.cpp -- TEST INFRASTRUCTURE: stand-alone program over the phase-level entries of the CPU driver of
// the batched circular split weights (fnn_splits_batch_emu.cpp: emu_splits_ratio_pass, emu_splits_append_row).  It holds no
// expectation of its own: it reads crafted states from standard input, runs the product's phase bodies on them and prints
// the states they leave; tests/test_splits_phases.py crafts the states and compares with its own restatement of the rules.
// With a main of its own it can be built with -fsanitize=address,undefined and run directly.
//
// Input, one case per line, numbers separated by blanks (doubles as strtod reads them: hexadecimal floats, "nan"):
//   ratio  n threads f enter_pos departed n_aside steps max_steps  Fi[f] xF[f] sF[f] cF[f]
//   append n threads r ftot fresh dep hkk ll lz enter_pos departed n_aside entered peak  Fi[ftot] xF[ftot] cF[ftot] rv[r]
// Every grid entry of gx starts at 1 + its index and every mask byte at 1 for the members of F, 0 elsewhere.
// Output, one line per case: the control words, then the vectors, then "gx"/"mask" with the entries of the case's members.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

extern "C" {
int32_t emu_splits_ratio_pass(int32_t n, int32_t threads, int32_t f, const int32_t* ctl_in, int32_t* ctl_out, double* alpha_out, int32_t* Fi, double* xF,
                              const double* sF, double* cF, double* gx, uint8_t* mask);
int32_t emu_splits_append_row(int32_t n, int32_t threads, int32_t r, int32_t ftot, int32_t fresh, double dep, double hkk, double ll, double lz,
                              const double* rv, const int32_t* ctl_in, int32_t* ctl_out, int32_t* Fi, double* xF, double* cF, double* gx, uint8_t* mask,
                              double* w_row, double* z_r);
}

static bool read_i(std::istringstream& in, int32_t& v) { long long x; if (!(in >> x)) return false; v = (int32_t)x; return true; }
static bool read_d(std::istringstream& in, double& v) { std::string t; if (!(in >> t)) return false; char* e = nullptr; v = std::strtod(t.c_str(), &e); return e && !*e; }
static bool read_iv(std::istringstream& in, std::vector<int32_t>& v, int k) { v.resize((size_t)k); for (auto& x : v) if (!read_i(in, x)) return false; return true; }
static bool read_dv(std::istringstream& in, std::vector<double>& v, int k) { v.resize((size_t)k); for (auto& x : v) if (!read_d(in, x)) return false; return true; }

static void grids(int n, const std::vector<int32_t>& Fi, std::vector<double>& gx, std::vector<uint8_t>& mask) {
    gx.resize((size_t)n * n); mask.assign((size_t)n * n, 0);
    for (size_t e = 0; e < gx.size(); e++) gx[e] = 1.0 + (double)e;
    for (int32_t k : Fi) mask[(size_t)k] = 1;
}
static void print_state(const std::vector<int32_t>& members, int cnt, const int32_t* Fi, const double* xF, const double* cF,
                        const std::vector<double>& gx, const std::vector<uint8_t>& mask) {
    std::printf(" Fi"); for (int j = 0; j < cnt; j++) std::printf(" %d", Fi[j]);
    std::printf(" xF"); for (int j = 0; j < cnt; j++) std::printf(" %a", xF[j]);
    std::printf(" cF"); for (int j = 0; j < cnt; j++) std::printf(" %a", cF[j]);
    std::printf(" gx"); for (int32_t k : members) std::printf(" %a", gx[(size_t)k]);
    std::printf(" mask"); for (int32_t k : members) std::printf(" %d", (int)mask[(size_t)k]);
    std::printf("\n");
}

int main() {
    std::string line;
    int cases = 0;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string kind;
        in >> kind;
        std::vector<int32_t> Fi;
        std::vector<double> xF, sF, cF, rv, gx;
        std::vector<uint8_t> mask;
        bool ok = true;
        if (kind == "ratio") {
            int32_t n, threads, f, ci[5], co[9];
            ok = read_i(in, n) && read_i(in, threads) && read_i(in, f);
            for (int k = 0; k < 5 && ok; k++) ok = read_i(in, ci[k]);
            ok = ok && f >= 0 && f < 4096 && read_iv(in, Fi, f) && read_dv(in, xF, f) && read_dv(in, sF, f) && read_dv(in, cF, f);
            if (ok) for (int32_t k : Fi) ok = ok && k >= 0 && k < n * n;
            if (!ok) { std::fprintf(stderr, "case %d: malformed\n", cases); return 2; }
            const std::vector<int32_t> members = Fi;
            grids(n, Fi, gx, mask);
            double alpha = 0.0;
            if (emu_splits_ratio_pass(n, threads, f, ci, co, &alpha, Fi.data(), xF.data(), sF.data(), cF.data(), gx.data(), mask.data()) != 0) {
                std::fprintf(stderr, "case %d: sizes outside the view\n", cases); return 2;
            }
            std::printf("ratio leave %d action %d f %d ftot %d enter_pos %d departed %d n_aside %d aside_enter %d steps %d alpha %a", co[0], co[1], co[2], co[3],
                        co[4], co[5], co[6], co[7], co[8], alpha);
            print_state(members, co[3], Fi.data(), xF.data(), cF.data(), gx, mask);
        } else if (kind == "append") {
            int32_t n, threads, r, ftot, fresh, ci[5], co[9];
            double dep, hkk, ll, lz;
            ok = read_i(in, n) && read_i(in, threads) && read_i(in, r) && read_i(in, ftot) && read_i(in, fresh) && read_d(in, dep) && read_d(in, hkk) &&
                 read_d(in, ll) && read_d(in, lz);
            for (int k = 0; k < 5 && ok; k++) ok = read_i(in, ci[k]);
            ok = ok && ftot > 0 && ftot < 4096 && r >= 0 && r < ftot && read_iv(in, Fi, ftot) && read_dv(in, xF, ftot) && read_dv(in, cF, ftot) && read_dv(in, rv, r);
            if (ok) for (int32_t k : Fi) ok = ok && k >= 0 && k < n * n;
            if (!ok) { std::fprintf(stderr, "case %d: malformed\n", cases); return 2; }
            const std::vector<int32_t> members = Fi;
            grids(n, Fi, gx, mask);
            mask[(size_t)Fi[(size_t)r]] = 0;  // (the split at r is not in the factor yet)
            std::vector<double> w((size_t)r + 1, -7.0);
            double z = -7.0;
            if (emu_splits_append_row(n, threads, r, ftot, fresh, dep, hkk, ll, lz, rv.data(), ci, co, Fi.data(), xF.data(), cF.data(), gx.data(), mask.data(),
                                      w.data(), &z) != 0) {
                std::fprintf(stderr, "case %d: sizes outside the view\n", cases); return 2;
            }
            std::printf("append f %d ftot %d enter_pos %d departed %d n_aside %d entered %d peak %d aside_fresh %d aside_rebuild %d z %a w", co[0], co[1], co[2],
                        co[3], co[4], co[5], co[6], co[7], co[8], z);
            for (double v : w) std::printf(" %a", v);
            print_state(members, co[1], Fi.data(), xF.data(), cF.data(), gx, mask);
        } else {
            std::fprintf(stderr, "case %d: unknown kind '%s'\n", cases, kind.c_str());
            return 2;
        }
        cases++;
    }
    std::printf("ok: %d cases\n", cases);
    return 0;
}

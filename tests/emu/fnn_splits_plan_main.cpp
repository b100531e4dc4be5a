// fnn_splits_plan_main.cpp -- a program of its own over fastneighbornet_amd/csrc/fnn_splits_plan.h, the host arithmetic of the
// split-weight solver's block method.  It reads one case per line from stdin, prints what the header's functions give and holds
// no expectation (tests/test_splits_plan.py compares).  Doubles travel as C99 hex floats ("nan" for a NaN).
//   plan n budget cap_want panel cap          -> plan cap kmax rcap pw kdiv rdiv fits cap_want elems f <hex> bytes <hex>
//   ratio m x[m] s[m] dead[m]                 -> ratio out ... alpha <hex> x <hex>[m]
//   compact m i[m] j[m] xw[m] cF[m] dead[m] r deadlist[r]
//                                             -> compact Fi ... Fj ... gonei ... gonej ... dead ... deadlist ... xw <hex>... cF <hex>...
//   revive f r nrev rev[nrev] dead[f] deadlist[r] -> revive keepcols ... newdead ... dead ...
//   objective m xs[m] cF[m] dead[m]           -> objective phi <hex>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../../fastneighbornet_amd/csrc/fnn_splits_plan.h"

using namespace fnnsw;

struct Split { int x, y; };

static double rd(std::istream& in) { std::string t; in >> t; return std::strtod(t.c_str(), nullptr); }
static std::vector<double> rdv(std::istream& in, size_t m) { std::vector<double> v(m); for (double& x : v) x = rd(in); return v; }
template <class Tp>
static std::vector<Tp> riv(std::istream& in, size_t m) { std::vector<Tp> v(m); for (Tp& x : v) { long long t; in >> t; x = (Tp)t; } return v; }
static void pd(double v) { if (v != v) std::printf(" nan"); else std::printf(" %a", v); }
template <class V>
static void pi(const char* key, const V& v) { std::printf(" %s", key); for (auto x : v) std::printf(" %lld", (long long)x); }
static void pdv(const char* key, const std::vector<double>& v) { std::printf(" %s", key); for (double x : v) pd(x); }

int main() {
    std::string line;
    long long cases = 0;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string kind;
        in >> kind;
        if (kind == "plan") {
            long long n, cap_want, panel;
            in >> n;
            const double budget = rd(in);
            in >> cap_want >> panel;
            Knobs kn;
            kn.panel = panel;
            kn.cap = rd(in);
            const CapacityPlan p = plan_capacity((int)n, budget, cap_want, kn);
            std::printf("plan cap %lld kmax %lld rcap %lld pw %lld kdiv %d rdiv %d fits %d cap_want %lld elems %lld f", (long long)p.cap, (long long)p.kmax,
                        (long long)p.rcap, (long long)p.pw, p.pick.kdiv, p.pick.rdiv, p.fits ? 1 : 0, (long long)p.cap_want, (long long)tri_elems(p.cap, p.pw));
            pd(p.pick.f);
            std::printf(" bytes");
            pd(p.bytes);
        } else if (kind == "ratio") {
            size_t m;
            in >> m;
            std::vector<double> x = rdv(in, m);
            const std::vector<double> s = rdv(in, m);
            const std::vector<uint8_t> dead = riv<uint8_t>(in, m);
            std::vector<int32_t> out;
            const double alpha = ratio_step(x, s, dead, out);
            std::printf("ratio");
            pi("out", out);
            std::printf(" alpha");
            pd(alpha);
            pdv("x", x);
        } else if (kind == "compact") {
            size_t m, r;
            in >> m;
            const std::vector<int> fi = riv<int>(in, m), fj = riv<int>(in, m);
            std::vector<double> xw = rdv(in, m), cF = rdv(in, m);
            std::vector<uint8_t> dead = riv<uint8_t>(in, m);
            in >> r;
            std::vector<int32_t> deadlist = riv<int32_t>(in, r);
            std::vector<Split> F(m), gone;
            for (size_t p = 0; p < m; p++) F[p] = Split{fi[p], fj[p]};
            compact_live(F, xw, cF, dead, deadlist, gone);
            std::vector<int> a, b, ga, gb;
            for (const Split& sp : F) { a.push_back(sp.x); b.push_back(sp.y); }
            for (const Split& sp : gone) { ga.push_back(sp.x); gb.push_back(sp.y); }
            std::printf("compact");
            pi("Fi", a); pi("Fj", b); pi("gonei", ga); pi("gonej", gb); pi("dead", dead); pi("deadlist", deadlist);
            pdv("xw", xw); pdv("cF", cF);
        } else if (kind == "revive") {
            size_t f, r, nrev;
            in >> f >> r >> nrev;
            const std::vector<int32_t> rev = riv<int32_t>(in, nrev);
            std::vector<uint8_t> dead = riv<uint8_t>(in, f);
            const std::vector<int32_t> deadlist = riv<int32_t>(in, r);
            std::vector<int32_t> keepcols, newdead;
            revival_lists(rev, (int64_t)f, dead, deadlist, keepcols, newdead);
            std::printf("revive");
            pi("keepcols", keepcols); pi("newdead", newdead); pi("dead", dead);
        } else if (kind == "objective") {
            size_t m;
            in >> m;
            const std::vector<double> xs = rdv(in, m), cF = rdv(in, m);
            const std::vector<uint8_t> dead = riv<uint8_t>(in, m);
            std::printf("objective phi");
            pd(objective(xs, cF, dead));
        } else {
            std::fprintf(stderr, "unknown case: %s\n", kind.c_str());
            return 2;
        }
        if (!in) { std::fprintf(stderr, "short case: %s\n", line.c_str()); return 2; }
        std::printf("\n");
        cases++;
    }
    std::printf("ok: %lld cases\n", cases);
    return 0;
}

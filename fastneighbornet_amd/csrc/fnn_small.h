// fnn_small.h -- the batched small-problem path: one workgroup runs a whole runNeighborNet
// (NetMakerOriginal.java:129-162) for 4 <= n <= SMALL_LDS_MAX_N out of LDS.  DESIGN.md section 11.
//
// The state is the reference's own: an n x n matrix addressed by distID whose shape never changes, and the
// packed position array N[0, m) with per position {id, distID, partner's position, Sx}.  SURVEY.md Appendix A
// is transcribed statement by statement; the comments cite its paragraphs.  Nothing of the one-problem
// engine's state (slots, windows, screening, certified choice) is used.
//
// Everything a thread does is an FNN_HD function of (tid, nthreads, view).  small_problem() strings the phases
// together through an executor: on the GPU (fnn_batch.hip) `all(f)` is f(threadIdx.x, blockDim.x) followed by
// __syncthreads(); in the CPU driver of the tests (tests/emu/fnn_batch_emu.cpp) it is a loop over tid.  The
// host side of the batch call (argument checks, chunking, validation, expansion) is small_batch<B>() below,
// shared by both in the same way Engine<B> is; small_ragged<B>() behind it is the same for problems of different sizes.
#ifndef FNN_SMALL_H
#define FNN_SMALL_H

#include <stdint.h>

#include <algorithm>
#include <map>

#include "fnn_engine.h"

namespace fnn {

constexpr int32_t SMALL_LDS_CAP = 163840;  // what one workgroup may declare on gfx950 (160 KiB)
constexpr int32_t SMALL_MAX_WAVES = 16;    // 1024 threads
constexpr int32_t SMALL_META_INTS = 8;     // per problem, to the host: {status, nlog, nev, last3[3], num_nodes, -}

enum { SMALL_OK = 0, SMALL_ERR_NO_PAIR = 1, SMALL_ERR_LOG_FULL = 2, SMALL_ERR_NO_PARTNER = 3 };

struct SmallCand { double q; int32_t i, j; };  // scan candidate at positions i > j; i < 0: none

struct SmallCtl {  // written by thread 0 in phases of its own; read by all after the barrier that ends such a phase
    int32_t m, c, num_nodes, nlog, nev, err, kind, pad0_;
    int32_t pcx, pcy;        // positions of Cx, Cy after the id swap
    int32_t px, py;          // positions of the chosen x, y
    int32_t pu, pv, py2;     // positions of u, u.nbr after a merge; of y2 between the two halves of agg4way
    int32_t X, Y, Z;         // distIDs of the running agg3way
    int32_t need_rx, pad_;
    double best, rx[4];      // scan minimum; Rx of Cx, Cx.nbr, Cy, Cy.nbr
    Event cur;
};

struct SmallLayout { int32_t ldm, off_sx, off_log, off_ctl, off_wred, off_id, off_did, off_pp, bytes; };

// Row stride in LDS: odd, so that a walk down a column (stride ldm doubles = 2 ldm dwords) spreads over all
// bank pairs instead of hitting one bank group when n is 64 or 128.
FNN_HD constexpr int32_t small_ldm(int32_t n) { return n | 1; }

FNN_HD constexpr SmallLayout small_layout(int32_t n) {
    SmallLayout L{};
    L.ldm = small_ldm(n);
    int32_t o = n * L.ldm * 8;                                    // the matrix
    L.off_sx = o;   o += n * 8;                                   // Sx per position
    L.off_log = o;  o += (n > 3 ? n - 3 : 1) * (int32_t)sizeof(Agg3Rec);  // merge log: one record per agg3way call, <= n - 3
    L.off_ctl = o;  o += (int32_t)sizeof(SmallCtl);
    L.off_wred = o; o += SMALL_MAX_WAVES * (int32_t)sizeof(SmallCand);
    L.off_id = o;   o += n * 4;
    L.off_did = o;  o += n * 4;
    L.off_pp = o;   o += n * 4;
    L.bytes = (o + 15) / 16 * 16;
    return L;
}

constexpr int32_t small_lds_max_n() {
    int32_t n = 4;
    while (small_layout(n + 1).bytes <= SMALL_LDS_CAP) n++;
    return n;
}
constexpr int32_t SMALL_LDS_MAX_N = small_lds_max_n();
static_assert(SMALL_LDS_MAX_N >= 128, "a 128-taxon problem must fit the LDS of one workgroup");
static_assert(sizeof(SmallCtl) % 8 == 0 && sizeof(SmallCand) == 16 && sizeof(Agg3Rec) == 16, "LDS layout");

// Workgroup size by n.  Unmeasured choice: the scan has m (m - 1) / 2 pairs to spread,
// everything else at most m items, and above 64 taxa the LDS admits few workgroups per CU anyway.
inline int32_t small_block_threads(int32_t n) { return n <= 64 ? 256 : (n <= 96 ? 512 : 1024); }

struct SmallView {
    double* D; double* Sx; Agg3Rec* log; SmallCtl* ctl; SmallCand* wred;
    int32_t *id, *did, *pp;  // per position: node id, distID, partner's position (-1: none)
    int32_t n, ldm;
    FNN_HD double& d(int32_t a, int32_t b) const { return D[a * ldm + b]; }  // D[a][b] by distID
};

FNN_HD SmallView small_view(unsigned char* base, int32_t n) {
    const SmallLayout L = small_layout(n);
    SmallView V;
    V.D = reinterpret_cast<double*>(base);
    V.Sx = reinterpret_cast<double*>(base + L.off_sx);
    V.log = reinterpret_cast<Agg3Rec*>(base + L.off_log);
    V.ctl = reinterpret_cast<SmallCtl*>(base + L.off_ctl);
    V.wred = reinterpret_cast<SmallCand*>(base + L.off_wred);
    V.id = reinterpret_cast<int32_t*>(base + L.off_id);
    V.did = reinterpret_cast<int32_t*>(base + L.off_did);
    V.pp = reinterpret_cast<int32_t*>(base + L.off_pp);
    V.n = n;
    V.ldm = L.ldm;
    return V;
}

struct alignas(16) SmallD2 { double a, b; };

// The matrix from global memory.  vec: the problem is dense (row stride n) and starts on a 16-byte boundary, so it is read
// as one run of 16-byte loads; otherwise element by element with row stride ld.  Consecutive threads read consecutive
// addresses either way.
FNN_HD void small_load(int tid, int nt, const SmallView& V, const double* g, int64_t ld, int vec) {
    const int32_t n = V.n, tot = n * n;
    if (vec) {
        const SmallD2* g2 = reinterpret_cast<const SmallD2*>(g);
        for (int32_t e = tid; e < tot / 2; e += nt) {
            const SmallD2 v = g2[e];
            const int32_t k = 2 * e, r = k / n, c = k - r * n;
            V.D[r * V.ldm + c] = v.a;
            if (c + 1 < n) V.D[r * V.ldm + c + 1] = v.b;
            else V.D[(r + 1) * V.ldm] = v.b;
        }
        if ((tot & 1) && tid == 0) V.D[(n - 1) * V.ldm + n - 1] = g[tot - 1];
    } else {
        for (int32_t e = tid; e < tot; e += nt) {
            const int32_t r = e / n, c = e - r * n;
            V.D[r * V.ldm + c] = g[(int64_t)r * ld + c];
        }
    }
}

// symmetric (bitwise), finite, zero diagonal - the rule of the one-problem engine's check
FNN_HD int small_validate_thread(int tid, int nt, const double* g, int32_t n, int64_t ld) {
    const uint64_t* u = reinterpret_cast<const uint64_t*>(g);
    int bad = 0;
    for (int32_t e = tid; e < n * n; e += nt) {
        const int32_t r = e / n, c = e - r * n;
        const uint64_t v = u[(int64_t)r * ld + c], t = u[(int64_t)c * ld + r];
        if (v != t) bad = 1;
        if (((v >> 52) & 0x7FF) == 0x7FF) bad = 1;
        if (r == c && v != 0) bad = 1;
    }
    return bad;
}

// A.1 set-up
FNN_HD void small_init_nodes(int tid, int nt, const SmallView& V) {
    for (int32_t k = tid; k < V.n; k += nt) { V.id[k] = k + 1; V.did[k] = k; V.pp[k] = -1; }
    if (tid == 0) {
        SmallCtl& K = *V.ctl;
        K = SmallCtl{};
        K.m = K.c = K.num_nodes = V.n;
    }
}

// A.2 initial sums: Sx[k] = left-to-right sum of D[0][k], ..., D[k-1][k], D[k][k+1], ..., D[k][n-1]
FNN_HD void small_init_sums(int tid, int nt, const SmallView& V) {
    for (int32_t k = tid; k < V.n; k += nt) {
        double s = 0.0;
        for (int32_t j = 0; j < k; j++) s += V.d(j, k);
        for (int32_t j = k + 1; j < V.n; j++) s += V.d(k, j);
        V.Sx[k] = s;
    }
}

FNN_HD bool small_rep(const SmallView& V, int32_t p) {  // p.nbr == null || p.nbr.id > p.id
    const int32_t q = V.pp[p];
    return q < 0 || V.id[q] > V.id[p];
}

// A.3 cluster distance CD(p, q), p the first argument (positions)
FNN_HD double small_cd(const SmallView& V, int32_t p, int32_t q) {
    const int32_t pn = V.pp[p], qn = V.pp[q], P = V.did[p], Q = V.did[q];
    if (pn < 0 && qn < 0) return V.d(P, Q);
    if (qn < 0) return (V.d(P, Q) + V.d(V.did[pn], Q)) / 2.0;
    if (pn < 0) return (V.d(P, Q) + V.d(P, V.did[qn])) / 2.0;
    const int32_t PN = V.did[pn], QN = V.did[qn];
    return (((V.d(P, Q) + V.d(P, QN)) + V.d(PN, Q)) + V.d(PN, QN)) / 4.0;
}

// total order (Q, i, j): does b come before a?  Its minimum is the first strict minimum of the i-ascending,
// j-ascending scan (the rule of wave_reduce in fnn_hip.hip).
FNN_HD bool small_before(const SmallCand& b, const SmallCand& a) {
    if (b.i < 0) return false;
    if (a.i < 0) return true;
    if (b.q < a.q) return true;
    if (b.q == a.q) return b.i < a.i || (b.i == a.i && b.j < a.j);
    return false;
}

// A.4 scan (NeighborNetCanonical.java:151-178), this thread's share: rows i = tid / 16 (+ nthreads / 16 ...), in each
// row the columns j = tid % 16 (+ 16 ...).  The thread visits its pairs i-ascending, j-ascending, so its own first
// strict minimum is its minimum under the total order.
FNN_HD SmallCand small_scan_thread(int tid, int nt, const SmallView& V, int32_t m, int32_t c) {
    SmallCand b{0.0, -1, -1};
    const double f = (double)c - 2.0;
    for (int32_t i = tid >> 4; i < m; i += nt >> 4) {
        if (!small_rep(V, i)) continue;  // one node per cluster
        const int32_t pn = V.pp[i];
        const double sxi = V.Sx[i];
        for (int32_t j = tid & 15; j < i; j += 16) {
            if (!small_rep(V, j)) continue;
            if (V.pp[j] == i) continue;
            const double Q = f * small_cd(V, i, j) - sxi - V.Sx[j];
            if ((b.i < 0 || Q < b.q) && pn != j) { b.q = Q; b.i = i; b.j = j; }
        }
    }
    return b;
}

// the scan's result from the per-wave records; Cx / Cy id swap (NetMakerOriginal.java:376-380); the event record's head
FNN_HD void small_pick(int tid, int nt, const SmallView& V, int32_t m, int32_t c) {
    if (tid != 0) return;
    SmallCtl& K = *V.ctl;
    SmallCand b = V.wred[0];
    for (int32_t w = 1; w < (nt + 63) / 64; w++) if (small_before(V.wred[w], b)) b = V.wred[w];
    if (b.i < 0) { K.err = SMALL_ERR_NO_PAIR; return; }  // unreachable for m >= 4, c >= 3
    int32_t cx = b.i, cy = b.j;
    if (V.id[cx] > V.id[cy]) { const int32_t t = cx; cx = cy; cy = t; }
    K.pcx = cx; K.pcy = cy; K.best = b.q;
    K.need_rx = (V.pp[cx] >= 0 || V.pp[cy] >= 0) ? 1 : 0;
    K.rx[0] = K.rx[1] = K.rx[2] = K.rx[3] = 0.0;
    K.cur = Event{};
    K.cur.m_before = m; K.cur.c_before = c;
    K.cur.cx_id = V.id[cx]; K.cur.cy_id = V.id[cy];
    K.cur.best = b.q;
    K.cur.entries = (int64_t)m * (m - 1) / 2 - (m - c);
}

// A.5 ComputeRx (:549-561): four sequential sums in position order, one lane each, on the first lanes of four waves
FNN_HD void small_rx(int tid, int nt, const SmallView& V, int32_t m) {
    if ((tid & 63) != 0 || (tid >> 6) >= 4) return;
    const SmallCtl& K = *V.ctl;
    const int32_t k = tid >> 6, cx = K.pcx, cy = K.pcy, cxn = V.pp[cx], cyn = V.pp[cy];
    const int32_t z = k == 0 ? cx : (k == 1 ? cxn : (k == 2 ? cy : cyn));
    if (z < 0) return;
    const int32_t Z = V.did[z];
    double r = 0.0;
    for (int32_t i = 0; i < m; i++) {
        const double v = V.d(Z, V.did[i]);
        if (i == cx || i == cxn || i == cy || i == cyn || V.pp[i] < 0) r += v;
        else r += v / 2.0;
    }
    V.ctl->rx[k] = r;
}

// A.5 the 4-candidate choice (:428-452), in the reference's order with strict <
FNN_HD void small_choose(const SmallView& V, int32_t c, int32_t& px, int32_t& py) {
    const SmallCtl& K = *V.ctl;
    const int32_t cx = K.pcx, cy = K.pcy, cxn = V.pp[cx], cyn = V.pp[cy];
    int32_t mm = c;
    if (cxn >= 0) mm++;
    if (cyn >= 0) mm++;
    const double f = (double)mm - 2.0;
    double best = f * V.d(V.did[cx], V.did[cy]) - K.rx[0] - K.rx[2];
    px = cx; py = cy;
    if (cxn >= 0) {
        const double Q = f * V.d(V.did[cxn], V.did[cy]) - K.rx[1] - K.rx[2];
        if (Q < best) { px = cxn; py = cy; best = Q; }
    }
    if (cyn >= 0) {
        const double Q = f * V.d(V.did[cx], V.did[cyn]) - K.rx[0] - K.rx[3];
        if (Q < best) { px = cx; py = cyn; best = Q; }
    }
    if (cxn >= 0 && cyn >= 0) {
        const double Q = f * V.d(V.did[cxn], V.did[cyn]) - K.rx[1] - K.rx[3];
        if (Q < best) { px = cxn; py = cyn; best = Q; }
    }
}

// subtractClusterDistance (:681-696) for the bystander at position p against t
FNN_HD void small_sub(const SmallView& V, int32_t p, int32_t t) {
    if (p != t && p != V.pp[t] && small_rep(V, p)) {
        const double v = small_cd(V, p, t);
        V.Sx[p] -= v;
        if (V.pp[p] >= 0) V.Sx[V.pp[p]] -= v;
    }
}

// A.5 subtract (:455-461): every thread makes the choice for itself (a handful of LDS reads; it spares a barrier), then
// position i, i not in {x.pos, y.pos}, subtracts for x, then for y.  Only the representative of a cluster writes, and it
// writes its own and its partner's Sx, so no two threads write one word.
FNN_HD void small_subtract(int tid, int nt, const SmallView& V, int32_t m, int32_t c) {
    int32_t px, py;
    small_choose(V, c, px, py);
    for (int32_t i = tid; i < m; i += nt) {
        if (i != px && i != py) { small_sub(V, i, px); small_sub(V, i, py); }
    }
    if (tid == 0) {
        SmallCtl& K = *V.ctl;
        K.px = px; K.py = py;
        K.cur.x_id = V.id[px]; K.cur.y_id = V.id[py];
    }
}

// A.6 agg3way(x, y, z) with live count m, the bookkeeping (:589-651): u replaces x, v replaces z, the last live node
// moves into y's place (swap with last).  Partners are kept as positions, so the moved node's partner learns its new
// place.  Thread 0 only.
FNN_HD void small_agg3_book(const SmallView& V, int32_t px, int32_t py, int32_t pz, int32_t m) {
    SmallCtl& K = *V.ctl;
    if (K.nlog >= V.n - 3) { K.err = SMALL_ERR_LOG_FULL; return; }  // unreachable: at most n - 3 agg3way calls
    const int32_t uid = K.num_nodes + 1;
    Agg3Rec r;
    r.u_id = uid; r.x_id = V.id[px]; r.y_id = V.id[py]; r.z_id = V.id[pz];
    V.log[K.nlog++] = r;
    K.X = V.did[px]; K.Y = V.did[py]; K.Z = V.did[pz];
    V.id[px] = uid;       // u inherits x's position and distID
    V.id[pz] = uid + 1;   // v inherits z's
    int32_t pu = px, pv = pz;
    const int32_t last = m - 1;
    if (last != py) {
        V.id[py] = V.id[last]; V.did[py] = V.did[last]; V.pp[py] = V.pp[last]; V.Sx[py] = V.Sx[last];
        if (last == pu) pu = py;
        else if (last == pv) pv = py;
        else if (V.pp[last] >= 0) V.pp[V.pp[last]] = py;
    }
    V.pp[pu] = pv; V.pp[pv] = pu;
    K.pu = pu; K.pv = pv;
    K.num_nodes += 2;
}

// A.6 the matrix update (:653-670) over the m - 1 live positions.  Every entry but D[X][Z] is independent of the loop's
// order; the aliased one is written by the iterations of u and of v, the later of which reads what the earlier wrote
// (compare agg3_special in fnn_core.h): the last thread replays those two iterations in position order.
FNN_HD void small_agg3_matrix(int tid, int nt, const SmallView& V, int32_t m) {
    const SmallCtl& K = *V.ctl;
    const int32_t X = K.X, Y = K.Y, Z = K.Z;
    for (int32_t i = tid; i < m - 1; i += nt) {
        const int32_t P = V.did[i];
        if (P == X || P == Z) continue;
        const double t1 = (2.0 / 3.0) * V.d(X, P) + V.d(Y, P) / 3.0;
        V.d(P, X) = t1; V.d(X, P) = t1;
        const double t2 = (2.0 / 3.0) * V.d(Z, P) + V.d(Y, P) / 3.0;
        V.d(P, Z) = t2; V.d(Z, P) = t2;
    }
    if (tid == nt - 1) {
        if (K.pu < K.pv) {
            const double t2 = (2.0 / 3.0) * V.d(Z, X) + V.d(Y, X) / 3.0;  // u's iteration (P = X), second statement
            V.d(X, Z) = t2; V.d(Z, X) = t2;
            const double t1 = (2.0 / 3.0) * V.d(X, Z) + V.d(Y, Z) / 3.0;  // v's iteration (P = Z), first statement
            V.d(Z, X) = t1; V.d(X, Z) = t1;
        } else {
            const double t1 = (2.0 / 3.0) * V.d(X, Z) + V.d(Y, Z) / 3.0;
            V.d(Z, X) = t1; V.d(X, Z) = t1;
            const double t2 = (2.0 / 3.0) * V.d(Z, X) + V.d(Y, X) / 3.0;
            V.d(X, Z) = t2; V.d(Z, X) = t2;
        }
        V.d(Z, Z) = 0.0;
        V.d(X, X) = 0.0;
    }
}

// A.5 merge (:462-488), thread 0: agg2way, or the bookkeeping of the (first) agg3way
FNN_HD void small_merge_book(int tid, int nt, const SmallView& V, int32_t m, int32_t c) {
    if (tid != 0) return;
    SmallCtl& K = *V.ctl;
    const int32_t px = K.px, py = K.py, xn = V.pp[px], yn = V.pp[py];
    if (xn < 0 && yn < 0) {           // agg2way (:570-577)
        V.pp[px] = py; V.pp[py] = px;
        K.pu = px; K.pv = py;
        K.kind = FNN_KIND_2WAY;
        K.cur.u_id = V.id[px];
        K.c = c - 1;
    } else if (xn < 0) {              // agg3way(x, y, y.nbr)
        K.kind = FNN_KIND_3WAY;
        K.cur.u_id = K.num_nodes + 1;
        small_agg3_book(V, px, py, yn, m);
        K.m = m - 1; K.c = c - 1;
    } else if (yn < 0 || m == 4) {    // agg3way(y, x, x.nbr)
        K.kind = FNN_KIND_3WAY;
        K.cur.u_id = K.num_nodes + 1;
        small_agg3_book(V, py, px, xn, m);
        K.m = m - 1; K.c = c - 1;
    } else {                          // agg4way(x.nbr, x, y, y.nbr): u = agg3way(x2, x, y) with m ...
        K.kind = FNN_KIND_4WAY;
        K.cur.u_id = K.num_nodes + 3;
        small_agg3_book(V, xn, px, py, m);
        K.py2 = (yn == m - 1) ? px : yn;  // (y2 moved into x's place if it was the last live node)
        K.m = m - 2; K.c = c - 1;
    }
    K.cur.kind = K.kind;
}

// ... then v = agg3way(u, u.nbr, y2) with m - 1 (:707-726)
FNN_HD void small_merge_book2(int tid, int nt, const SmallView& V, int32_t m) {
    if (tid != 0) return;
    SmallCtl& K = *V.ctl;
    small_agg3_book(V, K.pu, K.pv, K.py2, m - 1);
}

// A.5 add (updateClusterDistances :517-536): position i adds CD(p, u) to its own cluster's sums; u.Sx is the sequential
// sum of the same values in position order, by the last thread (it recomputes them: their loads do not depend on the
// running sum).  u and u.nbr take no part as bystanders, so their words have one writer.  Thread 0 emits the event.
FNN_HD void small_add(int tid, int nt, const SmallView& V, Event* gev) {
    SmallCtl& K = *V.ctl;
    const int32_t m = K.m, pu = K.pu, pv = K.pv;
    for (int32_t i = tid; i < m; i += nt) {
        if (small_rep(V, i) && i != pu && i != pv) {
            const double v = small_cd(V, i, pu);
            V.Sx[i] += v;
            if (V.pp[i] >= 0) V.Sx[V.pp[i]] += v;
        }
    }
    if (tid == nt - 1) {
        double s = 0.0;
        for (int32_t i = 0; i < m; i++)
            if (small_rep(V, i) && i != pu && i != pv) s += small_cd(V, i, pu);
        V.Sx[pu] = s;
        V.Sx[pv] = s;
    }
    if (tid == 0) {
        if (gev && K.nev < V.n) gev[K.nev] = K.cur;  // (every event takes a cluster away: fewer than n events)
        K.nev++;
    }
}

// A.7 special finish (:343-360), thread 0: the choice and the bookkeeping of its agg3way; the loop ends
FNN_HD void small_finish_book(int tid, int nt, const SmallView& V, Event* gev) {
    if (tid != 0) return;
    SmallCtl& K = *V.ctl;
    const int32_t p = 0, q = V.pp[0] != 1 ? 1 : 2, pn = V.pp[p], qn = V.pp[q];
    if (pn < 0 || qn < 0) { K.err = SMALL_ERR_NO_PARTNER; return; }  // unreachable: m == 4 && c == 2 is two pairs
    const int32_t P = V.did[p], Q = V.did[q], PN = V.did[pn], QN = V.did[qn];
    K.cur = Event{};
    K.cur.m_before = 4; K.cur.c_before = 2;
    K.cur.kind = FNN_KIND_FINISH;
    K.cur.x_id = V.id[p];
    K.cur.u_id = K.num_nodes + 1;
    if (V.d(P, Q) + V.d(PN, QN) < V.d(P, QN) + V.d(PN, Q)) {
        K.cur.y_id = V.id[q];
        small_agg3_book(V, p, q, qn, 4);
    } else {
        K.cur.y_id = V.id[qn];
        small_agg3_book(V, p, qn, q, 4);
    }
    if (gev && K.nev < V.n) gev[K.nev] = K.cur;  // (every event takes a cluster away: fewer than n events)
    K.nev++;
}

// the merge log and the final three nodes, for expandNodes on the host
FNN_HD void small_output(int tid, int nt, const SmallView& V, int32_t* gmeta, Agg3Rec* glog) {
    const SmallCtl& K = *V.ctl;
    for (int32_t k = tid; k < K.nlog; k += nt) glog[k] = V.log[k];
    if (tid == 0) {
        gmeta[0] = K.err; gmeta[1] = K.nlog; gmeta[2] = K.nev;
        gmeta[3] = V.id[0]; gmeta[4] = V.id[1]; gmeta[5] = V.id[2];
        gmeta[6] = K.num_nodes; gmeta[7] = 0;
    }
}

// The whole problem.  `ex.all(f)` runs f(tid, nthreads) for every thread and then waits for all of them; `ex.scan`
// runs small_scan_thread and leaves one record per wave in V.wred.  The control words read BETWEEN two phases (m, c at the
// loop top; err, need_rx, kind after a thread-0 phase) decide the branches, so every thread must see the same values:
//   - each was written before the barrier that ended the earlier phase (read after write), and
//   - none is written by the phase that FOLLOWS the read (write after read): a wave released from a barrier may still be
//     loading the word while wave 0 is already inside the next phase.  After the loop top come the scan or the special
//     finish's bookkeeping: neither writes m or c.  err and need_rx are read right after pick (then rx / subtract: they
//     write neither); err and kind right after a bookkeeping phase (then the matrix update, add or output: likewise).
// The loop ends by `break` alone; there is no "done" word that the finish would have to set under the other waves' eyes.
// The matrix is in LDS already.
template <class Exec>
FNN_HD void small_problem(Exec& ex, const SmallView& V, Event* gev, int32_t* gmeta, Agg3Rec* glog) {
    ex.all([&](int tid, int nt) { small_init_nodes(tid, nt, V); });
    ex.all([&](int tid, int nt) { small_init_sums(tid, nt, V); });
    for (;;) {  // agglomNodes (:339-393)
        const int32_t m = V.ctl->m, c = V.ctl->c;
        if (m <= 3) break;
        if (m == 4 && c == 2) {
            ex.all([&](int tid, int nt) { small_finish_book(tid, nt, V, gev); });
            if (!V.ctl->err) ex.all([&](int tid, int nt) { small_agg3_matrix(tid, nt, V, 4); });
            break;
        }
        ex.scan(V, m, c);
        ex.all([&](int tid, int nt) { small_pick(tid, nt, V, m, c); });
        if (V.ctl->err) break;
        if (V.ctl->need_rx) ex.all([&](int tid, int nt) { small_rx(tid, nt, V, m); });
        ex.all([&](int tid, int nt) { small_subtract(tid, nt, V, m, c); });
        ex.all([&](int tid, int nt) { small_merge_book(tid, nt, V, m, c); });
        if (V.ctl->err) break;
        const int32_t kind = V.ctl->kind;
        if (kind != FNN_KIND_2WAY) ex.all([&](int tid, int nt) { small_agg3_matrix(tid, nt, V, m); });
        if (kind == FNN_KIND_4WAY) {
            ex.all([&](int tid, int nt) { small_merge_book2(tid, nt, V, m); });
            if (V.ctl->err) break;
            ex.all([&](int tid, int nt) { small_agg3_matrix(tid, nt, V, m - 1); });
        }
        ex.all([&](int tid, int nt) { small_add(tid, nt, V, gev); });
    }
    ex.all([&](int tid, int nt) { small_output(tid, nt, V, gmeta, glog); });
}

// ------------------------------------------------------------------------------------------------ host side
// fnn_canonical_order_batch[_device]_f64 over a backend B (HIP: fnn_batch.hip; CPU driver: tests/emu):
//   open(device); alloc / release; h2d / d2h; validate(...); run(...); fallback(...); err()
// Results go to the caller's arrays only when the whole call has succeeded.
constexpr int64_t SMALL_CHUNK_BYTES = (int64_t)2 << 30;  // device buffer for matrices per chunk

// ---- steps that every batch call takes (the routes of this header, fnn_small_global.h and fnn_small_splits.h), one
// definition each.  A call reads a switch once, before its first chunk.
// FNN_BATCH_THREADS=256|512|1024: the block size of every launch of the call; 0: not set
inline int32_t batch_threads_switch() {
    if (const char* e = std::getenv("FNN_BATCH_THREADS")) { int v = std::atoi(e); if (v == 256 || v == 512 || v == 1024) return v; }
    return 0;
}
// FNN_BATCH_CHUNK=<problems >= 1>: the problems of one chunk; 0: not set
inline int64_t batch_chunk_switch() {
    if (const char* e = std::getenv("FNN_BATCH_CHUNK")) { long long v = std::atoll(e); if (v >= 1) return v; }
    return 0;
}
// Problems per chunk of a same-size call: what SMALL_CHUNK_BYTES holds (or the switch), at most the batch, at least one.
// even: as many chunks, of equal size (no short last launch).
inline int64_t batch_chunk(int64_t batch, int64_t bytes_per_problem, bool even) {
    int64_t chunk = SMALL_CHUNK_BYTES / bytes_per_problem;
    if (const int64_t v = batch_chunk_switch()) chunk = v;
    if (chunk > batch) chunk = batch;
    if (chunk < 1) chunk = 1;
    if (even) { const int64_t chunks = (batch + chunk - 1) / chunk; chunk = (batch + chunks - 1) / chunks; }
    return chunk;
}
// the rows of one n x n matrix (row stride ld) to an image with row stride dld; what lies between the rows is not written
inline void pack_rows(double* dst, int64_t dld, const double* src, int64_t ld, int32_t n) {
    for (int32_t r = 0; r < n; r++) std::memcpy(dst + (int64_t)r * dld, src + (int64_t)r * ld, sizeof(double) * (size_t)n);
}
// the two failures that name the caller's index of the problem at fault
inline int32_t fail_bad_matrix(const std::string& W, int64_t b) {
    return fail(FNN_EINVAL, W + "problem " + std::to_string(b) + ": matrix is not symmetric, not finite or has a non-zero diagonal");
}
inline int32_t fail_nonfinite(const std::string& W, int64_t b) {
    return fail(FNN_EINVAL, W + "problem " + std::to_string(b) + ": the distances contain a NaN or an infinity");
}
// The outputs of an order call.  The call fills these and commits as its last step: a failing call returns before that
// and leaves the caller's arrays untouched.
struct OrderStage {
    std::vector<int32_t> orders, nev;
    std::vector<fnn_event> evs;  // (zero: the fill behind each problem's last event; empty when no events are wanted)
    OrderStage(int64_t batch, size_t order_ints, size_t event_recs) : orders(order_ints), nev((size_t)batch, 0), evs(event_recs) {}
    void commit(int32_t* orders_out, fnn_event* events_out, int32_t* nevents_out) const {
        std::memcpy(orders_out, orders.data(), sizeof(int32_t) * orders.size());
        if (events_out) std::memcpy(events_out, evs.data(), sizeof(fnn_event) * evs.size());
        if (nevents_out) std::memcpy(nevents_out, nev.data(), sizeof(int32_t) * nev.size());
    }
};

// One chunk's result records (problems b0 ... b0 + cnt - 1) to orders, event counts and the zero fill behind each problem's
// last event; shared by the LDS route below and the global-memory route (fnn_small_global.h).
// one problem's result record (mt: its SMALL_META_INTS words, log: its merge log) to its order; the caller's index is `b`
inline int32_t small_collect_one(const std::string& W, int32_t n, int64_t b, const int32_t* mt, const Agg3Rec* log, int32_t* order) {
    const std::string P = W + "problem " + std::to_string(b) + ": ";
    if (mt[0] != SMALL_OK) return fail(FNN_EHIP, P + "the kernel took an unreachable branch (status " + std::to_string(mt[0]) + ")");
    const int32_t nn = mt[6];
    if (mt[1] < 0 || mt[1] > n - 3 || mt[2] < 0 || mt[2] >= n || nn < n || nn > 3 * n) return fail(FNN_EHIP, P + "corrupt result record");
    for (int k = 3; k < 6; k++) if (mt[k] < 1 || mt[k] > nn) return fail(FNN_EHIP, P + "corrupt result record");
    const char* why = expand_merge_log(n, nn, log, (size_t)mt[1], mt + 3, order);
    if (why) return fail(FNN_ESTATE, P + why);
    return FNN_OK;
}

inline int32_t small_collect(const std::string& W, int32_t n, int64_t b0, int64_t cnt, const int32_t* meta, const Agg3Rec* log,
                             int32_t* orders, int32_t* nev, fnn_event* evs, fnn_batch_stats& st) {
    for (int64_t b = 0; b < cnt; b++) {
        const int32_t* mt = &meta[(size_t)b * SMALL_META_INTS];
        const int32_t rc = small_collect_one(W, n, b0 + b, mt, &log[(size_t)b * (size_t)n], &orders[(size_t)(b0 + b) * (size_t)(n + 1)]);
        if (rc != FNN_OK) return rc;
        nev[(size_t)(b0 + b)] = mt[2];
        if (evs)  // (the records past the problem's last event were never written)
            std::memset(&evs[(size_t)(b0 + b) * (size_t)n + (size_t)mt[2]], 0, sizeof(fnn_event) * (size_t)(n - mt[2]));
        st.n_events += mt[2];
    }
    return FNN_OK;
}

template <class B>
int32_t small_batch(B& be, const char* who, const double* D, bool on_device, int32_t n, int64_t ld, int64_t stride, int64_t batch,
                    const fnn_opts* o, int32_t* orders_out, fnn_event* events_out, int32_t* nevents_out, fnn_batch_stats* stats) {
    const double t0 = now_s();
    const std::string W = std::string(who) + ": ";
    fnn_batch_stats st{};
    st.lds_max_n = SMALL_LDS_MAX_N;
    if (n < 0 || batch < 0) return fail(FNN_EINVAL, W + "n < 0 or batch < 0");
    fnn_opts opts{};
    if (o) opts = *o;
    if (opts.mode != FNN_MODE_CANONICAL && opts.mode != FNN_MODE_RELAXED) return fail(FNN_EINVAL, W + "unknown mode");
    if (batch == 0) { if (stats) *stats = st; return FNN_OK; }
    if (!orders_out || (n > 0 && !D)) return fail(FNN_EINVAL, W + "NULL argument");
    if (n > 0 && (ld < n || stride < (int64_t)n * ld)) return fail(FNN_EINVAL, W + "needs ld >= n and stride >= n * ld");
    st.n_problems = batch;
    if (n <= 3) {  // NetMakerOriginal.java:133-140: the identity, no device needed
        for (int64_t b = 0; b < batch; b++)
            for (int32_t i = 0; i <= n; i++) orders_out[b * (n + 1) + i] = i;
        if (nevents_out) for (int64_t b = 0; b < batch; b++) nevents_out[b] = 0;
        st.t_total_s = now_s() - t0;
        if (stats) *stats = st;
        return FNN_OK;
    }
    OrderStage out(batch, (size_t)batch * (size_t)(n + 1), events_out ? (size_t)batch * (size_t)n : 0);
    int32_t rc;
    if (n > SMALL_LDS_MAX_N) {  // too large for LDS: the one-problem engine, one handle for all
        rc = be.fallback(W, D, on_device, n, ld, stride, batch, opts, out.orders.data(), events_out ? out.evs.data() : nullptr, out.nev.data(), st);
        if (rc != FNN_OK) return rc;
    } else {
        rc = be.open(opts.device);
        if (rc != FNN_OK) return fail(rc, W + be.err());
        const SmallLayout L = small_layout(n);
        st.block_threads = small_block_threads(n);
        if (const int32_t v = batch_threads_switch()) st.block_threads = v;
        st.lds_bytes = L.bytes;
        const int64_t pitch = round_up((int64_t)n * n, 2);  // doubles per problem in the device buffer: every problem 16-byte aligned
        const int64_t chunk = batch_chunk(batch, 8 * pitch, false);  // (the last chunk may be short)
        // the caller's array is the device image already only if it is dense and every problem 16-byte aligned in it; anything
        // else is packed (an upload of whole pitches from the caller's array would read past its last problem)
        const bool dense = ld == n && stride == (int64_t)n * n && stride == pitch;
        double* dD = nullptr;
        int32_t* d_meta = (int32_t*)be.alloc(sizeof(int32_t) * SMALL_META_INTS * (size_t)chunk);
        Agg3Rec* d_log = (Agg3Rec*)be.alloc(sizeof(Agg3Rec) * (size_t)n * (size_t)chunk);
        Event* d_ev = events_out ? (Event*)be.alloc(sizeof(Event) * (size_t)n * (size_t)chunk) : nullptr;
        if (!on_device) dD = (double*)be.alloc(sizeof(double) * (size_t)pitch * (size_t)chunk);
        if (!d_meta || !d_log || (events_out && !d_ev) || (!on_device && !dD)) return fail(FNN_ENOMEM, W + "device allocation failed");
        std::vector<double> pack(on_device || dense ? 0 : (size_t)pitch * (size_t)chunk);
        std::vector<int32_t> meta((size_t)SMALL_META_INTS * (size_t)chunk);
        std::vector<Agg3Rec> log((size_t)n * (size_t)chunk);
        for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
            const int64_t cnt = batch - b0 < chunk ? batch - b0 : chunk;
            st.chunks++;
            const double* src = D + b0 * stride;
            int64_t kld = ld, kstride = stride;
            if (!on_device) {
                const double tu = now_s();
                const double* up = src;
                if (!dense) {  // rows to a dense image (padding is never read)
                    for (int64_t b = 0; b < cnt; b++) pack_rows(&pack[(size_t)(b * pitch)], n, src + b * stride, ld, n);
                    up = pack.data();
                }
                if (be.h2d(dD, up, sizeof(double) * (size_t)(cnt * pitch)) != FNN_OK) return fail(FNN_EHIP, W + "upload failed (" + be.err() + ")");
                st.t_upload_s += now_s() - tu;
                src = dD; kld = n; kstride = pitch;
            }
            if (opts.validate) {
                int64_t bad = -1;
                if (be.validate(src, n, kld, kstride, cnt, &bad) != FNN_OK) return fail(FNN_EHIP, W + "validate failed (" + be.err() + ")");
                if (bad >= 0) return fail_bad_matrix(W, b0 + bad);
            }
            double tk = 0.0;
            if (be.run(src, n, kld, kstride, cnt, st.block_threads, L.bytes, d_meta, d_log, d_ev, &tk) != FNN_OK)
                return fail(FNN_EHIP, W + "kernel failed (" + be.err() + ")");
            st.t_kernel_s += tk;
            if (be.d2h(meta.data(), d_meta, sizeof(int32_t) * SMALL_META_INTS * (size_t)cnt) != FNN_OK ||
                be.d2h(log.data(), d_log, sizeof(Agg3Rec) * (size_t)n * (size_t)cnt) != FNN_OK ||
                (d_ev && be.d2h(&out.evs[(size_t)b0 * (size_t)n], d_ev, sizeof(Event) * (size_t)n * (size_t)cnt) != FNN_OK))
                return fail(FNN_EHIP, W + "download failed (" + be.err() + ")");
            rc = small_collect(W, n, b0, cnt, meta.data(), log.data(), out.orders.data(), out.nev.data(), events_out ? out.evs.data() : nullptr, st);
            if (rc != FNN_OK) return rc;
            st.n_lds += cnt;
        }
    }
    out.commit(orders_out, events_out, nevents_out);
    st.t_total_s = now_s() - t0;
    if (stats) *stats = st;
    return FNN_OK;
}

// ------------------------------------------------------------------------------------------------ ragged batches
// Problems of different sizes in one call.  A workgroup of k_small_ragged / k_small_splits_ragged
// reads ONE descriptor and runs the unchanged small_problem() / small_splits_problem() on it.  All offsets count
// elements of the array they point into, from that array's base.
struct RaggedDesc {
    int64_t src, ld;         // the matrix: offset from the base pointer and row stride, in doubles
    int64_t id;              // the caller's index of the problem
    int64_t meta;            // result record: int32 words (orders), SplitsMeta records (weights)
    int64_t log, ev;         // orders: merge log (Agg3Rec) and events (Event)
    int64_t ord, out, work;  // weights: ordering (int32), weights and workspace slice (doubles)
    int32_t n, vec, cap, pad_;  // vec: dense and 16-byte aligned, read by 16-byte loads; cap: splits the factor holds
};
static_assert(sizeof(RaggedDesc) == 88, "descriptor layout");

// One launch: descriptors first ... first + count - 1 of the chunk's sorted array, one block size, one dynamic-LDS size.
struct RaggedClass { int64_t first, count; int32_t threads, lds_bytes; };

constexpr int32_t RAGGED_CU_THREADS = 2048;  // 32 waves per CU
constexpr int32_t RAGGED_MAX_CLASSES = 8;

// Workgroups of this shape that one CU holds at a time, rounded down to a power of two: the class key next to the block size.
inline int32_t ragged_resident(int32_t threads, int32_t lds_bytes) {
    int32_t r = SMALL_LDS_CAP / lds_bytes;
    if (r > RAGGED_CU_THREADS / threads) r = RAGGED_CU_THREADS / threads;
    int32_t p = 1;
    while (2 * p <= r) p *= 2;
    return p;
}

// Sorts a chunk's descriptors by descending n (ties: the caller's index) and cuts them into classes wherever the block
// size or the residency step changes.  Both are monotone in n, so a class is a range of n: it never straddles 64|65 or
// 96|97, and a problem is never launched under a reservation that halves the workgroups per CU its own size allows.  A
// class reserves the LDS of its largest member.  lds_of(desc) = the problem's own dynamic LDS in bytes; threads_switch =
// what batch_threads_switch() gave the call.
template <class LdsOf>
inline void ragged_classes(std::vector<RaggedDesc>& d, int32_t threads_switch, LdsOf lds_of, std::vector<RaggedClass>& out) {
    std::sort(d.begin(), d.end(), [](const RaggedDesc& a, const RaggedDesc& b) { return a.n != b.n ? a.n > b.n : a.id < b.id; });
    out.clear();
    int32_t key_t = 0, key_r = 0;
    for (size_t k = 0; k < d.size(); k++) {
        const int32_t t = threads_switch ? threads_switch : small_block_threads(d[k].n), bytes = lds_of(d[k]), r = ragged_resident(t, bytes);
        if (out.empty() || t != key_t || r != key_r) {
            out.push_back(RaggedClass{(int64_t)k, 0, t, bytes});
            key_t = t; key_r = r;
        }
        out.back().count++;
        if (bytes > out.back().lds_bytes) out.back().lds_bytes = bytes;
    }
}

// Consecutive runs of `items` (indices into the caller's arrays), each at most max_count problems and max_bytes bytes of
// bytes_of(index), at least one problem: cut[c] ... cut[c + 1] - 1 is chunk c.  FNN_BATCH_CHUNK=<problems> is honoured.
template <class BytesOf>
inline std::vector<int64_t> ragged_chunks(const std::vector<int64_t>& items, BytesOf bytes_of) {
    int64_t max_count = INT64_MAX;
    if (const int64_t v = batch_chunk_switch()) max_count = v;
    std::vector<int64_t> cut{0};
    int64_t bytes = 0, count = 0;
    for (size_t k = 0; k < items.size(); k++) {
        const int64_t w = bytes_of(items[k]);
        if (count > 0 && (count >= max_count || bytes + w > SMALL_CHUNK_BYTES)) { cut.push_back((int64_t)k); bytes = 0; count = 0; }
        bytes += w; count++;
    }
    cut.push_back((int64_t)items.size());
    return cut;
}

// fnn_canonical_order_ragged[_device]_f64 over a backend B (HIP: fnn_batch.hip; CPU driver: tests/emu/fnn_ragged_emu.cpp):
// small_batch's open / alloc / h2d / d2h / err and
//   validate_ragged(base, d_desc, cnt, &bad)        bad = the lowest caller's index whose matrix fails the check, or -1
//   run_ragged(base, d_desc, classes, ncls, d_meta, d_log, d_ev, &t_kernel_s)     one launch per class
//   large(W, D, on_device, n, offs, lds, cnt, opts, run, orders, events, nev, &stats, &bad)
//       cnt problems of ONE size above the LDS limit through the same-size entry (which picks the global-memory kernel or
//       the one-problem engine by its own rule); bad = index into offs of the lowest problem that fails the check, or -1;
//       run == false: the check alone
// Problem b is the ns[b] x ns[b] matrix at D + offsets[b] with row stride lds[b] (lds == NULL: ns[b]).  Outputs are
// concatenated in the caller's order, whatever order the device runs the problems in.
template <class B>
int32_t small_ragged(B& be, const char* who, const double* D, bool on_device, const int64_t* offsets, const int32_t* ns, const int64_t* lds,
                     int64_t batch, const fnn_opts* o, int32_t* orders_out, fnn_event* events_out, int32_t* nevents_out, fnn_batch_stats* stats) {
    const double t0 = now_s();
    const std::string W = std::string(who) + ": ";
    fnn_batch_stats st{};
    st.lds_max_n = SMALL_LDS_MAX_N;
    if (batch < 0) return fail(FNN_EINVAL, W + "batch < 0");
    fnn_opts opts{};
    if (o) opts = *o;
    if (opts.mode != FNN_MODE_CANONICAL && opts.mode != FNN_MODE_RELAXED) return fail(FNN_EINVAL, W + "unknown mode");
    if (batch == 0) { if (stats) *stats = st; return FNN_OK; }
    if (!offsets || !ns || !orders_out) return fail(FNN_EINVAL, W + "NULL argument");
    auto ld_of = [&](int64_t b) { return lds ? lds[b] : (int64_t)ns[b]; };
    std::vector<int64_t> oo((size_t)batch + 1, 0), eo((size_t)batch + 1, 0);  // where problem b's order and events start
    std::vector<int64_t> kern;                                                // kernel range, in the caller's order
    std::map<int32_t, std::vector<int64_t>> large;                            // above it, by size
    for (int64_t b = 0; b < batch; b++) {
        const int32_t n = ns[b];
        if (n < 0) return fail(FNN_EINVAL, W + "problem " + std::to_string(b) + ": n < 0");
        if (ld_of(b) < n) return fail(FNN_EINVAL, W + "problem " + std::to_string(b) + ": needs ld >= n");
        if (n > 0 && !D) return fail(FNN_EINVAL, W + "NULL argument");
        oo[(size_t)b + 1] = oo[(size_t)b] + n + 1;
        eo[(size_t)b + 1] = eo[(size_t)b] + n;
        if (n > SMALL_LDS_MAX_N) large[n].push_back(b);
        else if (n > 3) kern.push_back(b);
    }
    st.n_problems = batch;
    OrderStage out(batch, (size_t)oo[(size_t)batch], events_out ? (size_t)eo[(size_t)batch] : 0);
    for (int64_t b = 0; b < batch; b++)
        if (ns[b] <= 3)  // NetMakerOriginal.java:133-140: the identity, no device needed
            for (int32_t i = 0; i <= ns[b]; i++) out.orders[(size_t)(oo[(size_t)b] + i)] = i;
    int64_t bad = -1;  // the lowest caller's index that fails the check
    int32_t rc;
    if (!kern.empty() || !large.empty()) {
        rc = be.open(opts.device);
        if (rc != FNN_OK) return fail(rc, W + be.err());
    }
    if (!kern.empty()) {
        auto pitch_of = [&](int64_t b) { return round_up((int64_t)ns[b] * ns[b], 2); };  // every problem 16-byte aligned in the image
        const std::vector<int64_t> cut = ragged_chunks(kern, [&](int64_t b) { return 8 * pitch_of(b); });
        int64_t mcnt = 0, mrec = 0, mimg = 0;  // the largest chunk: problems, log / event records, doubles of the image
        for (size_t c = 0; c + 1 < cut.size(); c++) {
            int64_t rec = 0, img = 0;
            for (int64_t k = cut[c]; k < cut[c + 1]; k++) { rec += ns[kern[(size_t)k]]; img += pitch_of(kern[(size_t)k]); }
            mcnt = std::max(mcnt, cut[c + 1] - cut[c]); mrec = std::max(mrec, rec); mimg = std::max(mimg, img);
        }
        int32_t* d_meta = (int32_t*)be.alloc(sizeof(int32_t) * SMALL_META_INTS * (size_t)mcnt);
        Agg3Rec* d_log = (Agg3Rec*)be.alloc(sizeof(Agg3Rec) * (size_t)mrec);
        Event* d_ev = events_out ? (Event*)be.alloc(sizeof(Event) * (size_t)mrec) : nullptr;
        RaggedDesc* d_desc = (RaggedDesc*)be.alloc(sizeof(RaggedDesc) * (size_t)mcnt);
        double* dD = on_device ? nullptr : (double*)be.alloc(sizeof(double) * (size_t)mimg);
        if (!d_meta || !d_log || (events_out && !d_ev) || !d_desc || (!on_device && !dD)) return fail(FNN_ENOMEM, W + "device allocation failed");
        std::vector<double> pack(on_device ? 0 : (size_t)mimg);
        std::vector<int32_t> meta((size_t)SMALL_META_INTS * (size_t)mcnt);
        std::vector<Agg3Rec> log((size_t)mrec);
        std::vector<fnn_event> cev(events_out ? (size_t)mrec : 0);
        std::vector<RaggedDesc> slot, sorted;  // the chunk's descriptors in the caller's order / in launch order
        std::vector<RaggedClass> classes;
        const int32_t threads_switch = batch_threads_switch();
        for (size_t c = 0; c + 1 < cut.size() && bad < 0; c++) {
            const int64_t cnt = cut[c + 1] - cut[c];
            slot.clear();
            int64_t rec = 0, img = 0;
            const double tu = now_s();
            for (int64_t k = 0; k < cnt; k++) {
                const int64_t b = kern[(size_t)(cut[c] + k)];
                const int32_t n = ns[b];
                RaggedDesc d{};
                d.id = b; d.n = n;
                d.meta = k * SMALL_META_INTS; d.log = rec; d.ev = rec;
                if (on_device) {  // in place; 16-byte loads only where the problem is dense and aligned
                    d.src = offsets[b]; d.ld = ld_of(b);
                    d.vec = (d.ld == n && reinterpret_cast<uintptr_t>(D + offsets[b]) % 16 == 0) ? 1 : 0;
                } else {          // rows to the dense image (padding is never read)
                    pack_rows(&pack[(size_t)img], n, D + offsets[b], ld_of(b), n);
                    d.src = img; d.ld = n; d.vec = 1;
                    img += pitch_of(b);
                }
                rec += n;
                slot.push_back(d);
            }
            sorted = slot;
            ragged_classes(sorted, threads_switch, [](const RaggedDesc& d) { return small_layout(d.n).bytes; }, classes);
            if ((int64_t)classes.size() > RAGGED_MAX_CLASSES) return fail(FNN_ESTATE, W + "more size classes than launches allowed");
            if ((!on_device && be.h2d(dD, pack.data(), sizeof(double) * (size_t)img) != FNN_OK) ||
                be.h2d(d_desc, sorted.data(), sizeof(RaggedDesc) * (size_t)cnt) != FNN_OK)
                return fail(FNN_EHIP, W + "upload failed (" + be.err() + ")");
            st.t_upload_s += now_s() - tu;
            const double* base = on_device ? D : dD;
            if (opts.validate) {
                if (be.validate_ragged(base, d_desc, cnt, &bad) != FNN_OK) return fail(FNN_EHIP, W + "validate failed (" + be.err() + ")");
                if (bad >= 0) break;  // (chunks follow the caller's order: no later chunk holds a lower index)
            }
            double tk = 0.0;
            if (be.run_ragged(base, d_desc, classes.data(), (int32_t)classes.size(), d_meta, d_log, d_ev, &tk) != FNN_OK)
                return fail(FNN_EHIP, W + "kernel failed (" + be.err() + ")");
            st.t_kernel_s += tk;
            st.chunks += (int32_t)classes.size();
            if (classes[0].lds_bytes > st.lds_bytes) { st.lds_bytes = classes[0].lds_bytes; st.block_threads = classes[0].threads; }
            if (be.d2h(meta.data(), d_meta, sizeof(int32_t) * SMALL_META_INTS * (size_t)cnt) != FNN_OK ||
                be.d2h(log.data(), d_log, sizeof(Agg3Rec) * (size_t)rec) != FNN_OK ||
                (d_ev && be.d2h(cev.data(), d_ev, sizeof(Event) * (size_t)rec) != FNN_OK))
                return fail(FNN_EHIP, W + "download failed (" + be.err() + ")");
            for (const RaggedDesc& d : slot) {
                const int32_t* mt = &meta[(size_t)d.meta];
                rc = small_collect_one(W, d.n, d.id, mt, &log[(size_t)d.log], &out.orders[(size_t)oo[(size_t)d.id]]);
                if (rc != FNN_OK) return rc;
                out.nev[(size_t)d.id] = mt[2];
                if (events_out) std::memcpy(&out.evs[(size_t)eo[(size_t)d.id]], &cev[(size_t)d.ev], sizeof(fnn_event) * (size_t)mt[2]);
                st.n_events += mt[2];
            }
            st.n_lds += cnt;
        }
    }
    std::vector<int64_t> offs, glds;
    std::vector<int32_t> go, gn;
    std::vector<fnn_event> ge;
    for (const auto& g : large) {  // (after a failed check only the check runs: a lower index may still fail it)
        const int32_t n = g.first;
        const int64_t cnt = (int64_t)g.second.size();
        offs.clear(); glds.clear();
        for (int64_t b : g.second) { offs.push_back(offsets[b]); glds.push_back(ld_of(b)); }
        go.assign((size_t)cnt * (size_t)(n + 1), 0);
        gn.assign((size_t)cnt, 0);
        ge.assign(events_out ? (size_t)cnt * (size_t)n : 0, fnn_event{});
        fnn_batch_stats gs{};
        int64_t gbad = -1;
        rc = be.large(W, D, on_device, n, offs.data(), glds.data(), cnt, opts, bad < 0, go.data(), events_out ? ge.data() : nullptr, gn.data(), &gs, &gbad);
        if (rc != FNN_OK) return rc;
        if (gbad >= 0) { if (bad < 0 || g.second[(size_t)gbad] < bad) bad = g.second[(size_t)gbad]; continue; }
        if (bad >= 0) continue;
        for (int64_t k = 0; k < cnt; k++) {
            const int64_t b = g.second[(size_t)k];
            std::memcpy(&out.orders[(size_t)oo[(size_t)b]], &go[(size_t)k * (size_t)(n + 1)], sizeof(int32_t) * (size_t)(n + 1));
            out.nev[(size_t)b] = gn[(size_t)k];
            if (events_out) std::memcpy(&out.evs[(size_t)eo[(size_t)b]], &ge[(size_t)k * (size_t)n], sizeof(fnn_event) * (size_t)n);
        }
        st.n_global += gs.n_global; st.n_fallback += gs.n_fallback; st.n_lds += gs.n_lds; st.n_events += gs.n_events;
        st.chunks += gs.chunks; st.t_upload_s += gs.t_upload_s; st.t_kernel_s += gs.t_kernel_s;
    }
    if (bad >= 0) return fail_bad_matrix(W, bad);
    out.commit(orders_out, events_out, nevents_out);
    st.t_total_s = now_s() - t0;
    if (stats) *stats = st;
    return FNN_OK;
}

}  // namespace fnn
#endif

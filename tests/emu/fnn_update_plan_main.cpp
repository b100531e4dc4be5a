// fnn_update_plan_main.cpp -- TEST INFRASTRUCTURE ONLY.
//
// Stand-alone check of the packed update plan (fnn_core.h: UpdPlan): for random but well-formed plans in a control block,
// upd_plan_view(upd_plan_pack(st)) must equal plan_view(st, UniId{}) field by field.  Two generators:
//   * the four event kinds as decide_plan / finish_plan lay them out (agg2way: swaps; agg3way: one AGG3 + a move; agg4way: two
//     AGG3 + up to four moves; the special finish), replayed by build_targets - the plans a run really produces;
//   * plans drawn field by field: every nS in 2..8 with every ntgt in 0..nS, every recipe kind, operands present and absent (-1),
//     x / y with and without a partner, stale entries beyond ntgt and beyond nS.
// The program ends with the coverage it reached and fails if a class was not met.  It has its own main: it can be built with
// -fsanitize=address,undefined and run directly (tests/test_update_plan_pack.py does both).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../fastneighbornet_amd/csrc/fnn_core.h"

using namespace fnn;

static uint64_t g_rng = 0x9E3779B97F4A7C15ULL;
static uint32_t rnd(uint32_t bound) {  // splitmix64, uniform enough for a test
    g_rng += 0x9E3779B97F4A7C15ULL;
    uint64_t z = g_rng;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    z ^= z >> 31;
    return (uint32_t)(z % bound);
}

struct Coverage {
    long plans = 0, nS[MAX_S + 1] = {}, ntgt[MAX_TGT + 1] = {}, kind[4] = {}, events[6] = {};
    long xn_absent = 0, xn_present = 0, yn_absent = 0, yn_present = 0, op_absent = 0, op_present = 0, finish = 0;
};
static Coverage cov;

static int compare(const State& st, const char* what, long trial) {
    const PlanView a = plan_view(st, UniId{});
    const UpdPlan p = upd_plan_pack(st);
    const PlanView b = upd_plan_view(p);
    int bad = 0;
#define CMP(f) do { if (a.f != b.f) { std::printf("%s %ld: field %s differs: %d != %d\n", what, trial, #f, (int)a.f, (int)b.f); bad = 1; } } while (0)
    CMP(m_old); CMP(P_old); CMP(ev_finish); CMP(nS); CMP(ntgt); CMP(tU); CMP(tV); CMP(ix); CMP(ixn); CMP(iy); CMP(iyn);
    for (int i = 0; i < MAX_S; i++) CMP(S[i]);
    for (int i = 0; i < MAX_TGT; i++) { CMP(tdst[i]); CMP(tkind[i]); CMP(ta[i]); CMP(tb[i]); CMP(tc[i]); CMP(td[i]); }
#undef CMP
    if (p.event != st.n_events || p.u_id != st.cur.u_id) { std::printf("%s %ld: tag differs\n", what, trial); bad = 1; }
    cov.plans++;
    if (st.nS >= 0 && st.nS <= MAX_S) cov.nS[st.nS]++;
    if (st.ntgt >= 0 && st.ntgt <= MAX_TGT) cov.ntgt[st.ntgt]++;
    for (int i = 0; i < st.ntgt; i++) {
        cov.kind[st.tgt[i].kind]++;
        const int32_t ops[4] = {a.ta[i], a.tb[i], a.tc[i], a.td[i]};
        for (int k = 0; k < 4; k++) (ops[k] < 0 ? cov.op_absent : cov.op_present)++;
    }
    if (st.ev_finish) cov.finish++;
    else {
        (a.ixn < 0 ? cov.xn_absent : cov.xn_present)++;
        (a.iyn < 0 ? cov.yn_absent : cov.yn_present)++;
    }
    return bad;
}

static void add_op(State& st, int32_t kind, int32_t a, int32_t b, int32_t c, int32_t d, int32_t e, int32_t mcur) {
    Op& o = st.ops[st.nops++];
    o.kind = kind; o.a = a; o.b = b; o.c = c; o.d = d; o.e = e; o.mcur = mcur; o.flag = (int32_t)rnd(2);
}

// one event as decide_plan / finish_plan would plan it on a layout with P two-node clusters among m live nodes
static bool make_event(State& st) {
    std::memset(&st, 0, sizeof(st));
    for (int i = 0; i < MAX_S; i++) st.S[i] = (int32_t)rnd(1000);  // (stale: what an earlier event left)
    for (int i = 0; i < MAX_TGT; i++) { Tgt& t = st.tgt[i]; t.dst = (int32_t)rnd(64); t.kind = (int32_t)rnd(4); t.a = (int32_t)rnd(64) - 1; t.b = (int32_t)rnd(64) - 1; t.c = (int32_t)rnd(64) - 1; t.d = (int32_t)rnd(64) - 1; }
    st.n_events = (int64_t)rnd(1u << 30);
    st.cur.u_id = (int32_t)rnd(1u << 30);
    const bool finish = rnd(8) == 0;
    int32_t m = finish ? 4 : 5 + (int32_t)rnd(60), P = finish ? 2 : (int32_t)rnd((uint32_t)(m / 2 + 1));
    st.m_old = m; st.P_old = P; st.nops = 0;
    if (finish) {
        const int32_t ps = (int32_t)rnd(4), qs0 = (ps ^ 2) & 2, qs = qs0 + (int32_t)rnd(2);
        const int32_t Y = rnd(2) ? qs : (qs ^ 1), Z = Y ^ 1, k = qs >> 1;
        st.ev_finish = 1;
        st.xs = (int32_t)rnd(8) - 2; st.ys = (int32_t)rnd(8) - 2;  // (not set by the special finish: whatever was there)
        add_op(st, OP_AGG3, ps, Y, Z, 2 * k, 2 * k + 1, 4);
        st.m = m; st.P = P; st.U = 2 * k;
        cov.events[KIND_FINISH]++;
        return true;
    }
    int32_t x = (int32_t)rnd((uint32_t)m), y = (int32_t)rnd((uint32_t)m);
    const int32_t twoP = 2 * P;
    if (x == y || (x < twoP && y < twoP && (x >> 1) == (y >> 1))) return false;  // (one cluster: not a pair of clusters)
    const int32_t xn = x < twoP ? (x ^ 1) : -1, yn = y < twoP ? (y ^ 1) : -1;
    st.xs = x; st.ys = y;
    if (xn < 0 && yn < 0) {
        int32_t lo = rnd(2) ? x : y, hi = lo == x ? y : x;
        const int32_t t0 = twoP, t1 = twoP + 1;
        if (lo != t0) { add_op(st, OP_SWAP, lo, t0, 0, 0, 0, m); if (hi == t0) hi = lo; }
        if (hi != t1) add_op(st, OP_SWAP, hi, t1, 0, 0, 0, m);
        st.m = m; st.P = P + 1; st.U = t0;
        cov.events[KIND_2WAY]++;
    } else if (xn < 0 || yn < 0) {
        int32_t X, Y, Z;
        if (xn < 0) { X = x; Y = y; Z = yn; } else { X = y; Y = x; Z = xn; }
        const int32_t k = Y >> 1;
        add_op(st, OP_AGG3, X, Y, Z, 2 * k, 2 * k + 1, m);
        if (X != m - 1) add_op(st, OP_MOVE, m - 1, X, 0, 0, 0, m);
        st.m = m - 1; st.P = P; st.U = 2 * k;
        cov.events[KIND_3WAY]++;
    } else {
        const int32_t kx = x >> 1, ky = y >> 1;
        int32_t U = 2 * kx;
        const int32_t V = 2 * kx + 1;
        add_op(st, OP_AGG3, xn, x, y, U, V, m);
        add_op(st, OP_AGG3, U, V, yn, U, V, m - 1);
        const int32_t lastp = P - 1;
        if (ky != lastp) {
            add_op(st, OP_MOVE, 2 * lastp, 2 * ky, 0, 0, 0, m);
            add_op(st, OP_MOVE, 2 * lastp + 1, 2 * ky + 1, 0, 0, 0, m);
            if (kx == lastp) U = 2 * ky;
        }
        const int32_t h0 = 2 * lastp, h1 = 2 * lastp + 1, S = m - 2 * P;
        if (S >= 1) add_op(st, OP_MOVE, m - 1, h0, 0, 0, 0, m);
        if (S >= 2) add_op(st, OP_MOVE, m - 2, h1, 0, 0, 0, m);
        st.m = m - 2; st.P = P - 1; st.U = U;
        cov.events[KIND_4WAY]++;
    }
    return true;
}

// a plan drawn field by field: nS distinct slots, ntgt <= nS recipes on distinct rows of S
static void make_drawn(State& st, int nS, int ntgt) {
    std::memset(&st, 0, sizeof(st));
    st.n_events = (int64_t)rnd(1u << 30);
    st.cur.u_id = (int32_t)rnd(1u << 30);
    st.m_old = 20 + (int32_t)rnd(100);
    st.P_old = (int32_t)rnd((uint32_t)(st.m_old / 2 + 1));
    st.ev_finish = rnd(10) == 0 ? 1 : 0;
    st.nS = nS;
    for (int i = 0; i < MAX_S; i++) {  // distinct slots (entries beyond nS are stale but distinct as well)
        for (;;) {
            const int32_t s = (int32_t)rnd((uint32_t)st.m_old);
            bool dup = false;
            for (int j = 0; j < i; j++) dup = dup || st.S[j] == s;
            if (!dup) { st.S[i] = s; break; }
        }
    }
    auto pick_in = [&]() { return st.S[rnd((uint32_t)nS)]; };
    st.xs = pick_in();
    do { st.ys = pick_in(); } while (st.ys == st.xs);
    if (rnd(2) && nS >= 3) {  // x's partner among the involved slots, where x has one and a place is free
        for (int i = 0; i < nS; i++)
            if (st.S[i] != st.xs && st.S[i] != st.ys) {
                bool taken = false;
                for (int j = 0; j < MAX_S; j++) taken = taken || st.S[j] == (st.xs ^ 1);
                if (!taken) st.S[i] = st.xs ^ 1;
                break;
            }
    }
    st.ntgt = ntgt;
    for (int i = 0; i < MAX_TGT; i++) {
        Tgt& t = st.tgt[i];
        t.dst = i < ntgt ? st.S[i] : (int32_t)rnd((uint32_t)st.m_old);
        t.kind = (int32_t)rnd(4);
        auto operand = [&]() { return i < ntgt ? pick_in() : (int32_t)rnd((uint32_t)st.m_old + 1) - 1; };
        t.a = t.b = t.c = t.d = -1;
        if (t.kind == T_COPY) t.a = operand();
        else if (t.kind == T_L1) { t.a = operand(); t.b = operand(); }
        else if (t.kind == T_L2U) { t.a = operand(); t.b = operand(); t.c = operand(); }
        else { t.d = operand(); t.c = operand(); t.b = operand(); }
    }
    st.tU = ntgt > 0 ? (int32_t)rnd((uint32_t)ntgt + 1) - 1 : -1;
    st.tV = ntgt > 0 ? (int32_t)rnd((uint32_t)ntgt + 1) - 1 : -1;
}

int main() {
    static State st;
    int bad = 0;
    long made = 0;
    for (long trial = 0; trial < 6000; trial++) {
        if (!make_event(st)) continue;
        Dev d{};
        d.st = &st;
        build_targets(d);
        if (st.error) { std::printf("event %ld: build_targets reports %d\n", trial, st.error); return 1; }
        bad |= compare(st, "event", trial);
        made++;
    }
    for (int rep = 0; rep < 40; rep++)
        for (int nS = 2; nS <= MAX_S; nS++)
            for (int ntgt = 0; ntgt <= nS; ntgt++) {
                make_drawn(st, nS, ntgt);
                bad |= compare(st, "drawn", (long)rep * 100 + nS * 10 + ntgt);
            }
    bool full = cov.finish > 0 && cov.xn_absent > 0 && cov.xn_present > 0 && cov.yn_absent > 0 && cov.yn_present > 0 &&
                cov.op_absent > 0 && cov.op_present > 0;
    for (int k = KIND_2WAY; k <= KIND_FINISH; k++) full = full && cov.events[k] > 0;
    for (int i = 2; i <= MAX_S; i++) full = full && cov.nS[i] > 0;
    for (int i = 0; i <= MAX_TGT; i++) full = full && cov.ntgt[i] > 0;
    for (int k = 0; k < 4; k++) full = full && cov.kind[k] > 0;
    if (!full) { std::printf("coverage incomplete\n"); return 1; }
    if (bad) return 1;
    std::printf("ok: %ld plans (%ld replayed events: %ld / %ld / %ld / %ld of agg2way / agg3way / agg4way / finish)\n", cov.plans, made,
                cov.events[KIND_2WAY], cov.events[KIND_3WAY], cov.events[KIND_4WAY], cov.events[KIND_FINISH]);
    return 0;
}

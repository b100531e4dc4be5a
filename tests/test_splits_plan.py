"""The host arithmetic of the one-problem split-weight solver's block method (fastneighbornet_amd/csrc/fnn_splits_plan.h) on the
CPU: the capacity plan of the factor, the host part of Lawson & Hanson's ratio step, the compaction of a rebuild, the lists of a
revival and the objective - each against a plain Python restatement of the rule, exactly (integers and doubles by value, NaN by
position).

tests/emu/fnn_splits_plan_main.cpp is a program of its own over that header: it reads the cases, prints what the header's
functions give and holds no expectation.  It is built twice: plainly, and with -fsanitize=address,undefined (run directly:
nothing is loaded into the interpreter).

The panel storage the plan sizes: panel q of width pw starts at off(q) = pw (q cap - pw q (q - 1) / 2) doubles (TriStore in
fnn_splits.hip) and holds min(pw, cap - q pw) columns of cap - q pw rows.  The panels tile the capacity, every panel starts where
the one before it ends, and the last one ends at tri_elems(cap, pw).  (off() of the panel AFTER the last one equals tri_elems
only where pw divides cap: a narrower last panel has fewer columns than off()'s stride assumes.)"""
import math
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
SRCS = [os.path.join(EMU_DIR, "fnn_splits_plan_main.cpp"), os.path.join(ROOT, "fastneighbornet_amd", "csrc", "fnn_splits_plan.h")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g", "-O1"]
NAN = float("nan")
AMPLE = 1e15


def build(name, flags):
    exe = os.path.join(EMU_DIR, "build", name)
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in SRCS):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall"] + flags + ["-o", exe, SRCS[0]])
    return exe


@pytest.fixture(scope="module", params=[("fnn_splits_plan_main", ["-O2"]), ("fnn_splits_plan_main_asan", SAN)], ids=["plain", "asan_ubsan"])
def program(request):
    exe = build(*request.param)

    def run(lines):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        out = r.stdout.splitlines()
        assert out[-1] == f"ok: {len(lines)} cases", out[-1]
        return [parse(x) for x in out[:-1]]
    return run


def fmt(v):
    return "nan" if v != v else float(v).hex()


def parse(line):
    """'kind key v ... key v ...' -> {key: [values]} (the keys are the words that are not numbers)."""
    out, key = {}, None
    for t in line.split()[1:]:
        try:
            v = float.fromhex(t) if ("x" in t or "nan" in t or "inf" in t) else int(t)
        except ValueError:
            key = t
            out[key] = []
            continue
        out[key].append(v)
    return out


def same(a, b):
    """By value, NaN equal to NaN at the same position."""
    return len(a) == len(b) and all((x != x and y != y) or x == y for x, y in zip(a, b))


# ---- the capacity plan -------------------------------------------------------------------------------------------------------

def up64(v):
    return (v + 63) // 64 * 64


def elems(cap, pw):
    return sum(min(pw, cap - q0) * (cap - q0) for q0 in range(0, cap, pw))


SHAPES = [(6.0, 12, 5), (5.0, 12, 5), (4.5, 12, 5), (4.0, 12, 5), (4.0, 16, 8), (3.5, 12, 5), (3.25, 12, 5)]
TRIES = [(0.0, 12, 5), (0.0, 16, 8), (0.0, 24, 12)]


def plan_rule(n, budget, cap_want, panel, capknob):
    """The shape table, restated: the first shape {capacity / n, block = capacity / kdiv, departed = capacity / rdiv} whose buffers
    fit the budget, the last one if none does; FNN_SW_CAP takes the first shape's side buffers at its own capacity / n; a retry
    (cap_want > 0) takes the wanted capacity with the roomiest of three side-buffer shapes that fits, shrinking the wanted capacity
    by a tenth up to 40 times."""
    N = n * (n - 1) // 2
    p = {}

    def sized(factor, kdiv, rdiv, want):
        cap = up64(min(N, max(int(factor * n) + 1024, min(8 * n + 64, 20000), 512)))
        if want > 0:
            cap = up64(min(N, want))
        kmax = min(cap, max(64, up64(cap // kdiv)), 8192)
        rcap = min(cap, up64(cap // rdiv) + 64)
        pw = max(1024, up64(cap // 8))
        if panel >= 64:
            pw = up64(panel)
        m = max(rcap, kmax)
        p.update(cap=cap, kmax=kmax, rcap=rcap, pw=pw)
        return 8.0 * (float(elems(cap, pw)) + 3.0 * cap * kmax + float(cap) * rcap + 4.0 * rcap * rcap + 3.0 * kmax * kmax + 0.5 * m * m) + \
            64.0 * cap + 48.0 * max(1 << 16, N // 16 + 1024)

    pick, fits = SHAPES[6], False
    if cap_want > 0:
        for _ in range(40):
            for sh in TRIES:
                pick = sh
                p["bytes"] = sized(0.0, sh[1], sh[2], cap_want)
                if p["bytes"] <= budget:
                    fits = True
                    break
            if fits:
                break
            cap_want = int(0.9 * cap_want)
        p.update(f=pick[0], kdiv=pick[1], rdiv=pick[2], fits=int(fits), cap_want=cap_want)
        if not fits:
            return p
    else:
        for sh in SHAPES:
            pick = sh
            if capknob > 0.0:
                pick = (capknob, sh[1], sh[2])
                break
            if sized(*sh, 0) <= budget:
                break
    p["bytes"] = sized(*pick, cap_want)
    p.update(f=pick[0], kdiv=pick[1], rdiv=pick[2], fits=int(p["bytes"] <= budget), cap_want=cap_want)
    return p


def plan_line(n, budget, cap_want=0, panel=0, capknob=0.0):
    return f"plan {n} {fmt(budget)} {cap_want} {panel} {fmt(capknob)}"


def check_tiling(cap, pw, total):
    off = lambda q: pw * (q * cap - pw * (q * (q - 1) // 2))
    end, cols = 0, 0
    for q in range((cap + pw - 1) // pw):
        assert off(q) == end, (cap, pw, q)
        w, ld = min(pw, cap - q * pw), cap - q * pw
        end += w * ld
        cols += w
    assert cols == cap and end == total == elems(cap, pw), (cap, pw, end, total)


def test_capacity_plan_grid(program):
    cases = []
    for n in (2, 3, 64, 1024, 4096, 16384, 32768):
        default_cap = plan_rule(n, AMPLE, 0, 0, 0.0)["cap"]
        for budget in (1e8, 1e9, 1e10, 5e10, 0.92 * 100e9, 0.92 * 150e9, 2e11, 0.92 * 250e9, 0.92 * 270e9, 2.5e11, AMPLE):
            for cap_want in (0, 4 * default_cap):
                for panel in (0, 64):
                    cases.append((n, budget, cap_want, panel, 0.0))
        cases += [(n, 1e11, 0, 0, 2.0), (n, 1e8, 0, 0, 0.05), (n, 1e8, 1, 0, 0.0), (n, 1e8, 7, 64, 0.0)]
    got = program([plan_line(*c) for c in cases])
    unfit = 0
    for c, g in zip(cases, got):
        want = plan_rule(*c)
        for k, v in want.items():
            assert same(g[k], [v]), (c, k, g[k], v)
        assert g["elems"] == [elems(want["cap"], want["pw"])], (c, g)
        check_tiling(want["cap"], want["pw"], g["elems"][0])
        unfit += 1 - want["fits"]
    assert 0 < unfit < len(cases)       # both outcomes occur


def test_capacity_plan_anchors(program):
    """The shapes a solve picks today, derived from the shape table by hand.  Budget = 0.92 x the free memory."""
    rows = [  # n, free memory, cap_want -> cap, kmax, rcap, pw, fits
        (64, AMPLE, 0, 1408, 128, 384, 1024, 1), (1024, AMPLE, 0, 8256, 704, 1728, 1088, 1), (4096, AMPLE, 0, 25600, 2176, 5184, 3200, 1),
        (16384, 250e9, 0, 99328, 8192, 19968, 12416, 1),
        (32768, 270e9, 0, 164864, 8192, 33088, 20608, 1),      # shape 5.0 n
        (32768, 150e9, 0, 132096, 8192, 16576, 16512, 1),      # shape {4.0, 16, 8}
        (32768, 100e9, 0, 107520, 8192, 21568, 13440, 0),      # the last shape, and it does not fit: the plan still returns it (the
                                                               # allocation then fails and the solve ends as FNN_SW_GIVEUP_SETUP)
        (1024, AMPLE, 33024, 33024, 2752, 6720, 4160, 1)]      # the retry
    got = program([plan_line(n, 0.92 * free, cap_want) for n, free, cap_want, *_ in rows])
    for (n, free, cap_want, cap, kmax, rcap, pw, fits), g in zip(rows, got):
        assert (g["cap"], g["kmax"], g["rcap"], g["pw"], g["fits"]) == ([cap], [kmax], [rcap], [pw], [fits]), (n, free, g)
    assert got[4]["f"] == [5.0] and (got[5]["f"], got[5]["kdiv"], got[5]["rdiv"]) == ([4.0], [16], [8]) and got[6]["f"] == [3.25]


# ---- the ratio step ----------------------------------------------------------------------------------------------------------

def ratio_rule(x, s, dead):
    """alpha = the smallest x / (x - s) over the members whose s is not positive (a NaN s is not positive; a NaN quotient does
    not lower alpha), 2 if there is none; above 1 nothing moves.  Else x += alpha (s - x); a member whose quotient is not above
    alpha (0 / 0 is not) is at zero exactly; it and every member with s not positive that does not stay positive leave."""
    x = list(x)
    alpha = 2.0
    for p in range(len(s)):
        if not dead[p] and not s[p] > 0.0:
            q = div(x[p], x[p] - s[p])
            if q < alpha:
                alpha = q
    out = []
    if alpha > 1.0:
        return alpha, x, out
    for p in range(len(s)):
        if dead[p]:
            continue
        neg = not s[p] > 0.0
        hit = neg and not div(x[p], x[p] - s[p]) > alpha
        x[p] = 0.0 if hit else x[p] + alpha * (s[p] - x[p])
        if hit or (neg and not x[p] > 0.0):
            out.append(p)
    return alpha, x, out


def div(a, b):
    if b == 0.0:                       # (IEEE division: Python raises where C++ gives a NaN or an infinity)
        return NAN if (a != a or a == 0.0) else math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def ratio_line(x, s, dead):
    return " ".join(["ratio", str(len(x))] + [fmt(v) for v in list(x) + list(s)] + [str(int(d)) for d in dead])


def test_ratio_step(program):
    rng = random.Random(15)
    cases = [
        ([1.0, 2.0, 3.0], [0.5, 2.5, 1.0], [0, 0, 0]),             # no member with s <= 0: alpha = 2, nothing leaves
        ([1.0, 2.0, 3.0], [0.5, -2.0, 1.0], [0, 0, 0]),            # one hit
        ([1.0, 2.0, 3.0, 4.0], [-1.0, -2.0, 1.0, 5.0], [0, 0, 0, 0]),  # two members reach zero in the same step: an exact tie (alpha = 1/2)
        ([0.0, 2.0, 3.0], [0.0, -2.0, 4.0], [0, 0, 0]),            # x = 0 and s = 0 beside a hit: 0 / 0 counts as a hit too
        ([0.0, 2.0, 3.0], [0.0, 1.0, 4.0], [0, 0, 0]),             # ... but alone it does not lower alpha: nothing moves
        ([0.0, 2.0, 3.0], [-1.0, 1.0, 4.0], [0, 0, 0]),            # x = 0 with s < 0: alpha = 0
        ([1.0, 2.0, 3.0], [0.5, NAN, 1.0], [0, 0, 0]),             # a NaN in s: not positive, its quotient is no number
        ([1.0, 2.0, 3.0], [NAN, -2.0, 1.0], [0, 0, 0]),
        ([1.0, 0.0, 3.0, 0.0], [0.5, -7.0, -1.0, NAN], [0, 1, 0, 1]),  # dead members are ignored
        ([0.0, 0.0], [-1.0, -2.0], [1, 1]),                        # all dead
        ([1.0], [1.0 - 2.0 ** -52], [0]), ([1.0], [-0.0], [0]), ([2.0 ** -1074], [-1.0], [0]),
    ]
    for _ in range(60):
        m = rng.randint(1, 200)
        x = [rng.choice([0.0, rng.random(), rng.random() * 1e6]) for _ in range(m)]
        s = [rng.choice([v, v, rng.uniform(-1.0, 1.0), -v, 0.0]) for v in x]
        dead = [int(rng.random() < 0.2) for _ in range(m)]
        x = [0.0 if d else v for v, d in zip(x, dead)]
        cases.append((x, s, dead))
    got = program([ratio_line(*c) for c in cases])
    moved = 0
    for c, g in zip(cases, got):
        alpha, x, out = ratio_rule(*c)
        assert same(g["alpha"], [alpha]) and same(g["x"], x) and g["out"] == out, (c, g, alpha, x, out)
        moved += alpha <= 1.0
    assert got[0]["alpha"] == [2.0] and got[0]["out"] == [] and got[1]["out"] == [1] and got[2]["out"] == [0, 1] and got[2]["alpha"] == [0.5]
    assert got[3]["out"] == [0, 1] and got[3]["alpha"] == [0.5] and got[4]["alpha"] == [2.0] and got[4]["out"] == []
    assert got[8]["out"] == [2] and 10 < moved < len(cases)


# ---- compaction, revival lists, objective ------------------------------------------------------------------------------------

def compact_line(F, xw, cF, dead, deadlist):
    return " ".join(["compact", str(len(F))] + [str(a) for a, _ in F] + [str(b) for _, b in F] + [fmt(v) for v in xw + cF] +
                    [str(d) for d in dead] + [str(len(deadlist))] + [str(p) for p in deadlist])


def revive_line(rev, dead, deadlist):
    return " ".join(["revive", str(len(dead)), str(len(deadlist)), str(len(rev))] + [str(v) for v in rev + dead + deadlist])


def factor_state(rng, m, kind):
    F = [(i, i + 1 + rng.randint(0, 5)) for i in range(m)]
    xw, cF = [rng.random() for _ in range(m)], [rng.uniform(-1.0, 1.0) for _ in range(m)]
    dead = {"none": [0] * m, "all": [1] * m, "ends": [int(p in (0, m - 1)) for p in range(m)],
            "random": [int(rng.random() < 0.3) for _ in range(m)]}[kind]
    deadlist = [p for p in range(m) if dead[p]]
    rng.shuffle(deadlist)                       # (the order of Y's columns is the order of departure)
    return F, [0.0 if d else v for v, d in zip(xw, dead)], cF, dead, deadlist


def test_compaction_revival_lists_and_objective(program):
    rng = random.Random(16)
    states = [factor_state(rng, m, kind) for m in (1, 2, 7, 200) for kind in ("none", "all", "ends", "random")]
    lines, want = [], []
    for F, xw, cF, dead, deadlist in states:
        live = [p for p in range(len(F)) if not dead[p]]
        lines.append(compact_line(F, xw, cF, dead, deadlist))     # a rebuild keeps the splits that are in, in order
        want.append({"Fi": [F[p][0] for p in live], "Fj": [F[p][1] for p in live], "gonei": [F[p][0] for p in range(len(F)) if dead[p]],
                     "gonej": [F[p][1] for p in range(len(F)) if dead[p]], "dead": [0] * len(live), "deadlist": [],
                     "xw": [xw[p] for p in live], "cF": [cF[p] for p in live]})
        for share in (0.0, 0.5, 1.0):                              # a revival brings back none, some, all of the departed
            rev = sorted(p for p in deadlist if rng.random() < share) if share < 1.0 else sorted(deadlist)
            lines.append(revive_line(rev, dead, deadlist))
            keep = [q for q, p in enumerate(deadlist) if p not in rev]
            want.append({"keepcols": keep, "newdead": [deadlist[q] for q in keep], "dead": [int(d and p not in rev) for p, d in enumerate(dead)]})
        xs = [rng.choice([v, NAN if rng.random() < 0.02 else -v]) for v in xw]
        lines.append(" ".join(["objective", str(len(F))] + [fmt(v) for v in xs + cF] + [str(d) for d in dead]))
        acc = 0.0
        for p in live:
            acc += cF[p] * xs[p]
        want.append({"phi": [-0.5 * acc]})
    for line, w, g in zip(lines, want, program(lines)):
        assert set(w) == set(g), (line, g)
        for k in w:
            assert same(g[k], w[k]), (line, k, g[k], w[k])

"""Phase bodies of the batched circular split weights (fnn_small_splits.h) on crafted free sets, on the CPU: the ratio step
with its compaction (splits_ratio_min, splits_fold_ratio, splits_ratio_step, splits_compact) and the append step's two arms
(splits_append_row), against a plain Python restatement of each rule.

Why at phase level.  No whole problem reaches these paths, with or without the test switches of
tests/splits_batch_common.py, and for three of them that is a property of the method, not of the inputs tried:
  * a split that leaves in the step in which it entered: at every pick x is the least-squares optimum on F, so the
    sub-problem's solution of the entering split has the sign of its multiplier, which is positive (Lawson & Hanson's
    lemma); only rounding can turn it, and the splits of one circular ordering are linearly independent and mildly
    conditioned (up to 20 taxa no problem of tests/inputs.py ever met delta^2 / H_kk below 2e-2);
  * a split set aside as dependent while the factor is REBUILT: the rebuilt factor conditions on a subset of the members
    the split passed against when it entered, and a Schur complement does not shrink when conditioning members go;
  * two members reaching zero in one ratio step, a member at x = 0 with s <= 0, a NaN in s: these need exact ties or a
    broken factor; the classes with ties (dup, dec4, integer matrices) never produced one.
The bodies are the source the kernel compiles; these cases stay CPU-only.

tests/emu/fnn_splits_phase_main.cpp is a program of its own over the CPU driver's phase-level entries: it reads the crafted
states, prints what the phase bodies leave and holds no expectation.  It is built twice: plainly, and with
-fsanitize=address,undefined (run directly: nothing is loaded into the interpreter); the view it runs on is carved from
heap blocks of exactly the kernel's LDS and workspace sizes."""
import math
import os
import subprocess

import numpy as np
import pytest

import splits_batch_common as sc

SRCS = [os.path.join(sc.EMU_DIR, "fnn_splits_phase_main.cpp")] + sc.EMU_SRCS
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g", "-O1"]
ACT_APPEND, ACT_GIVEUP = 0, 3
NAN = float("nan")


def build(name, flags):
    exe = os.path.join(sc.EMU_DIR, "build", name)
    if sc.newer(exe, SRCS):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas"] + flags + ["-o", exe, SRCS[0], SRCS[1]])
    return exe


@pytest.fixture(scope="module", params=[("fnn_splits_phase_main", ["-O2"]), ("fnn_splits_phase_main_asan", SAN)], ids=["plain", "asan_ubsan"])
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
    """Bit for bit, NaN equal to NaN."""
    return len(a) == len(b) and all((x != x and y != y) or (x == y and math.copysign(1, x) == math.copysign(1, y)) for x, y in zip(a, b))


def gx0(k):
    return 1.0 + k                # the program's initial grid of weights


# ---- the ratio step and the compaction -----------------------------------------------------------------------------------

def ratio_case(n, threads, Fi, x, s, c, enter_pos=-1, departed=0, n_aside=0, steps=0, max_steps=1000):
    line = " ".join(["ratio", str(n), str(threads), str(len(Fi)), str(enter_pos), str(departed), str(n_aside), str(steps), str(max_steps)] +
                    [str(k) for k in Fi] + [fmt(v) for v in list(x) + list(s) + list(c)])
    return line, ratio_rule(Fi, x, s, c, enter_pos, departed, n_aside, steps, max_steps)


def ratio_rule(Fi, x, s, c, enter_pos, departed, n_aside, steps, max_steps):
    """Lawson-Hanson's ratio step, restated: among the members whose sub-problem solution is not positive the smallest
    x / (x - s) (0 where x is not positive or the quotient is no number; ties: the lowest position) is alpha and that member
    leaves; x += alpha (s - x); whatever does not stay positive leaves with it.  The members that stay close ranks in
    order; the factor is valid up to the first position that left; a member that leaves in the step in which it entered is
    set aside (mask 2), the others may enter again (mask 0); the entering position follows its member."""
    f = len(Fi)
    best = None
    for j in range(f):
        if s[j] > 0.0:
            continue
        ratio = x[j] / (x[j] - s[j]) if x[j] > 0.0 else 0.0
        if not ratio >= 0.0:
            ratio = 0.0
        if best is None or ratio < best[0]:
            best = (ratio, j)
    exp = {"Fi": list(Fi), "xF": list(x), "cF": list(c), "gx": [gx0(k) for k in Fi], "mask": [1] * f, "f": [f], "ftot": [f],
           "enter_pos": [enter_pos], "departed": [departed], "n_aside": [n_aside], "aside_enter": [0], "steps": [steps], "action": [ACT_APPEND]}
    if best is None:
        exp.update(leave=[-1], alpha=[1.0])
        return exp
    alpha, leave = best
    exp.update(leave=[leave], alpha=[alpha], steps=[steps + 1])
    if steps + 1 > max_steps:
        exp["action"] = [ACT_GIVEUP]
        return exp
    xn = []
    for j in range(f):
        v = x[j] + alpha * (s[j] - x[j])
        xn.append(0.0 if j == leave or not v > 0.0 else v)
    stay = [j for j in range(f) if xn[j] > 0.0]
    gone = [j for j in range(f) if not xn[j] > 0.0]
    exp.update(Fi=[Fi[j] for j in stay], xF=[xn[j] for j in stay], cF=[c[j] for j in stay], f=[gone[0]], ftot=[len(stay)],
               departed=[departed + len(gone)], enter_pos=[stay.index(enter_pos) if enter_pos in stay else -1],
               gx=[gx0(Fi[j]) if j in stay else 0.0 for j in range(f)],
               mask=[1 if j in stay else (2 if j == enter_pos else 0) for j in range(f)])
    if enter_pos in gone:
        exp.update(n_aside=[n_aside + 1], aside_enter=[1])
    return exp


def assert_state(got, exp, tag):
    for k, v in exp.items():
        assert same(got[k], v), (tag, k, got[k], v)


FI6 = [1, 2, 11, 20, 29, 38]      # splits (0,1) (0,2) (1,3) (2,4) (3,5) (4,6) of 8 taxa: grid index i * 8 + j
C6 = [0.5, -1.5, 2.5, 3.5, -4.5, 5.5]


def crafted_ratio_cases():
    X = [4.0, 2.0, 3.0, 1.0, 5.0, 6.0]
    tied = [9.0, -2.0, 7.0, -1.0, 8.0, 10.0]                 # positions 1 and 3: ratio 1/2 both, both reach zero
    out = []
    for ep in (-1, 0, 1, 2, 3, 4, 5):                        # the entering position: none, in front of, among, between, behind the leavers
        out.append((("two leave, tied", ep), ratio_case(8, 256, FI6, X, tied, C6, enter_pos=ep, departed=3, n_aside=2)))
    for threads in (1, 64, 1024):
        out.append((("two leave, threads", threads), ratio_case(8, threads, FI6, X, tied, C6, enter_pos=5)))
    for ep in (2, 5, -1):                                    # a member at x = 0 with s < 0 and with s = 0: ratio 0, nothing else moves
        out.append((("x = 0, s < 0", ep), ratio_case(8, 256, FI6, [4.0, 2.0, 0.0, 1.0, 5.0, 6.0], [9.0, 1.0, -1.0, 3.0, 8.0, 10.0], C6, enter_pos=ep)))
        out.append((("x = 0, s = 0", ep), ratio_case(8, 256, FI6, [4.0, 2.0, 0.0, 1.0, 5.0, 6.0], [9.0, 1.0, 0.0, 3.0, 8.0, 10.0], C6, enter_pos=ep)))
        out.append((("x = 0, s = -0", ep), ratio_case(8, 256, FI6, [4.0, 2.0, 0.0, 1.0, 5.0, 6.0], [9.0, 1.0, -0.0, 3.0, 8.0, 10.0], C6, enter_pos=ep)))
    out.append((("two at x = 0", 0), ratio_case(8, 256, FI6, [4.0, 0.0, 3.0, 1.0, 0.0, 6.0], [9.0, -1.0, 7.0, 3.0, -2.0, 10.0], C6, enter_pos=4)))
    out.append((("x < 0", 0), ratio_case(8, 256, FI6, [4.0, 2.0, 3.0, -1.0, 5.0, 6.0], [9.0, 1.0, 7.0, -3.0, 8.0, 10.0], C6, enter_pos=5)))
    for ep in (4, 5, 0):                                     # a NaN in s: ratio 0, that member leaves, the others keep their weight
        out.append((("NaN in s", ep), ratio_case(8, 256, FI6, X, [9.0, 1.0, 7.0, 3.0, NAN, 10.0], C6, enter_pos=ep)))
    out.append((("NaN in s and a leaver", 0), ratio_case(8, 256, FI6, X, [9.0, -2.0, 7.0, 3.0, NAN, 10.0], C6, enter_pos=5)))
    out.append((("NaN in x", 0), ratio_case(8, 256, FI6, [4.0, 2.0, NAN, 1.0, 5.0, 6.0], [9.0, 1.0, -7.0, 3.0, 8.0, 10.0], C6, enter_pos=5)))
    out.append((("x = s = inf", 0), ratio_case(8, 256, FI6, [4.0, 2.0, math.inf, 1.0, 5.0, 6.0], [9.0, 1.0, -math.inf, 3.0, 8.0, 10.0], C6, enter_pos=5)))
    out.append((("none leaves", 0), ratio_case(8, 256, FI6, X, [9.0, 1.0, 7.0, 3.0, 8.0, 10.0], C6, enter_pos=5, steps=1000, max_steps=1000)))
    out.append((("one leaves, first", 0), ratio_case(8, 256, FI6, X, [-4.0, 1.0, 7.0, 3.0, 8.0, 10.0], C6, enter_pos=5)))
    out.append((("one leaves, last", 0), ratio_case(8, 256, FI6, X, [9.0, 1.0, 7.0, 3.0, 8.0, -6.0], C6, enter_pos=5)))
    out.append((("all leave", 0), ratio_case(8, 256, FI6, X, [-4.0, -2.0, -3.0, -1.0, -5.0, -6.0], C6, enter_pos=5)))
    for steps, mx in ((998, 1000), (999, 1000), (1000, 1000), (0, 1), (1, 1)):   # the step limit counts ratio steps: steps + 1 > limit gives up
        out.append((("step limit", steps, mx), ratio_case(8, 256, FI6, X, tied, C6, enter_pos=5, steps=steps, max_steps=mx)))
    return out


def drawn_ratio_cases(count=300):
    """Free sets of 1 to 96 members of 16 taxa (two waves of candidates under 128 threads) with values from a few small
    integers, so that ties, zeros and several departures are the rule, and now and then a NaN."""
    rng = np.random.default_rng(2024)
    n, out = 16, []
    pairs = [i * n + j for i in range(n) for j in range(i + 1, n)]
    for t in range(count):
        f = int(rng.integers(1, 97))
        Fi = [int(k) for k in rng.choice(pairs, f, replace=False)]
        x = [float(v) for v in rng.choice([0.0, 1.0, 2.0, 3.0, 0.5], f, p=[0.1, 0.3, 0.3, 0.2, 0.1])]
        s = [float(v) for v in rng.choice([-2.0, -1.0, -0.5, 0.0, 1.0, 2.0, 4.0], f, p=[0.05, 0.05, 0.03, 0.02, 0.35, 0.3, 0.2])]
        if t % 7 == 0:
            s[int(rng.integers(f))] = NAN
        c = [float(v) for v in rng.standard_normal(f)]
        ep = int(rng.integers(-1, f))
        out.append((("drawn", t), ratio_case(n, int(rng.choice([64, 128, 512])), Fi, x, s, c, enter_pos=ep, departed=int(rng.integers(5)),
                                              n_aside=int(rng.integers(3)), steps=int(rng.integers(10)))))
    return out


def test_ratio_step_and_compaction(program):
    cases = crafted_ratio_cases() + drawn_ratio_cases()
    got = program([line for _, (line, _) in cases])
    seen = {"two": 0, "enter_left": 0, "enter_moved": 0, "ratio0": 0, "giveup": 0, "none": 0}
    for (tag, (_, exp)), g in zip(cases, got):
        assert_state(g, exp, tag)
        seen["two"] += exp["mask"].count(0) + exp["mask"].count(2) >= 2
        seen["enter_left"] += exp["aside_enter"][0]
        seen["ratio0"] += exp["leave"][0] >= 0 and exp["alpha"][0] == 0.0
        seen["giveup"] += exp["action"][0] == ACT_GIVEUP
        seen["none"] += exp["leave"][0] < 0
    # the crafted list alone pins each rule; the counts say that the drawn ones met them many times more
    assert seen["two"] >= 50 and seen["enter_left"] >= 10 and seen["ratio0"] >= 20 and seen["giveup"] >= 2 and seen["none"] >= 2, seen


def test_crafted_cases_say_what_the_issue_lists():
    """The restated rule on the named cases, spelled out, so that a slip in the restatement itself cannot pass both sides."""
    by = {tag: exp for tag, (_, exp) in crafted_ratio_cases()}
    e = by[("two leave, tied", 5)]        # behind both leavers: position 5 becomes 3
    assert e["leave"] == [1] and e["alpha"] == [0.5] and e["f"] == [1] and e["ftot"] == [4] and e["enter_pos"] == [3] and e["departed"] == [5]
    assert e["Fi"] == [1, 11, 29, 38] and e["xF"] == [6.5, 5.0, 6.5, 8.0] and e["mask"] == [1, 0, 1, 0, 1, 1] and e["n_aside"] == [2]
    e = by[("two leave, tied", 3)]        # among the leavers: set aside
    assert e["enter_pos"] == [-1] and e["mask"] == [1, 0, 1, 2, 1, 1] and e["n_aside"] == [3] and e["aside_enter"] == [1]
    assert by[("two leave, tied", 2)]["enter_pos"] == [1] and by[("two leave, tied", 0)]["enter_pos"] == [0]
    e = by[("x = 0, s < 0", 2)]
    assert e["leave"] == [2] and e["alpha"] == [0.0] and e["xF"] == [4.0, 2.0, 1.0, 5.0, 6.0] and e["mask"] == [1, 1, 2, 1, 1, 1]
    e = by[("NaN in s", 5)]
    assert e["leave"] == [4] and e["alpha"] == [0.0] and e["xF"] == [4.0, 2.0, 3.0, 1.0, 6.0] and e["enter_pos"] == [4]
    assert by[("step limit", 1000, 1000)]["action"] == [ACT_GIVEUP] and by[("step limit", 999, 1000)]["action"] == [ACT_APPEND]


# ---- the append step's two arms ----------------------------------------------------------------------------------------------

def append_case(n, threads, r, Fi, x, c, rv, fresh, dep, hkk, ll, lz, enter_pos, departed=0, n_aside=0, entered=0, peak=0):
    ftot = len(Fi)
    line = " ".join(["append", str(n), str(threads), str(r), str(ftot), str(fresh), fmt(dep), fmt(hkk), fmt(ll), fmt(lz), str(enter_pos), str(departed),
                     str(n_aside), str(entered), str(peak)] + [str(k) for k in Fi] + [fmt(v) for v in list(x) + list(c) + list(rv)])
    return line, append_rule(r, Fi, x, c, rv, fresh, dep, hkk, ll, lz, enter_pos, departed, n_aside, entered, peak)


def append_rule(r, Fi, x, c, rv, fresh, dep, hkk, ll, lz, enter_pos, departed, n_aside, entered, peak):
    """Appending position r to the inverse Cholesky factor, restated: with delta^2 = H_kk - l.l above dep * H_kk the row is
    [-(l^T W) / delta, 1 / delta], z_r = (c_r - l.z) / delta and the split is a member (mask 1); otherwise it is set aside
    (mask 2, weight 0) and leaves F: the positions behind it move down, the entering position with them; on a rebuild it
    counts as departed."""
    ftot = len(Fi)
    exp = {"Fi": list(Fi), "xF": list(x), "cF": list(c), "gx": [gx0(k) for k in Fi], "mask": [0 if j == r else 1 for j in range(ftot)],
           "f": [r], "ftot": [ftot], "enter_pos": [enter_pos], "departed": [departed], "n_aside": [n_aside], "entered": [entered], "peak": [peak],
           "aside_fresh": [0], "aside_rebuild": [0], "w": [-7.0] * (r + 1), "z": [-7.0]}
    d2 = hkk - ll
    if d2 > dep * hkk:
        dl = math.sqrt(d2)
        exp.update(w=[-v / dl for v in rv] + [1.0 / dl], z=[(c[r] - lz) / dl], f=[r + 1], entered=[entered + (1 if fresh else 0)], peak=[max(peak, r + 1)])
        exp["mask"][r] = 1
        return exp
    keep = [j for j in range(ftot) if j != r]
    exp.update(Fi=[Fi[j] for j in keep], xF=[x[j] for j in keep], cF=[c[j] for j in keep], ftot=[ftot - 1], n_aside=[n_aside + 1],
               enter_pos=[-1 if enter_pos == r else (enter_pos - 1 if enter_pos > r else enter_pos)])
    exp["gx"][r] = 0.0
    exp["mask"][r] = 2
    exp.update(aside_fresh=[1]) if fresh else exp.update(aside_rebuild=[1], departed=[departed + 1])
    return exp


def test_append_row_both_arms(program):
    X = [4.0, 2.0, 3.0, 1.5, 5.0, 6.0]
    RV = [0.25, -0.5, 0.75]
    cases = []
    for fresh in (0, 1):
        for ep in (-1, 1, 3, 4, 5):           # the entering position: none, in front of r = 3, r itself, behind it, last
            # delta^2 = 0.1 of H_kk = 12: dependent at 0.02, not at 1e-9
            cases.append((("aside", fresh, ep), append_case(8, 256, 3, FI6, X, C6, RV, fresh, 0.02, 12.0, 11.9, 0.5, ep, departed=2, n_aside=1, entered=7, peak=5)))
            cases.append((("enters", fresh, ep), append_case(8, 256, 3, FI6, X, C6, RV, fresh, 1e-9, 12.0, 11.9, 0.5, ep, departed=2, n_aside=1, entered=7, peak=3)))
    for threads in (1, 64, 1024):
        cases.append((("aside, threads", threads), append_case(8, threads, 3, FI6, X, C6, RV, 0, 0.02, 12.0, 11.9, 0.5, 5)))
        cases.append((("enters, threads", threads), append_case(8, threads, 3, FI6, X, C6, RV, 0, 1e-9, 12.0, 11.9, 0.5, 5)))
    # the boundary: delta^2 == dep * H_kk is dependent (all three are exact in binary), one ulp more is not
    cases.append((("boundary, equal", 0), append_case(8, 256, 3, FI6, X, C6, RV, 1, 2.0 ** -6, 16.0, 15.75, 0.5, 3)))
    cases.append((("boundary, above", 0), append_case(8, 256, 3, FI6, X, C6, RV, 1, 2.0 ** -6, 16.0, math.nextafter(15.75, 0.0), 0.5, 3)))
    cases.append((("negative delta^2", 0), append_case(8, 256, 3, FI6, X, C6, RV, 0, 1e-9, 12.0, 12.5, 0.5, 4)))
    cases.append((("NaN delta^2", 0), append_case(8, 256, 3, FI6, X, C6, RV, 0, 1e-9, 12.0, NAN, 0.5, 4)))
    cases.append((("first position", 0), append_case(8, 256, 0, FI6, X, C6, [], 1, 0.02, 7.0, 0.0, 0.0, 0)))              # the empty factor: always enters
    cases.append((("first position aside", 0), append_case(8, 256, 0, FI6, X, C6, [], 0, 0.02, 7.0, 6.99, 0.0, 2)))
    cases.append((("last position aside", 0), append_case(8, 256, 5, FI6, X, C6, RV + [1.0, -2.0], 0, 0.02, 12.0, 11.9, 0.5, 5)))
    cases.append((("only member aside", 0), append_case(8, 256, 0, FI6[:1], X[:1], C6[:1], [], 1, 0.02, 7.0, 6.99, 0.0, 0)))
    got = program([line for _, (line, _) in cases])
    for (tag, (_, exp)), g in zip(cases, got):
        assert_state(g, exp, tag)
    by = {tag: exp for tag, (_, exp) in cases}
    e = by[("aside", 0, 5)]                    # spelled out: r = 3 of 6 set aside on a rebuild, the entering position behind it
    assert e["Fi"] == [1, 2, 11, 29, 38] and e["xF"] == [4.0, 2.0, 3.0, 5.0, 6.0] and e["cF"] == [0.5, -1.5, 2.5, -4.5, 5.5]
    assert e["f"] == [3] and e["ftot"] == [5] and e["enter_pos"] == [4] and e["departed"] == [3] and e["n_aside"] == [2] and e["aside_rebuild"] == [1]
    assert e["mask"] == [1, 1, 1, 2, 1, 1] and e["gx"][3] == 0.0 and e["entered"] == [7]
    assert by[("aside", 1, 3)]["enter_pos"] == [-1] and by[("aside", 1, 3)]["aside_fresh"] == [1] and by[("aside", 1, 3)]["departed"] == [2]
    assert by[("aside", 0, 1)]["enter_pos"] == [1]
    assert by[("boundary, equal", 0)]["ftot"] == [5] and by[("boundary, above", 0)]["ftot"] == [6] and by[("NaN delta^2", 0)]["ftot"] == [5]
    assert by[("enters", 1, 3)]["f"] == [4] and by[("enters", 1, 3)]["entered"] == [8] and by[("enters", 1, 3)]["peak"] == [4]

"""Input classes beyond the bench's uniform matrices, shared by tests/golden/make_golden_big.py (which froze the
oracle's results for them in the build container) and the GPU tests that replay them.

  uniform53, dec4   SURVEY.md 8(d) generators; the engine generates them on the device from the seed
  tree              additive tree metric, dyadic branch lengths: path sums are exact, so the Q criterion has exact
                    ties everywhere (NeighborNetCanonical.java:151-178 first-strict-minimum, NetMakerOriginal.java:428-452)
  treenoise         additive tree metric with real-valued branch lengths + 5 % uniform noise (what real data look like)
  neg               uniform53 shifted by -0.25: a third of the entries negative (the lookahead windows' monotonicity
                    argument needs non-negative entries: the engine takes the plain fp64 scan for every event - no screening
                    pass, no windows; with several ranks the scan of every event is sharded -)
  outgroup          uniform53 with 3 taxa pushed 1e6 away from everyone (1e6 added to their rows and columns).  The Q
                    criterion only shifts under such pendant lengths, but max |D| grows by 1e6, so the screening slack
                    (screen_delta, proportional to max |D|) outgrows the spread of Q: every screening unit is a candidate
  dup               n/4 distinct treenoise taxa, each present 4 times, permuted: zero distances and identical rows
  dupk(n, k, ...)   the same with every taxon present k times: identical rows give bit-identical values of the selection
                    criterion, so every row has k - 1 tied row minima at the first event (the Relaxed mode's tie lists)

Host-generated classes depend on numpy's default_rng stream (PCG64), which is stable across numpy versions.
"""
import hashlib

import numpy as np

DEVICE_DISTS = ("uniform53", "dec4")
OUTGROUP_DIST = 1e6


def _tree(n, seed, dyadic):
    r = np.random.default_rng(seed)
    D = np.zeros((n, n))
    depth = np.zeros(n)
    stack = [(0, n, 0.0)]
    while stack:
        a, b, h = stack.pop()           # h = length of the path from the root to this node
        if b - a == 1:
            depth[a] = h
            continue
        c = int(r.integers(a + 1, b))
        la = float(r.integers(1, 64)) / 64.0 if dyadic else float(r.random()) + 0.01
        lb = float(r.integers(1, 64)) / 64.0 if dyadic else float(r.random()) + 0.01
        stack.append((a, c, h + la))
        stack.append((c, b, h + lb))
        D[a:c, c:b] -= 2.0 * h          # -2 h(lca); the leaf depths are added below
    iu = np.triu_indices(n, 1)
    D[iu] += depth[iu[0]] + depth[iu[1]]
    D = np.triu(D, 1)
    D = D + D.T
    p = r.permutation(n)
    return np.ascontiguousarray(D[np.ix_(p, p)])


def circ_noise(n, seed, noise=0.01, density=1.0):
    """A circular metric (random hidden cycle; a fraction `density` of the circular splits carries a random positive weight)
    with multiplicative noise: every distance times 1 + noise * U(-1, 1).  Built with the split-weight oracle's prefix-sum
    operator (test infrastructure).  The optimum of such distances has O(n^2) positive splits - the case that the dense
    factor of the block active-set method cannot hold ("capacity")."""
    from oracle import csw_oracle as W
    r = np.random.default_rng(seed)
    npairs = n * (n - 1) // 2
    x = r.random(npairs) + 0.01
    if density < 1.0:
        x *= r.random(npairs) < density
    dpos = W.calculate_ab(n, x)                   # distances between cycle POSITIONS (packed strict upper triangle)
    P = np.zeros((n, n))
    P[np.triu_indices(n, 1)] = dpos
    N = np.triu(1.0 + noise * (2.0 * r.random((n, n)) - 1.0), 1)
    P *= N
    P = P + P.T
    tax = r.permutation(n)                        # position -> taxon
    D = np.empty((n, n))
    D[np.ix_(tax, tax)] = P
    return np.ascontiguousarray(D)


def make(n, dist, seed, oracle):
    """The n x n matrix of an input class (host side; `oracle` = the oracle module, for the SplitMix64 generators)."""
    if dist in DEVICE_DISTS:
        return oracle.synth(n, seed, dist)
    if dist == "tree":
        return _tree(n, seed, True)
    if dist == "treenoise":
        T = _tree(n, seed, False)
        N = np.triu(np.random.default_rng(seed + 1000).random((n, n)) * 0.05, 1)
        return np.ascontiguousarray(T + N + N.T)
    if dist == "circnoise":
        return circ_noise(n, seed)
    if dist == "outgroup":
        D = oracle.synth(n, seed, "uniform53")
        o = np.random.default_rng(seed).choice(n, 3, replace=False)
        D[o, :] += OUTGROUP_DIST
        D[:, o] += OUTGROUP_DIST
        np.fill_diagonal(D, 0.0)
        return D
    if dist == "dup":
        k = (n + 3) // 4
        T = make(k, "treenoise", seed, oracle)
        idx = np.random.default_rng(seed + 2000).permutation(np.repeat(np.arange(k), 4)[:n])
        return np.ascontiguousarray(T[np.ix_(idx, idx)])
    if dist == "neg":
        D = oracle.synth(n, seed, "uniform53")
        D -= 0.25
        np.fill_diagonal(D, 0.0)
        return D
    raise ValueError(dist)


def dupk(n, k, seed, oracle):
    """ceil(n / k) distinct treenoise taxa, each present k times (the last one as often as fits), permuted as "dup" is."""
    t = -(-n // k)
    T = make(t, "treenoise", seed, oracle)
    idx = np.random.default_rng(seed + 2000).permutation(np.repeat(np.arange(t), k)[:n])
    return np.ascontiguousarray(T[np.ix_(idx, idx)])


def first_event_ties(D, rows=None):
    """For each of `rows` (default: all) the indices q != p that attain min_q (n - 2) D[p, q] - S[p] - S[q], the selection
    criterion of the first event (no clusters yet), as a list of index arrays.  Plain numpy, independent of the engine: the
    tests use it to assert what their inputs are meant to provoke."""
    n = D.shape[0]
    S = D.sum(axis=1)
    out = []
    for p in (range(n) if rows is None else rows):
        q = ((n - 2.0) * D[p] - S[p]) - S
        q[p] = np.inf
        out.append(np.nonzero(q == q.min())[0])
    return out


def sha_big(a):
    h = hashlib.sha256()
    flat = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    step = 1 << 28
    for o in range(0, flat.size, step):
        h.update(flat[o:o + step].tobytes())
    return h.hexdigest()


# Power-of-two scalings of a matrix for the value-range tests (tests/test_value_range.py).  D -> ldexp(D, k) commutes with every
# fp64 operation of the algorithm while nothing overflows or goes subnormal, so the trajectory stays the same and every scan
# minimum is ldexp(best, k); the engine's fp32 / bf16 screening copy, on the other hand, sees very different numbers.
FLT_MAX = float(np.finfo(np.float32).max)
SCREEN_DMAX_LIMIT = 1e37          # max |D| (3n + 64) must stay below this for the engine to screen (fnn_core.h: init_thread)


def screens(D, k=0):
    """Whether the engine screens ldexp(D, k) (fnn_core.h: init_thread, screen_ok)."""
    return np.ldexp(float(np.abs(D).max()), k) * (3.0 * D.shape[0] + 64.0) < SCREEN_DMAX_LIMIT


def float_rowsum_overflow(D, k):
    """Fraction of the rows whose fp64 row sum at the start, scaled by 2^k, rounds to inf in float (as (float)Sx does)."""
    s = np.abs(D).sum(axis=1)
    with np.errstate(over="ignore"):
        return float(np.isinf(np.ldexp(s, k).astype(np.float32)).mean())


def scale_exponents(D, band=(0.1, 0.9)):
    """The exponents k of the value-range sweep, with the band they are meant to reach:
      k_band  max |D| 2^k < 1e37 and 10-90 % (`band`) of the float row sums overflow at the start (the one closest to half);
              absent when no power of two reaches that band
      k_all   the largest k with max |D| 2^k < 1e37: every float row sum overflows at the start
      k_off   the smallest k with max |D| 2^k >= 1e37
      k_edge  the largest k at which the engine still screens (max |D| 2^k (3n + 64) < 1e37: no float overflows; the engine
              screened up to k_all once, and diverged from the oracle in the band)
      -60, -140, -900: small entries, entries in the fp32 / bf16 subnormal range, entries that are 0 in float"""
    dmax = float(np.abs(D).max())
    k_all = int(np.floor(np.log2(SCREEN_DMAX_LIMIT / dmax)))
    while np.ldexp(dmax, k_all) >= SCREEN_DMAX_LIMIT:
        k_all -= 1
    while np.ldexp(dmax, k_all + 1) < SCREEN_DMAX_LIMIT:
        k_all += 1
    k_edge = k_all
    while not screens(D, k_edge):
        k_edge -= 1
    ks = {"k_all": k_all, "k_off": k_all + 1, "k_edge": k_edge, "k_m60": -60, "k_m140": -140, "k_m900": -900}
    fr = {k: float_rowsum_overflow(D, k) for k in range(k_all - 40, k_all + 1)}
    inband = [(abs(f - 0.5), k) for k, f in fr.items() if band[0] <= f <= band[1]]
    if inband:  # (small n: the row sums may be too concentrated for any power of two to split them)
        ks["k_band"] = min(inband)[1]
    return ks

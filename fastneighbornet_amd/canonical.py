"""Host-side mirror of the reference's plug-in seam for the Canonical path.

Reference: `class NeighborNetCanonical extends NetMakerOriginal`
(NeighborNetCanonical.java:29-36), constructed by FastNN.main for `-mode Canonical`
(FastNN.java:324-328) and driven by one call to `runNeighborNet()`
(NetMakerOriginal.java:129-162, FastNN.java:378/:391).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi


class NeighborNetCanonical:
    """Same constructor shape and method name as the Java class.

    d          -- n x n symmetric fp64 distance matrix with zero diagonal (`double[][] d`).
                  Unlike the reference (NetMakerOriginal.java:653-656) the caller's array
                  is not modified.
    numTaxa    -- number of taxa (`ntax`)
    numThreads -- accepted for signature compatibility; the GPU engine always produces the
                  `-threads 1` result (the reference's pool branch is not deterministic,
                  SURVEY.md F7)
    pool       -- ignored (the Java ExecutorService)
    """

    def __init__(self, d, numTaxa: int, numThreads: int = 1, pool=None, *, device: int = 0,
                 validate: bool = True, record_events: bool = False):
        from . import api
        self._api = api()
        self.ntax = int(numTaxa)
        self.numThreads = int(numThreads)
        self.pool = pool
        self.D = np.ascontiguousarray(d, dtype=np.float64)
        if self.D.shape != (self.ntax, self.ntax):
            raise ValueError(f"d must be {self.ntax} x {self.ntax}")
        self._device = device
        self._validate = validate
        self._record = record_events
        self._relaxed_seed = None
        self.ordering = None
        self.stats = None
        self.events = None

    def runNeighborNet(self) -> np.ndarray:
        """int[ntax+1]: ordering[0] = 0, ordering[1] = 1, 1-based ids in circular order."""
        if self.ntax <= 3:  # NetMakerOriginal.java:133-140
            self.ordering = np.arange(self.ntax + 1, dtype=np.int32)
            return self.ordering
        with _capi.Handle(self._api, self.ntax, device=self._device, validate=self._validate,
                          record_events=self._record, relaxed_seed=self._relaxed_seed) as h:
            h.set_matrix(self.D)
            order, st = h.run()
            if self._record:
                self.events = h.events()
        self.ordering = order
        self.stats = st.as_dict()
        return order

    def getOrdering(self):  # NetMakerOriginal.java:72-74
        return self.ordering


class NeighborNetLocal(NeighborNetCanonical):
    """`-mode Relaxed` (NeighborNetLocal.java:25-32; FastNN.java:329-338): same constructor shape as the Java class
    plus `seed`.  The reference draws from ThreadLocalRandom, which cannot be seeded; the engine draws from
    java.util.Random(seed) - the generator of the line the reference commented out (:27) - so a run can be
    repeated.  `additive=True` (the additivity check) is not provided."""

    def __init__(self, d, numTaxa: int, numThreads: int = 1, additive: bool = False, pool=None, *, seed: int = 0,
                 device: int = 0, validate: bool = True, record_events: bool = False):
        if additive:
            raise NotImplementedError("the additivity check of the relaxed search (-additive) is not provided")
        super().__init__(d, numTaxa, numThreads, pool, device=device, validate=validate, record_events=record_events)
        self._relaxed_seed = int(seed)


def canonical_order(D: np.ndarray, device: int = 0, validate: bool = True) -> np.ndarray:
    """One-call form over `fnn_canonical_order_f64`."""
    from . import api
    a = api()
    D = np.ascontiguousarray(D, dtype=np.float64)
    n = D.shape[0]
    order = np.zeros(n + 1, dtype=np.int32)
    opts = _capi.FnnOpts()
    opts.device = device
    opts.validate = 1 if validate else 0
    a.check(a.canonical_order_f64(D.ctypes.data_as(C.POINTER(C.c_double)), n, n, C.byref(opts),
                                  order.ctypes.data_as(C.POINTER(C.c_int32)), None))
    return order


def batch_layout(D: np.ndarray):
    """(array, ld, stride) for a (B, n, n) fp64 array: the array itself where its strides can be said as a row stride and a
    problem stride in doubles (ld >= n, stride >= n * ld), a contiguous copy otherwise."""
    B, n, _ = D.shape
    s0, s1, s2 = D.strides
    if D.dtype == np.float64 and D.flags.aligned and D.dtype.isnative and B > 0 and n > 0 and s2 == 8 and s1 % 8 == 0 \
            and s0 % 8 == 0 and s1 // 8 >= n and s0 // 8 >= n * (s1 // 8):
        return D, s1 // 8, s0 // 8
    D = np.ascontiguousarray(D, dtype=np.float64)
    return D, max(n, 1), max(n * n, 1)


def canonical_order_batch(D, validate: bool = False, device: int = 0, events: bool = False):
    """Many problems of one size in one call (`fnn_canonical_order_batch_f64`): D has shape (B, n, n).  Up to
    `fnn_batch_lds_max_n()` taxa (140) every problem runs in a workgroup of its own, out of LDS; up to
    `fnn_batch_global_max_n()` taxa (1024), given at least `fnn_batch_global_min_batch(n)` problems, likewise with the
    matrix in a working copy in global memory (D itself is never written); anything else goes problem by problem
    through the one-problem engine.  A numpy array goes to the host entry (its strides are honoured where they amount to a
    row and a problem stride, otherwise it is copied); a torch.float64 tensor on the GPU goes to the device entry after
    torch.cuda.synchronize().  Returns orders[B, n + 1], or (orders, events[B, n], nevents[B]) with events=True."""
    from . import api
    a = api()
    on_device = False
    if hasattr(D, "is_cuda") and hasattr(D, "data_ptr"):  # a torch tensor
        import torch
        if D.dim() != 3 or D.shape[1] != D.shape[2]:
            raise ValueError("D must have shape (B, n, n)")
        if D.is_cuda:
            if D.dtype != torch.float64:
                raise TypeError("a tensor on the GPU must be torch.float64")
            D = D.contiguous()
            torch.cuda.synchronize(D.device)  # the batch call is not ordered against the stream that produced D
            if D.device.index is not None:
                device = D.device.index
            B, n = int(D.shape[0]), int(D.shape[1])
            ptr, ld, stride, on_device, keep = D.data_ptr(), max(n, 1), max(n * n, 1), True, D
        else:
            D = D.numpy()
    if not on_device:
        D = np.asarray(D)
        if D.ndim != 3 or D.shape[1] != D.shape[2]:
            raise ValueError("D must have shape (B, n, n)")
        B, n = D.shape[0], D.shape[1]
        keep, ld, stride = batch_layout(D)
        ptr = keep.ctypes.data
    orders, ev, nev, _ = _capi.run_batch(a, ptr, n, ld, stride, B, validate=validate, device=device, events=events,
                                         on_device=on_device)
    del keep
    return (orders, ev, nev) if events else orders


def split_weights(D: np.ndarray, ordering: np.ndarray, device: int = 0, allow_inexact: bool = False):
    """Non-negative least-squares weights of the circular splits of `ordering` over
    `fnn_split_weights_f64` (the optimum the reference's live path computes, FastNN.java:401-454, in its
    index order :405-419).  Returns (weights[n(n-1)/2], stats dict); stats["method"]: "closed form"
    (the unconstrained optimum is feasible), "from below" (the block active-set method on an inverse Cholesky
    factor of the free set) or "reference" (CircularSplitWeights.java's active-set /
    conjugate-gradient method); stats["refactorizations"] = rebuilds of the factor, stats["solves"] = sub-problems;
    stats["certified"] / stats["kkt_violation"]: the solver's own Kuhn-Tucker check of the returned weights.  Raises FnnError
    with code -6 (FNN_ECAPACITY: the optimum has more positive splits than the block method's factor holds and the
    reference's route is not affordable at this size) or -7 (FNN_EINEXACT, unless allow_inexact)."""
    from . import api
    a = api()
    D = np.ascontiguousarray(D, dtype=np.float64)
    n = D.shape[0]
    o = np.ascontiguousarray(ordering, dtype=np.int32)
    w = np.zeros(n * (n - 1) // 2, dtype=np.float64)
    st = _capi.FnnSwStats()
    rc = a.split_weights_f64(D.ctypes.data_as(C.POINTER(C.c_double)), n, n, o.ctypes.data_as(C.POINTER(C.c_int32)),
                             device, w.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st))
    if rc == -7 and allow_inexact:   # FNN_EINEXACT: the weights are there, their Kuhn-Tucker check is above 1e-9 (stats say by how much)
        rc = 0
    try:
        a.check(rc)
    except _capi.FnnError as e:       # FNN_ECAPACITY leaves the give-up reason, the capacity and the peak of the free set in the stats
        e.stats = {k: getattr(st, k) for k, _ in st._fields_ if not k.startswith(("reserved", "pad_"))}
        raise
    out = {k: getattr(st, k) for k, _ in st._fields_ if not k.startswith(("reserved", "pad_"))}
    out["method"] = ("closed form", "from below", "reference")[st.route]
    out["refactorizations"] = int(st.reserved[1])
    out["solves"] = int(st.reserved[2])
    return w, out


def split_weights_batch(D, orders, device: int = 0, allow_inexact: bool = False):
    """Split weights of many problems of one size in one call (`fnn_split_weights_batch_f64`): D has shape (B, n, n), `orders`
    (B, n + 1) is what `canonical_order_batch` returned for it.  Up to `fnn_split_weights_batch_max_n()` taxa (140) every
    problem is solved in a workgroup of its own (closed form, else Lawson-Hanson from below); a problem
    that gives up there, every problem of a larger n, and every call with fewer than `fnn_split_weights_batch_min_batch(n)`
    problems (the measured crossover: 1 / 4 / 8 / 16 / 32 up to 32 / 64 / 96 / 128 / 140 taxa) goes through the one-problem solver.  A numpy array goes to the
    host entry (strides honoured as in `canonical_order_batch`), a torch.float64 tensor on the GPU to the device entry after
    torch.cuda.synchronize().  Returns (W[B, n(n-1)/2], stats): stats is a dict of per-problem numpy arrays (the fields of
    fnn_sw_stats, and "method" as in `split_weights`); stats["call"] holds the fnn_sw_batch_stats fields.  Raises FnnError as
    `split_weights` does, the message naming the lowest failing problem; -7 (FNN_EINEXACT) unless allow_inexact."""
    from . import api
    a = api()
    on_device = False
    if hasattr(D, "is_cuda") and hasattr(D, "data_ptr"):  # a torch tensor
        import torch
        if D.dim() != 3 or D.shape[1] != D.shape[2]:
            raise ValueError("D must have shape (B, n, n)")
        if D.is_cuda:
            if D.dtype != torch.float64:
                raise TypeError("a tensor on the GPU must be torch.float64")
            D = D.contiguous()
            torch.cuda.synchronize(D.device)  # the batch call is not ordered against the stream that produced D
            if D.device.index is not None:
                device = D.device.index
            B, n = int(D.shape[0]), int(D.shape[1])
            ptr, ld, stride, on_device, keep = D.data_ptr(), max(n, 1), max(n * n, 1), True, D
        else:
            D = D.numpy()
    if not on_device:
        D = np.asarray(D)
        if D.ndim != 3 or D.shape[1] != D.shape[2]:
            raise ValueError("D must have shape (B, n, n)")
        B, n = D.shape[0], D.shape[1]
        keep, ld, stride = batch_layout(D)
        ptr = keep.ctypes.data
    if hasattr(orders, "cpu") and hasattr(orders, "numpy"):
        orders = orders.cpu().numpy()
    w, sw, st = _capi.run_splits_batch(a, ptr, n, ld, stride, B, orders, device=device, on_device=on_device, allow_inexact=allow_inexact)
    del keep
    out = {k: sw[k].copy() for k in sw.dtype.names if not k.startswith(("reserved", "pad_"))}
    out["method"] = np.array(_capi.SW_ROUTES, dtype=object)[sw["route"]] if B else np.array([], dtype=object)
    out["call"] = st.as_dict()
    return w, out


def ragged_layout(mats):
    """(base address, offsets, n, ld, on_device, device or None, keep) for a sequence of square matrices of any sizes: numpy
    arrays (host entry), or torch.float64 tensors that are all on one GPU (device entry, after torch.cuda.synchronize()).
    A matrix is used where it lies when it is float64 with unit column stride and a row stride of whole doubles (ld >= n);
    anything else is copied.  Offsets count doubles from the lowest address; `keep` holds what the addresses point into."""
    mats = list(mats)
    on_device = bool(mats) and all(hasattr(m, "is_cuda") and m.is_cuda for m in mats)
    keep, addr, ns, lds, device = [], [], [], [], None
    if on_device:
        import torch
        if len({m.device for m in mats}) != 1:
            raise ValueError("the tensors must be on one GPU")
        device = mats[0].device.index
        for m in mats:
            if m.dim() != 2 or m.shape[0] != m.shape[1]:
                raise ValueError("every matrix must be square")
            if m.dtype != torch.float64:
                raise TypeError("a tensor on the GPU must be torch.float64")
            n = int(m.shape[0])
            if n > 0 and not (m.stride(1) == 1 and m.stride(0) >= n):
                m = m.contiguous()
            keep.append(m)
            addr.append(m.data_ptr())
            ns.append(n)
            lds.append(max(int(m.stride(0)), n) if n > 1 else max(n, 1))
        torch.cuda.synchronize(mats[0].device)  # the call is not ordered against the stream that produced the tensors
    else:
        for m in mats:
            if hasattr(m, "is_cuda") and hasattr(m, "numpy"):
                m = m.cpu().numpy()
            m = np.asarray(m)
            if m.ndim != 2 or m.shape[0] != m.shape[1]:
                raise ValueError("every matrix must be square")
            n = m.shape[0]
            if not (m.dtype == np.float64 and m.dtype.isnative and m.flags.aligned and
                    (n <= 1 or (m.strides[1] == 8 and m.strides[0] % 8 == 0 and m.strides[0] // 8 >= n))):
                m = np.ascontiguousarray(m, dtype=np.float64)
            keep.append(m)
            addr.append(m.ctypes.data)
            ns.append(n)
            lds.append(m.strides[0] // 8 if n > 1 else max(n, 1))
    base = min(addr) if addr else 0
    if any((p - base) % 8 for p in addr):  # (numpy and torch allocate doubles on 8-byte boundaries; a view into a byte buffer may not be)
        raise ValueError("the matrices are not on 8-byte boundaries relative to each other")
    offsets = np.array([(p - base) // 8 for p in addr], dtype=np.int64)
    return base, offsets, np.array(ns, dtype=np.int32), np.array(lds, dtype=np.int64), on_device, device, keep


def canonical_order_ragged(mats, validate: bool = False, device: int = 0, events: bool = False):
    """Many problems of DIFFERENT sizes in one call (`fnn_canonical_order_ragged_f64`): `mats` is a
    sequence of square fp64 matrices, e.g. per-gene matrices over alignments with missing taxa.  Every problem gets exactly
    the order that `canonical_order_batch` gives it in a batch of its own size; up to `fnn_batch_lds_max_n()` taxa (140) the
    problems of all sizes share a few kernel launches, larger ones are grouped by size and take that call's route.  numpy
    arrays go to the host entry; torch.float64 tensors that are all on one GPU go to the device entry.  Returns a list of
    orders (n_b + 1 entries each), or (orders, events, nevents) with events=True: a list of event arrays, each cut to its
    problem's event count, and the counts."""
    from . import api
    a = api()
    base, offsets, ns, lds, on_device, dev, keep = ragged_layout(mats)
    orders, ev, nev, _ = _capi.run_ragged(a, base, offsets, ns, lds, validate=validate, device=device if dev is None else dev,
                                          events=events, on_device=on_device)
    del keep
    orders = [o.copy() for o in orders]
    return (orders, [e[:k].copy() for e, k in zip(ev, nev)], nev) if events else orders


def split_weights_ragged(mats, orders, device: int = 0, allow_inexact: bool = False):
    """Split weights of many problems of different sizes in one call (`fnn_split_weights_ragged_f64`): `mats` as for
    `canonical_order_ragged`, `orders` what it returned.  Every problem of up to `fnn_split_weights_batch_max_n()` taxa (140)
    is solved in a workgroup of its own, with the weights `split_weights_batch` gives it bit for bit, when the call holds at
    least `fnn_split_weights_batch_min_batch(largest such n)` of them; the rest, and what gives up in the kernel, goes through
    the one-problem solver.  Returns (weights, stats): a list of weight arrays (n_b (n_b - 1) / 2 each) and a dict of
    per-problem numpy arrays as `split_weights_batch` returns it, stats["call"] holding the fnn_sw_batch_stats fields.
    Raises FnnError as `split_weights_batch` does, the message naming the lowest failing problem."""
    from . import api
    a = api()
    base, offsets, ns, lds, on_device, dev, keep = ragged_layout(mats)
    orders = [o.cpu().numpy() if hasattr(o, "cpu") and hasattr(o, "numpy") else np.asarray(o) for o in orders]
    w, sw, st = _capi.run_splits_ragged(a, base, offsets, ns, orders, lds, device=device if dev is None else dev, on_device=on_device,
                                        allow_inexact=allow_inexact)
    del keep
    out = {k: sw[k].copy() for k in sw.dtype.names if not k.startswith(("reserved", "pad_"))}
    out["method"] = np.array(_capi.SW_ROUTES, dtype=object)[sw["route"]] if len(ns) else np.array([], dtype=object)
    out["call"] = st.as_dict()
    return [x.copy() for x in w], out


def split_weights_sparse(D: np.ndarray, ordering: np.ndarray, threshold: float = 1e-6, device: int = 0, capacity: int = 0):
    """`fnn_split_weights_sparse_f64`: only the weights above `threshold` (the reference's list, FastNN.java:455-466), as
    (indices[k], weights[k]) in ascending live index.  Returns (indices, weights, stats dict)."""
    from . import api
    a = api()
    D = np.ascontiguousarray(D, dtype=np.float64)
    n = D.shape[0]
    o = np.ascontiguousarray(ordering, dtype=np.int32)
    cap = int(capacity) if capacity > 0 else min(n * (n - 1) // 2, max(64 * n, 4096))
    while True:
        idx = np.zeros(cap, dtype=np.int64)
        w = np.zeros(cap, dtype=np.float64)
        cnt = C.c_int64(0)
        st = _capi.FnnSwStats()
        a.check(a.split_weights_sparse_f64(D.ctypes.data_as(C.POINTER(C.c_double)), n, n, o.ctypes.data_as(C.POINTER(C.c_int32)), device,
                                           float(threshold), idx.ctypes.data_as(C.POINTER(C.c_int64)), w.ctypes.data_as(C.POINTER(C.c_double)),
                                           cap, C.byref(cnt), C.byref(st)))
        if cnt.value <= cap:
            break
        cap = int(cnt.value)   # (more splits than room: once more with exactly enough)
    out = {k: getattr(st, k) for k, _ in st._fields_ if not k.startswith(("reserved", "pad_"))}
    out["method"] = ("closed form", "from below", "reference")[st.route]
    return idx[:cnt.value], w[:cnt.value], out


# ---- distance matrices of bootstrap replicates from an alignment

def encode_alignment(seqs, missing: str = "-?NX") -> np.ndarray:
    """A list of equal-length strings as the uint8 (n, L) array `alignment_distances_batch` takes: case is folded (to upper
    case), every character of `missing` becomes 255 (`FNN_SITE_MISSING`), every other character its byte."""
    rows = [s.upper().encode("latin-1") for s in seqs]
    if not rows or any(len(r) != len(rows[0]) for r in rows):
        raise ValueError("the sequences must be a non-empty list of strings of one length")
    out = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), len(rows[0])).copy()
    for ch in set(missing.upper().encode("latin-1")):
        out[out == ch] = _capi.SITE_MISSING
    return out


def bootstrap_counts(L: int, B: int, seed: int) -> np.ndarray:
    """Site multiplicities uint16 (B, L) of B bootstrap replicates of an L-site alignment (`fnn_bootstrap_counts`: host only,
    reproducible from `seed`; every row sums to L)."""
    from . import api
    return _capi.run_bootstrap_counts(api(), int(L), int(B), int(seed))


def _dist_inputs(seq, counts):
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    counts = np.ascontiguousarray(counts, dtype=np.uint16)
    if seq.ndim != 2 or counts.ndim != 2 or counts.shape[1] != seq.shape[1]:
        raise ValueError("seq must have shape (n, L) and counts (B, L)")
    return seq, counts


def alignment_distances_batch(seq, counts, device: int = 0, out: str = "numpy", model: str = "p", states: int = 4,
                              on_saturation: str = "fail", cap=None, gamma_shape=None):
    """Distance matrices of the replicates `counts` (uint16 (B, L) site multiplicities) of the alignment `seq` (uint8 (n, L),
    255 = missing: `encode_alignment`) over `fnn_alignment_distances_batch_f64`: exact integer counts on the int8 matrix
    cores and one IEEE division per entry.  out="numpy" returns a float64 array (B, n, n); out="torch" allocates a
    torch.float64 tensor (B, n, n) on the GPU and hands its address to the device entry, so that `canonical_order_batch` and
    `split_weights_batch` can read it in place.  Returns (matrices, stats dict).  Raises FnnError with code -1 naming the
    lowest (b, i, j) when two taxa share no site in a replicate.
    model: "p" (the default: mism / valid), "jc69" (Jukes-Cantor with `states` states, compared by equality) or "k2p" (Kimura
    two-parameter: the bytes A C G T U in either case are the four states, 255 stays missing and every other byte is counted
    in stats["n_recoded"] and treated as missing), over `fnn_alignment_distances_model_batch_f64`: the same exact counts, then a
    fixed sequence of fp64 operations with the library's own log1p.  A saturated pair (the model's distance is infinite) fails
    the call like an empty one with on_saturation="fail"; with "cap" it becomes `cap` (finite, > 0) and
    stats["n_saturated_problems"] counts the replicates that had one.
    "f81", "felsenstein84" (F84), "tn93" and "logdet" work on the exact 4 x 4 table of state pairs of every pair (`pair_counts_batch`), recoded
    as for "k2p", with the pair's own base frequencies; a pair that lacks a base the model divides by is degenerate and follows
    on_saturation like a saturated one (include/fastnn.h has each model's sequence of operations).
    gamma_shape: None (equal rates across sites) or the shape alpha > 0 of gamma-distributed rates for "jc69", "k2p", "f81",
    "felsenstein84" and "tn93": alpha * expm1(-log1p(-y) / alpha), with the library's own expm1, in place of every -ln(1 - y);
    "p" and "logdet" have no gamma form and refuse it.  A pair whose expm1 overflows (a very small alpha) is saturated."""
    from . import api
    a = api()
    seq, counts = _dist_inputs(seq, counts)
    (n, L), B = seq.shape, counts.shape[0]
    if model == "p" and gamma_shape is None:
        def run(ptr, **kw):
            return _capi.run_dist(a, seq.ctypes.data, n, L, L, counts.ctypes.data, B, L, ptr, max(n, 1), max(n * n, 1), device=device, **kw)
    else:
        m = _capi.dist_model(model, states, on_saturation, cap, gamma_shape)

        def run(ptr, **kw):
            return _capi.run_dist_model(a, seq.ctypes.data, n, L, L, counts.ctypes.data, B, L, ptr, max(n, 1), max(n * n, 1), m, device=device, **kw)
    if out == "torch":
        import torch
        dev = torch.device("cuda", device)
        D = torch.empty((B, n, n), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        st = run(D.data_ptr() if B and n else None, on_device=True)
    elif out == "numpy":
        D = np.empty((B, n, n), dtype=np.float64)
        st = run(D.ctypes.data)
    else:
        raise ValueError('out must be "numpy" or "torch"')
    return D, st.as_dict()


def pair_counts_batch(seq, counts, device: int = 0, out: str = "numpy"):
    """The 4 x 4 tables of state pairs of the replicates `counts` of the alignment `seq` over
    `fnn_alignment_pair_counts_batch_i64`: F[b, i, j, s, t] = the count-weighted number of sites at which taxon i shows state s
    and taxon j state t (A 0, C 1, G 2, T 3; recoded as for model="k2p"), exact int64 from the int8 matrix cores; F[b, j, i] is
    the transpose of F[b, i, j] and F[b, i, i] is zero.  out="numpy" returns an int64 array (B, n, n, 4, 4), out="torch" a
    torch.int64 tensor on the GPU.  Returns (tables, stats dict).  An empty pair is a table of zeros; nothing fails the call."""
    from . import api
    a = api()
    seq, counts = _dist_inputs(seq, counts)
    (n, L), B = seq.shape, counts.shape[0]

    def run(ptr, **kw):
        return _capi.run_pair_counts(a, seq.ctypes.data, n, L, L, counts.ctypes.data, B, L, ptr, max(n, 1), max(16 * n * n, 1), device=device, **kw)
    if out == "torch":
        import torch
        dev = torch.device("cuda", device)
        F = torch.empty((B, n, n, 4, 4), dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        st = run(F.data_ptr() if B and n else None, on_device=True)
    elif out == "numpy":
        F = np.empty((B, n, n, 4, 4), dtype=np.int64)
        st = run(F.ctypes.data)
    else:
        raise ValueError('out must be "numpy" or "torch"')
    return F, st.as_dict()


def bootstrap_distances(seq, B: int, seed: int, lead: int = 0, device: int = 0, out: str = "numpy", model: str = "p", states: int = 4,
                        on_saturation: str = "fail", cap=None, gamma_shape=None):
    """Distance matrices of B bootstrap replicates of the alignment `seq` (uint8 (n, L)) over
    `fnn_bootstrap_distances_batch_f64`: the replicates of `bootstrap_counts(L, B, seed)` without the counts - up to
    `fnn_bootstrap_draw_max_sites()` sites a kernel draws them on the GPU where the distance kernel reads them, and the
    alignment is all that is uploaded.  lead=1 puts the original data (every site once) in front as problem 0.  Returns
    (matrices (B + lead, n, n), stats dict), bit for bit what `alignment_distances_batch` returns for those counts; out, model,
    states, on_saturation, cap, gamma_shape as there.  stats adds "draw_route" ("device" or "host"), "max_count" and "t_draw_s"."""
    from . import api
    a = api()
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    if seq.ndim != 2:
        raise ValueError("seq must have shape (n, L)")
    if lead not in (0, 1) or B < 0:
        raise ValueError("lead must be 0 or 1 and B >= 0")
    n, L = seq.shape
    batch = int(B) + int(lead)
    m = _capi.dist_model(model, states, on_saturation, cap, gamma_shape)

    def run(ptr, **kw):
        return _capi.run_boot(a, seq.ctypes.data, n, L, L, batch, int(seed), int(lead), ptr, max(n, 1), max(n * n, 1), m, device=device, **kw)
    if out == "torch":
        import torch
        dev = torch.device("cuda", device)
        D = torch.empty((batch, n, n), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        st = run(D.data_ptr() if batch and n else None, on_device=True)
    elif out == "numpy":
        D = np.empty((batch, n, n), dtype=np.float64)
        st = run(D.ctypes.data)
    else:
        raise ValueError('out must be "numpy" or "torch"')
    return D, st.as_dict()


def _bootstrap_matrices(seq, B, seed, lead, draw, device, **model):
    """The replicates' matrices as a tensor on the GPU: draw="device" through `bootstrap_distances`, draw="host" through
    `bootstrap_counts` and `alignment_distances_batch`."""
    if draw == "device":
        return bootstrap_distances(seq, B, seed, lead=lead, device=device, out="torch", **model)
    if draw != "host":
        raise ValueError('draw must be "device" or "host"')
    counts = bootstrap_counts(seq.shape[1], B, seed)
    if lead:
        counts = np.concatenate([np.ones((1, seq.shape[1]), dtype=np.uint16), counts])
    return alignment_distances_batch(seq, counts, device=device, out="torch", **model)


def bootstrap(seq, B: int, seed: int, weights: bool = True, device: int = 0, model: str = "p", states: int = 4, on_saturation: str = "fail",
              cap=None, draw: str = "device", gamma_shape=None):
    """B bootstrap replicates of the alignment `seq` (uint8 (n, L)) end to end: the distance matrices of the replicates of
    `bootstrap_counts(L, B, seed)` as a tensor on the GPU, `canonical_order_batch` of that tensor and (weights=True)
    `split_weights_batch` of it.  No matrix crosses to the host.  Returns (orders[B, n + 1], W[B, n(n-1)/2] or None, stats) with
    stats = {"distances": ..., "splits": ... (weights=True)}.  model, states, on_saturation, cap, gamma_shape: as
    `alignment_distances_batch` takes them.  draw="device" (the default) draws the replicates on the GPU (`bootstrap_distances`); draw="host" makes the
    counts on the host and uploads them: the same matrices, bit for bit."""
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    D, dst = _bootstrap_matrices(seq, B, seed, 0, draw, device, model=model, states=states, on_saturation=on_saturation, cap=cap,
                                 gamma_shape=gamma_shape)
    orders = canonical_order_batch(D, device=device)
    stats = {"distances": dst}
    W = None
    if weights:
        W, stats["splits"] = split_weights_batch(D, orders, device=device)
    return orders, W, stats


# ---- site ranges: per-gene matrices and sliding windows without a counts matrix

def window_ranges(L: int, width: int, step: int = 1):
    """(starts, ends), int64: the windows [k step, k step + width) that lie fully inside [0, L), in order."""
    L, width, step = int(L), int(width), int(step)
    if width < 1 or width > L or step < 1:
        raise ValueError("window_ranges needs 1 <= width <= L and step >= 1")
    starts = np.arange(0, L - width + 1, step, dtype=np.int64)
    return starts, starts + width


def _range_inputs(seq, starts, ends):
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    starts = np.ascontiguousarray(starts, dtype=np.int64)
    ends = np.ascontiguousarray(ends, dtype=np.int64)
    if seq.ndim != 2 or starts.ndim != 1 or ends.shape != starts.shape:
        raise ValueError("seq must have shape (n, L), starts and ends one shape (B,)")
    return seq, starts, ends


def range_distances(seq, starts, ends, device: int = 0, out: str = "numpy", model: str = "p", states: int = 4, on_saturation: str = "fail",
                    cap=None, gamma_shape=None):
    """Distance matrices of the alignment `seq` (uint8 (n, L)) restricted to the site ranges [starts[b], ends[b]) - genes of a
    concatenated alignment, windows of a scan (`window_ranges`) - over `fnn_alignment_distances_ranges_f64`: bit for bit what
    `alignment_distances_batch` returns on the 0/1 counts of the ranges, without those counts: the kernel makes its operand
    from the bounds and walks the ranges' sites only.  Ranges may overlap, nest, repeat and come in any order (ranges that lie
    close together are cheapest next to each other); an empty range fails like a replicate without sites.  out, model, states,
    on_saturation, cap, gamma_shape as there.  Returns (matrices (B, n, n), stats dict); stats adds "n_site_blocks" (64-site
    blocks walked, per tile of 16 consecutive ranges) and "n_site_blocks_dense" (what the counts route would walk)."""
    from . import api
    a = api()
    seq, starts, ends = _range_inputs(seq, starts, ends)
    (n, L), B = seq.shape, starts.shape[0]
    m = _capi.dist_model(model, states, on_saturation, cap, gamma_shape)

    def run(ptr, **kw):
        return _capi.run_ranges(a, seq.ctypes.data, n, L, L, starts.ctypes.data, ends.ctypes.data, B, ptr, max(n, 1), max(n * n, 1), m, device=device, **kw)
    if out == "torch":
        import torch
        dev = torch.device("cuda", device)
        D = torch.empty((B, n, n), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        st = run(D.data_ptr() if B and n else None, on_device=True)
    elif out == "numpy":
        D = np.empty((B, n, n), dtype=np.float64)
        st = run(D.ctypes.data)
    else:
        raise ValueError('out must be "numpy" or "torch"')
    return D, st.as_dict()


def pair_counts_ranges(seq, starts, ends, device: int = 0, out: str = "numpy"):
    """The 4 x 4 tables of state pairs of the site ranges [starts[b], ends[b]) of the alignment `seq` over
    `fnn_alignment_pair_counts_ranges_i64`: what `pair_counts_batch` returns on the 0/1 counts of the ranges.  Returns (tables
    (B, n, n, 4, 4) int64, stats dict as `range_distances` reports it)."""
    from . import api
    a = api()
    seq, starts, ends = _range_inputs(seq, starts, ends)
    (n, L), B = seq.shape, starts.shape[0]

    def run(ptr, **kw):
        return _capi.run_pair_counts_ranges(a, seq.ctypes.data, n, L, L, starts.ctypes.data, ends.ctypes.data, B, ptr, max(n, 1), max(16 * n * n, 1),
                                            device=device, **kw)
    if out == "torch":
        import torch
        dev = torch.device("cuda", device)
        F = torch.empty((B, n, n, 4, 4), dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        st = run(F.data_ptr() if B and n else None, on_device=True)
    elif out == "numpy":
        F = np.empty((B, n, n, 4, 4), dtype=np.int64)
        st = run(F.ctypes.data)
    else:
        raise ValueError('out must be "numpy" or "torch"')
    return F, st.as_dict()


def range_networks(seq, starts, ends, weights: bool = True, device: int = 0, model: str = "p", states: int = 4, on_saturation: str = "fail",
                   cap=None, gamma_shape=None):
    """One Neighbor-Net per site range end to end, as `bootstrap` runs its replicates: `range_distances` as a tensor on the GPU,
    `canonical_order_batch` of that tensor and (weights=True) `split_weights_batch` of it.  No matrix crosses to the host.
    Returns (orders[B, n + 1], W[B, n(n-1)/2] or None, stats) with stats = {"distances": ..., "splits": ... (weights=True)}."""
    D, dst = range_distances(seq, starts, ends, device=device, out="torch", model=model, states=states, on_saturation=on_saturation, cap=cap,
                             gamma_shape=gamma_shape)
    orders = canonical_order_batch(D, device=device)
    stats = {"distances": dst}
    W = None
    if weights:
        W, stats["splits"] = split_weights_batch(D, orders, device=device)
    return orders, W, stats


def sliding_windows(seq, width: int, step: int = 1, weights: bool = True, device: int = 0, model: str = "p", states: int = 4,
                    on_saturation: str = "fail", cap=None, gamma_shape=None):
    """A scan along the alignment `seq`: `range_networks` on `window_ranges(L, width, step)`.  Returns (starts, ends, orders, W,
    stats)."""
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    if seq.ndim != 2:
        raise ValueError("seq must have shape (n, L)")
    starts, ends = window_ranges(seq.shape[1], width, step)
    orders, W, stats = range_networks(seq, starts, ends, weights=weights, device=device, model=model, states=states, on_saturation=on_saturation,
                                      cap=cap, gamma_shape=gamma_shape)
    return starts, ends, orders, W, stats


# ---- bootscan: bootstrap replicates inside every site range

def bootscan_counts(L: int, starts, ends, R: int, seed: int, lead: int = 0, first: int = 0, count=None) -> np.ndarray:
    """The counts a bootscan stands for (`fnn_bootscan_counts`, host only): rows first ... first + count - 1 (count=None: to the
    last) of the len(starts) * (R + lead) problems, window-major - per window `lead` rows of its 0/1 indicator, then the R rows of
    `bootstrap_counts(width, R, seed_w)` placed at the window's columns, seed_w the w-th SplitMix64 output of `seed`.  uint16
    (count, L)."""
    from . import api
    return _capi.run_bootscan_counts(api(), int(L), starts, ends, int(R), int(seed), int(lead), int(first), None if count is None else int(count))


def _bootscan_call(seq, starts, ends, R, seed, lead, device, out, m, tables):
    from . import api
    a = api()
    seq, starts, ends = _range_inputs(seq, starts, ends)
    if lead not in (0, 1) or R < 0:
        raise ValueError("lead must be 0 or 1 and R >= 0")
    (n, L), W, P = seq.shape, starts.shape[0], int(R) + int(lead)
    cell = (4, 4) if tables else ()

    def run(ptr, **kw):
        return _capi.run_scan(a, seq.ctypes.data, n, L, L, starts.ctypes.data, ends.ctypes.data, W, int(R), int(seed), int(lead), ptr, max(n, 1),
                              max((16 if tables else 1) * n * n, 1), m, device=device, tables=tables, **kw)
    if out == "torch":
        import torch
        dev = torch.device("cuda", device)
        D = torch.empty((W, P, n, n) + cell, dtype=torch.int64 if tables else torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        st = run(D.data_ptr() if W and P and n else None, on_device=True)
    elif out == "numpy":
        D = np.empty((W, P, n, n) + cell, dtype=np.int64 if tables else np.float64)
        st = run(D.ctypes.data)
    else:
        raise ValueError('out must be "numpy" or "torch"')
    return D, st.as_dict()


def bootscan_distances(seq, starts, ends, R: int, seed: int, lead: int = 1, device: int = 0, out: str = "numpy", model: str = "p", states: int = 4,
                       on_saturation: str = "fail", cap=None, gamma_shape=None):
    """Distance matrices of R bootstrap replicates inside every site range [starts[w], ends[w]) of the alignment `seq` (uint8
    (n, L)) over `fnn_bootscan_distances_f64`, lead=1 (the default) with the window's original data in front of them: for
    window w bit for bit what `bootstrap_distances(seq[:, starts[w]:ends[w]], R, seed_w, lead)` returns, seed_w the w-th
    SplitMix64 output of `seed`, and bit for bit what `alignment_distances_batch` returns on `bootscan_counts` - in one call,
    without those counts: a kernel draws every row of a plane that is only as long as its window, and the distance kernel
    walks that window's sites only.  out, model, states, on_saturation, cap, gamma_shape as there.  Returns (matrices (W, R +
    lead, n, n), stats dict); stats adds "n_windows", "n_site_blocks", "n_site_blocks_dense" and "n_host_chunks" (chunks that
    needed a second digit and were computed from the host's counts) to what `bootstrap_distances` reports."""
    m = _capi.dist_model(model, states, on_saturation, cap, gamma_shape)
    return _bootscan_call(seq, starts, ends, R, seed, lead, device, out, m, False)


def bootscan_pair_counts(seq, starts, ends, R: int, seed: int, lead: int = 1, device: int = 0, out: str = "numpy"):
    """The 4 x 4 tables of state pairs of the same problems over `fnn_bootscan_pair_counts_i64`: what `pair_counts_batch` returns
    on `bootscan_counts`.  Returns (tables (W, R + lead, n, n, 4, 4) int64, stats dict as `bootscan_distances` reports it)."""
    return _bootscan_call(seq, starts, ends, R, seed, lead, device, out, None, True)


def bootscan_networks(seq, starts, ends, R: int, seed: int, threshold: float = 1e-6, device: int = 0, model: str = "p", states: int = 4,
                      on_saturation: str = "fail", cap=None, gamma_shape=None):
    """A bootscan end to end: `bootscan_distances(..., lead=1)` as a tensor on the GPU, `canonical_order_batch` and
    `split_weights_batch` of all W (R + 1) problems at once, then `split_support(..., lead=1)` of every window's R + 1 problems,
    one call per window.  No matrix crosses to the host.  Returns (orders[W, n + 1], weights[W, n(n-1)/2], tables, stats): the
    order and the weights of every window's original data, one support table per window - as `bootstrap_support` returns it for
    the window's slice - and stats = {"distances", "splits", "support": one dict per window}."""
    D, dst = bootscan_distances(seq, starts, ends, R, seed, lead=1, device=device, out="torch", model=model, states=states, on_saturation=on_saturation,
                                cap=cap, gamma_shape=gamma_shape)
    W, P, n = D.shape[0], D.shape[1], D.shape[2]
    flat = D.reshape(W * P, n, n)
    orders = canonical_order_batch(flat, device=device)
    Wt, sst = split_weights_batch(flat, orders, device=device)
    tables, ust = [], []
    for w in range(W):
        t, u = split_support(orders[w * P:(w + 1) * P], Wt[w * P:(w + 1) * P], threshold=threshold, lead=1, device=device)
        tables.append(t)
        ust.append(u)
    return orders[::P].copy(), Wt[::P].copy(), tables, {"distances": dst, "splits": sst, "support": ust}


def bootscan(seq, width: int, step: int, R: int, seed: int, threshold: float = 1e-6, device: int = 0, model: str = "p", states: int = 4,
             on_saturation: str = "fail", cap=None, gamma_shape=None):
    """A bootscan along the alignment `seq`: `bootscan_networks` on `window_ranges(L, width, step)`.  Returns (starts, ends,
    orders, weights, tables, stats)."""
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    if seq.ndim != 2:
        raise ValueError("seq must have shape (n, L)")
    starts, ends = window_ranges(seq.shape[1], width, step)
    orders, Wt, tables, stats = bootscan_networks(seq, starts, ends, R, seed, threshold=threshold, device=device, model=model, states=states,
                                                  on_saturation=on_saturation, cap=cap, gamma_shape=gamma_shape)
    return starts, ends, orders, Wt, tables, stats


# ---- split support: the distinct splits of many problems, tallied

def split_support(orders, W, threshold: float = 1e-6, lead: int = 0, device: int = 0):
    """The table of the distinct splits of B problems over one taxon set (`fnn_split_support_f64`): `orders` (B, n + 1) as
    `canonical_order_batch` returns them, `W` (B, n(n-1)/2) as `split_weights_batch` returns it - a numpy array (host entry) or
    a torch.float64 tensor on the GPU (device entry, after torch.cuda.synchronize()).  A weight counts when it is above
    `threshold`; the first `lead` problems define rows but are not tallied (lead=1 with the original data as problem 0: the
    rows with first_b == 0 are the reference network's splits, each with its bootstrap support).  Returns (table, stats):
    table is a dict of numpy arrays in order of first appearance - keys (S, words) uint64 (bit t - 1 of the key = taxon t, on
    the side without taxon 1; `key_taxa`), first_b, first_k, count, weight_sum (the sum over the counted problems in
    ascending b, one rounding per addition) and support = count / (B - lead); stats holds the fnn_support_stats fields and
    "method" ("kernel" or "host")."""
    from . import api
    a = api()
    if hasattr(orders, "cpu") and hasattr(orders, "numpy"):
        orders = orders.cpu().numpy()
    orders = np.ascontiguousarray(orders, dtype=np.int32)
    if orders.ndim != 2 or orders.shape[1] < 3:
        raise ValueError("orders must have shape (B, n + 1) with n >= 2")
    B, n = orders.shape[0], orders.shape[1] - 1
    K = n * (n - 1) // 2
    on_device = False
    if hasattr(W, "is_cuda") and hasattr(W, "data_ptr"):  # a torch tensor
        import torch
        if W.is_cuda:
            if W.dtype != torch.float64:
                raise TypeError("a tensor on the GPU must be torch.float64")
            W = W.contiguous()
            torch.cuda.synchronize(W.device)  # the call is not ordered against the stream that produced W
            if W.device.index is not None:
                device = W.device.index
            on_device, ptr = True, W.data_ptr()
        else:
            W = W.numpy()
    if not on_device:
        W = np.ascontiguousarray(W, dtype=np.float64)
        ptr = W.ctypes.data
    if tuple(W.shape) != (B, K):
        raise ValueError(f"W must have shape ({B}, {K})")
    # room for an upper bound of S: the counting records (a NaN threshold is the call's to refuse)
    cap = int((W > float(threshold)).sum()) if B else 0
    table, S, st = _capi.run_support(a, n, B, orders.ctypes.data, ptr if B else None, float(threshold), int(lead), cap, device=device,
                                     on_device=on_device)
    table = {k: v[:S].copy() for k, v in table.items()}
    table["support"] = table["count"] / float(B - lead) if B > lead else np.zeros(S, dtype=np.float64)
    out = st.as_dict()
    out["method"] = _capi.SUPPORT_ROUTES[st.route]
    return table, out


def split_keys(order, ks) -> np.ndarray:
    """The keys (len(ks), words) uint64 of the splits `ks` (indices k of `split_weights`) of one ordering (`fnn_split_keys`:
    host only), as the rows of `split_support`'s table hold them."""
    from . import api
    order = np.ascontiguousarray(order, dtype=np.int32)
    return _capi.run_split_keys(api(), len(order) - 1, order, ks)


def key_taxa(key) -> list:
    """The sorted 1-based taxon ids of one key (a row of table["keys"])."""
    return [64 * w + b + 1 for w, x in enumerate(np.asarray(key, dtype=np.uint64).tolist()) for b in range(64) if (x >> b) & 1]


def bootstrap_support(seq, B: int, seed: int, threshold: float = 1e-6, device: int = 0, model: str = "p", states: int = 4,
                      on_saturation: str = "fail", cap=None, draw: str = "device", gamma_shape=None):
    """A bootstrap run with its result: the original alignment as problem 0 (every site once) in front of the B replicates of
    `bootstrap_counts(L, B, seed)`, through distances, orders and split weights as `bootstrap` runs them, then
    `split_support(..., lead=1)`.  Returns (order, weights, table, stats): the order and the weights of the original data, the
    table - its rows with first_b == 0 are the original network's splits above `threshold` in ascending k, `support` the share
    of the B replicates that hold each - and stats = {"distances", "splits", "support"}.  model, states, on_saturation, cap, gamma_shape: as
    `alignment_distances_batch` takes them; draw: as `bootstrap` takes it."""
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    D, dst = _bootstrap_matrices(seq, B, seed, 1, draw, device, model=model, states=states, on_saturation=on_saturation, cap=cap,
                                 gamma_shape=gamma_shape)
    orders = canonical_order_batch(D, device=device)
    W, sst = split_weights_batch(D, orders, device=device)
    table, ust = split_support(orders, W, threshold=threshold, lead=1, device=device)
    return orders[0], W[0], table, {"distances": dst, "splits": sst, "support": ust}

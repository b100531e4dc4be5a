"""ctypes view of the C ABI declared in include/fastnn.h.

`Api(lib, prefix)` binds one shared library.  The product uses
`Api(libfastnn_hip.so, "fnn_")`; the CPU tests reuse the same class for the
emulation driver (`tests/emu`, prefix "emu_"), which exports the same entry
points over the same host logic.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

FNN_OK = 0
STATUS_NAMES = {0: "FNN_OK", -1: "FNN_EINVAL", -2: "FNN_ENOMEM", -3: "FNN_EHIP", -4: "FNN_ERCCL",
                -5: "FNN_ESTATE", -6: "FNN_ECAPACITY", -7: "FNN_EINEXACT"}

KIND_2WAY, KIND_3WAY, KIND_4WAY, KIND_FINISH = 2, 3, 4, 5


class FnnOpts(C.Structure):
    _fields_ = [("device", C.c_int32), ("validate", C.c_int32), ("record_events", C.c_int32),
                ("force_exact_rx", C.c_int32), ("disable_screen", C.c_int32), ("lookahead", C.c_int32),
                ("lookahead_pairs", C.c_int32), ("mode", C.c_int32), ("relaxed_seed_lo", C.c_uint32),
                ("relaxed_seed_hi", C.c_uint32), ("relaxed_min_active", C.c_int32), ("reserved", C.c_int32 * 5)]


class FnnEvent(C.Structure):
    _fields_ = [("m_before", C.c_int32), ("c_before", C.c_int32), ("cx_id", C.c_int32),
                ("cy_id", C.c_int32), ("x_id", C.c_int32), ("y_id", C.c_int32), ("kind", C.c_int32),
                ("u_id", C.c_int32), ("best", C.c_double), ("entries", C.c_int64)]

    def key(self):
        return (self.m_before, self.c_before, self.cx_id, self.cy_id, self.x_id, self.y_id,
                self.kind, self.u_id)


class FnnStats(C.Structure):
    _fields_ = [("n_events", C.c_int64), ("sum_entries", C.c_int64), ("t_init_s", C.c_double),
                ("t_agglom_s", C.c_double), ("t_expand_s", C.c_double), ("t_total_s", C.c_double),
                ("t_scan_s", C.c_double), ("scan_launches", C.c_int64), ("scan_bytes", C.c_int64),
                ("n_rx_certified", C.c_int64), ("n_rx_exact", C.c_int64), ("n_screen_events", C.c_int64),
                ("n_rescan_units", C.c_int64), ("n_base_scans", C.c_int64), ("n_window_hits", C.c_int64),
                ("n_window_fails", C.c_int64), ("window_pairs", C.c_int64), ("bytes_total", C.c_int64),
                ("n_handover_retries", C.c_int64), ("n_sweeps_exact", C.c_int64), ("t_plain_s", C.c_double),
                ("plain_launches", C.c_int64), ("plain_bytes", C.c_int64), ("n_stalled_events", C.c_int64),
                ("n_relaxed_events", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class FnnSwStats(C.Structure):
    _fields_ = [("outer_iterations", C.c_int64), ("cg_calls", C.c_int64), ("cg_iterations", C.c_int64),
                ("nsplits", C.c_int64), ("t_solve_s", C.c_double), ("reserved", C.c_int64 * 3),
                # ABI version 2
                ("route", C.c_int32), ("certified", C.c_int32), ("kkt_violation", C.c_double), ("final_threshold_rel", C.c_double),
                ("n_set_aside", C.c_int64), ("capacity", C.c_int64), ("free_set_peak", C.c_int64), ("giveup_reason", C.c_int32),
                ("pad_", C.c_int32), ("entered", C.c_int64), ("screened_out", C.c_int64), ("departed", C.c_int64),
                ("t_alloc_s", C.c_double),
                # reserved2[0..3] of include/fastnn.h: how often the batch kernel's safety net ran for this problem (splits set
                # aside as dependent on a fresh append / on a rebuild / because they left in their entering step; rechecks of the
                # splits set aside; releases after progress).  [3] holds two 32-bit counts.  0 from the one-problem solver.
                ("aside_fresh", C.c_int64), ("aside_rebuild", C.c_int64), ("aside_entering", C.c_int64),
                ("rechecks", C.c_int32), ("releases", C.c_int32)]


class FnnBatchStats(C.Structure):
    _fields_ = [("n_problems", C.c_int64), ("n_lds", C.c_int64), ("n_fallback", C.c_int64), ("n_events", C.c_int64),
                ("lds_max_n", C.c_int32), ("block_threads", C.c_int32), ("lds_bytes", C.c_int32), ("chunks", C.c_int32),
                ("t_upload_s", C.c_double), ("t_kernel_s", C.c_double), ("t_total_s", C.c_double), ("n_global", C.c_int64), ("reserved", C.c_int64 * 3)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class FnnSwBatchStats(C.Structure):
    _fields_ = [("n_problems", C.c_int64), ("n_closed_form", C.c_int64), ("n_kernel", C.c_int64), ("n_fallback", C.c_int64),
                ("max_n", C.c_int32), ("block_threads", C.c_int32), ("lds_bytes", C.c_int32), ("chunks", C.c_int32),
                ("workspace_bytes", C.c_int64), ("capacity", C.c_int64),
                ("t_upload_s", C.c_double), ("t_kernel_s", C.c_double), ("t_total_s", C.c_double), ("reserved", C.c_int64 * 4)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


EVENT_DTYPE = np.dtype(
    [("m_before", "<i4"), ("c_before", "<i4"), ("cx_id", "<i4"), ("cy_id", "<i4"),
     ("x_id", "<i4"), ("y_id", "<i4"), ("kind", "<i4"), ("u_id", "<i4"),
     ("best", "<f8"), ("entries", "<i8")], align=True)


# int32_t (*fnn_allgather_fn)(void* ctx, const void* send, void* recv, int32_t bytes_per_rank)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32)


class FnnError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{STATUS_NAMES.get(code, code)}: {msg}")
        self.code = code


_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


class Api:
    def __init__(self, lib: C.CDLL, prefix: str, engine: bool = True):
        self.lib = lib
        self.prefix = prefix
        f = self._fn
        f("last_error", C.c_char_p, [])
        if not engine:  # (a library with the batch entry points only: the CPU driver of tests/emu/fnn_batch_emu.cpp)
            return
        f("create", C.c_int32, [C.c_int32, C.POINTER(FnnOpts), C.POINTER(C.c_void_p)])
        f("destroy", C.c_int32, [C.c_void_p])
        f("set_rows", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, _dp, C.c_int64])
        f("set_packed_upper", C.c_int32, [C.c_void_p, _dp])
        f("synth", C.c_int32, [C.c_void_p, C.c_uint64, C.c_int32])
        f("run", C.c_int32, [C.c_void_p, _ip, C.POINTER(FnnStats)])
        f("begin", C.c_int32, [C.c_void_p])
        f("step", C.c_int32, [C.c_void_p, C.POINTER(FnnEvent)])
        f("finish", C.c_int32, [C.c_void_p, _ip])
        f("get_events", C.c_int64, [C.c_void_p, C.c_void_p, C.c_int64])
        f("get_counts", C.c_int32, [C.c_void_p, _ip, _ip, _ip])
        f("get_nodes", C.c_int32, [C.c_void_p, _ip, _ip, _dp])
        f("get_live_matrix", C.c_int32, [C.c_void_p, _dp])
        f("get_matrix", C.c_int32, [C.c_void_p, _dp, C.c_int64])
        f("comm_init_host", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, ALLGATHER_FN, C.c_void_p])

    def _fn(self, name, restype, argtypes, optional=False):
        try:
            fn = getattr(self.lib, self.prefix + name)
        except AttributeError:
            if optional:
                return None
            raise
        fn.restype = restype
        fn.argtypes = argtypes
        setattr(self, name, fn)
        return fn

    def check(self, rc):
        if rc < 0:
            raise FnnError(rc, (self.last_error() or b"").decode("utf-8", "replace"))
        return rc


_BATCH_ARGS = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.POINTER(FnnOpts), _ip, C.c_void_p, _ip,
               C.POINTER(FnnBatchStats)]


def bind_batch(a: Api) -> Api:
    """The batch entry points of include/fastnn.h (many small problems, one workgroup each) on `a`."""
    a._fn("batch_lds_max_n", C.c_int32, [])
    a._fn("batch_global_max_n", C.c_int32, [], optional=True)            # (the CPU driver of the LDS route has neither)
    a._fn("batch_global_min_batch", C.c_int64, [C.c_int32], optional=True)
    a._fn("canonical_order_batch_f64", C.c_int32, _BATCH_ARGS)
    a._fn("canonical_order_batch_device_f64", C.c_int32, _BATCH_ARGS)
    return a


def run_batch(a: Api, D, n: int, ld: int, stride: int, batch: int, validate: bool = False, device: int = 0,
              events: bool = False, on_device: bool = False, fill: int = 0):
    """One batch call; D = address of problem 0 (host memory, or device memory with on_device).  Returns
    (orders[batch, n + 1], events[batch, n] or None, nevents[batch], stats); on failure FnnError carries the untouched
    output array as `.orders` (filled with `fill`)."""
    orders = np.full((batch, n + 1), fill, dtype=np.int32)
    ev = np.zeros((batch, max(n, 1)), dtype=EVENT_DTYPE) if events else None
    nev = np.full(batch, fill, dtype=np.int32)
    opts = FnnOpts()
    opts.device = device
    opts.validate = 1 if validate else 0
    st = FnnBatchStats()
    fn = a.canonical_order_batch_device_f64 if on_device else a.canonical_order_batch_f64
    rc = fn(D, n, ld, stride, batch, C.byref(opts), orders.ctypes.data_as(_ip), ev.ctypes.data if events else None,
            nev.ctypes.data_as(_ip), C.byref(st))
    try:
        a.check(rc)
    except FnnError as e:
        e.orders = orders
        raise
    return orders, ev, nev, st


_SPLITS_BATCH_ARGS = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int64, _ip, C.c_int32, _dp, C.POINTER(FnnSwStats),
                      C.POINTER(FnnSwBatchStats)]
SW_ROUTES = ("closed form", "from below", "reference")


def bind_splits_batch(a: Api) -> Api:
    """The batched split-weight entry points of include/fastnn.h (one workgroup per small problem) on `a`."""
    a._fn("split_weights_batch_max_n", C.c_int32, [])
    a._fn("split_weights_batch_min_batch", C.c_int64, [C.c_int32])
    a._fn("split_weights_batch_f64", C.c_int32, _SPLITS_BATCH_ARGS)
    a._fn("split_weights_batch_device_f64", C.c_int32, _SPLITS_BATCH_ARGS)
    return a


def run_splits_batch(a: Api, D, n: int, ld: int, stride: int, batch: int, orders, device: int = 0, on_device: bool = False,
                     allow_inexact: bool = False, fill: float = 0.0):
    """One batched split-weight call; D = address of problem 0 (host memory, or device memory with on_device), orders =
    int32 array (batch, n + 1).  Returns (weights[batch, n(n-1)/2], per-problem stats as a numpy record array, call
    stats); on failure FnnError carries the untouched output array as `.weights` (filled with `fill`)."""
    orders = np.ascontiguousarray(orders, dtype=np.int32)
    if orders.shape != (batch, n + 1):
        raise ValueError(f"orders must have shape ({batch}, {n + 1})")
    w = np.full((batch, max(n * (n - 1) // 2, 0)), fill, dtype=np.float64)
    sw = (FnnSwStats * max(batch, 1))()
    st = FnnSwBatchStats()
    fn = a.split_weights_batch_device_f64 if on_device else a.split_weights_batch_f64
    rc = fn(D, n, ld, stride, batch, orders.ctypes.data_as(_ip), device, w.ctypes.data_as(_dp), sw, C.byref(st))
    if rc == -7 and allow_inexact:   # FNN_EINEXACT: the weights are there; stats say which problems failed their check
        rc = 0
    try:
        a.check(rc)
    except FnnError as e:
        e.weights = w
        raise
    return w, np.ctypeslib.as_array(sw)[:batch].copy(), st


class FnnDistStats(C.Structure):
    _fields_ = [("n_problems", C.c_int64), ("n_pairs", C.c_int64), ("n_sites", C.c_int64),
                ("digit_passes", C.c_int32), ("has_missing", C.c_int32), ("block_threads", C.c_int32), ("chunks", C.c_int32),
                ("t_upload_s", C.c_double), ("t_kernel_s", C.c_double), ("t_total_s", C.c_double), ("reserved", C.c_int64 * 4)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


SITE_MISSING = 255
DIST_P = 0
_DIST_ARGS = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
              C.c_int64, C.c_int64, C.POINTER(FnnDistStats)]


def bind_dist(a: Api) -> Api:
    """The alignment-distance entry points of include/fastnn.h (distance matrices of bootstrap replicates) on `a`."""
    a._fn("alignment_distances_batch_f64", C.c_int32, _DIST_ARGS)
    a._fn("alignment_distances_batch_device_f64", C.c_int32, _DIST_ARGS)
    a._fn("bootstrap_counts", C.c_int32, [C.c_int64, C.c_int64, C.c_uint64, C.c_void_p])
    return a


def run_dist(a: Api, seq, n: int, L: int, lds: int, counts, batch: int, ldc: int, out, ld: int, stride: int,
             model: int = DIST_P, device: int = 0, on_device: bool = False):
    """One alignment-distance call on raw addresses (seq, counts: host memory; out: host memory, or device memory with
    on_device); any of them may be None (NULL).  Returns the stats."""
    st = FnnDistStats()
    fn = a.alignment_distances_batch_device_f64 if on_device else a.alignment_distances_batch_f64
    a.check(fn(seq, n, L, lds, counts, batch, ldc, model, device, out, ld, stride, C.byref(st)))
    return st


class FnnDistModel(C.Structure):
    _fields_ = [("model", C.c_int32), ("states", C.c_int32), ("on_saturation", C.c_int32), ("reserved", C.c_int32), ("cap", C.c_double)]


class FnnDistModelRates(C.Structure):
    """fnn_dist_model_rates: `base.reserved` = DIST_RATES_GAMMA and the entries are handed the address of `base`."""
    _fields_ = [("base", FnnDistModel), ("shape", C.c_double), ("reserved", C.c_double * 3)]


class FnnDistModelStats(C.Structure):
    _fields_ = [("base", FnnDistStats), ("n_recoded", C.c_int64), ("n_saturated_problems", C.c_int64), ("reserved", C.c_int64 * 2)]

    def as_dict(self):
        return dict(self.base.as_dict(), n_recoded=self.n_recoded, n_saturated_problems=self.n_saturated_problems)


DIST_JC69, DIST_K2P = 1, 2
DIST_SAT_FAIL, DIST_SAT_CAP = 0, 1
DIST_F81, DIST_F84, DIST_TN93, DIST_LOGDET = 16, 17, 18, 19   # on the 4 x 4 table of state pairs
# (Felsenstein 1984 is spelled out: "f84" stays a name these wrappers do not know)
DIST_MODELS = {"p": DIST_P, "jc69": DIST_JC69, "k2p": DIST_K2P, "f81": DIST_F81, "felsenstein84": DIST_F84, "tn93": DIST_TN93, "logdet": DIST_LOGDET}
DIST_POLICIES = {"fail": DIST_SAT_FAIL, "cap": DIST_SAT_CAP}
DIST_RATES_EQUAL, DIST_RATES_GAMMA = 0, 1
_DIST_MODEL_ARGS = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(FnnDistModel), C.c_int32,
                    C.c_void_p, C.c_int64, C.c_int64, C.POINTER(FnnDistModelStats)]


def bind_dist_model(a: Api) -> Api:
    """The entry points of the corrected alignment distances of include/fastnn.h (JC69, K2P) on `a`."""
    a._fn("alignment_distances_model_batch_f64", C.c_int32, _DIST_MODEL_ARGS)
    a._fn("alignment_distances_model_batch_device_f64", C.c_int32, _DIST_MODEL_ARGS)
    return a


def dist_model(model="p", states: int = 4, on_saturation="fail", cap=None, gamma_shape=None):
    """fnn_dist_model from names ("p", "jc69", "k2p", "f81", "felsenstein84", "tn93", "logdet"; "fail", "cap") or the header's numbers;
    cap=None is 0.0.  gamma_shape=None: equal rates, a FnnDistModel; a number: a FnnDistModelRates with that shape (the call
    refuses what is not finite and > 0)."""
    if gamma_shape is not None:
        mr = FnnDistModelRates()
        mr.base = dist_model(model, states, on_saturation, cap)
        mr.base.reserved = DIST_RATES_GAMMA
        mr.shape = float(gamma_shape)
        return mr
    m = FnnDistModel()
    m.model = DIST_MODELS[model.lower()] if isinstance(model, str) else int(model)
    m.states = int(states)
    m.on_saturation = DIST_POLICIES[on_saturation.lower()] if isinstance(on_saturation, str) else int(on_saturation)
    m.cap = 0.0 if cap is None else float(cap)
    return m


def dist_model_ref(m):
    """What the entries take for `m`: the address of a FnnDistModel, of the first member of a FnnDistModelRates, or NULL."""
    if m is None:
        return None
    return C.byref(m.base) if isinstance(m, FnnDistModelRates) else C.byref(m)


def run_dist_model(a: Api, seq, n: int, L: int, lds: int, counts, batch: int, ldc: int, out, ld: int, stride: int, m: FnnDistModel,
                   device: int = 0, on_device: bool = False):
    """`run_dist` through the model entries; m=None passes NULL.  Returns the stats (FnnDistModelStats)."""
    st = FnnDistModelStats()
    fn = a.alignment_distances_model_batch_device_f64 if on_device else a.alignment_distances_model_batch_f64
    a.check(fn(seq, n, L, lds, counts, batch, ldc, dist_model_ref(m), device, out, ld, stride, C.byref(st)))
    return st


_PAIR_COUNTS_ARGS = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int64,
                     C.POINTER(FnnDistModelStats)]


def bind_pair_counts(a: Api) -> Api:
    """The entry points of include/fastnn.h that hand out the 4 x 4 tables of state pairs on `a`."""
    a._fn("alignment_pair_counts_batch_i64", C.c_int32, _PAIR_COUNTS_ARGS)
    a._fn("alignment_pair_counts_batch_device_i64", C.c_int32, _PAIR_COUNTS_ARGS)
    return a


def run_pair_counts(a: Api, seq, n: int, L: int, lds: int, counts, batch: int, ldc: int, out, ld: int, stride: int, device: int = 0,
                    on_device: bool = False):
    """One pair-count call on raw addresses (out: int64, 16 per (i, j); host memory, or device memory with on_device).  Returns
    the stats (FnnDistModelStats)."""
    st = FnnDistModelStats()
    fn = a.alignment_pair_counts_batch_device_i64 if on_device else a.alignment_pair_counts_batch_i64
    a.check(fn(seq, n, L, lds, counts, batch, ldc, device, out, ld, stride, C.byref(st)))
    return st


def run_bootstrap_counts(a: Api, L: int, batch: int, seed: int) -> np.ndarray:
    counts = np.zeros((max(batch, 0), max(L, 0)), dtype=np.uint16)
    a.check(a.bootstrap_counts(L, batch, seed & 0xFFFFFFFFFFFFFFFF, counts.ctypes.data))
    return counts


class FnnBootStats(C.Structure):
    _fields_ = [("model", FnnDistModelStats), ("draw_route", C.c_int32), ("max_count", C.c_int32), ("t_draw_s", C.c_double),
                ("reserved", C.c_int64 * 4)]

    def as_dict(self):
        return dict(self.model.as_dict(), draw_route=DRAW_ROUTES[self.draw_route], max_count=self.max_count, t_draw_s=self.t_draw_s)


DRAW_DEVICE, DRAW_HOST = 0, 1
DRAW_ROUTES = ("device", "host")
_BOOT_ARGS = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_uint64, C.c_int64, C.POINTER(FnnDistModel), C.c_int32,
              C.c_void_p, C.c_int64, C.c_int64, C.POINTER(FnnBootStats)]


def bind_boot(a: Api) -> Api:
    """The bootstrap entry points of include/fastnn.h that draw their replicates themselves on `a`."""
    a._fn("bootstrap_distances_batch_f64", C.c_int32, _BOOT_ARGS)
    a._fn("bootstrap_distances_batch_device_f64", C.c_int32, _BOOT_ARGS)
    a._fn("bootstrap_draw_max_sites", C.c_int32, [])
    return a


def run_boot(a: Api, seq, n: int, L: int, lds: int, batch: int, seed: int, lead: int, out, ld: int, stride: int, m: FnnDistModel,
             device: int = 0, on_device: bool = False):
    """One bootstrap-distance call on raw addresses (seq: host memory; out: host memory, or device memory with on_device);
    m=None passes NULL.  Returns the stats (FnnBootStats)."""
    st = FnnBootStats()
    fn = a.bootstrap_distances_batch_device_f64 if on_device else a.bootstrap_distances_batch_f64
    a.check(fn(seq, n, L, lds, batch, seed & 0xFFFFFFFFFFFFFFFF, lead, dist_model_ref(m), device, out, ld, stride, C.byref(st)))
    return st


class FnnRangeStats(C.Structure):
    _fields_ = [("model", FnnDistModelStats), ("n_site_blocks", C.c_int64), ("n_site_blocks_dense", C.c_int64), ("reserved", C.c_int64 * 4)]

    def as_dict(self):
        return dict(self.model.as_dict(), n_site_blocks=self.n_site_blocks, n_site_blocks_dense=self.n_site_blocks_dense)


_RANGES_ARGS = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(FnnDistModel), C.c_int32, C.c_void_p,
                C.c_int64, C.c_int64, C.POINTER(FnnRangeStats)]
_PAIR_COUNTS_RANGES_ARGS = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64,
                            C.c_int64, C.POINTER(FnnRangeStats)]


def bind_ranges(a: Api) -> Api:
    """The entry points of include/fastnn.h whose problems are site ranges of one alignment on `a`."""
    a._fn("alignment_distances_ranges_f64", C.c_int32, _RANGES_ARGS)
    a._fn("alignment_distances_ranges_device_f64", C.c_int32, _RANGES_ARGS)
    a._fn("alignment_pair_counts_ranges_i64", C.c_int32, _PAIR_COUNTS_RANGES_ARGS)
    a._fn("alignment_pair_counts_ranges_device_i64", C.c_int32, _PAIR_COUNTS_RANGES_ARGS)
    return a


def run_ranges(a: Api, seq, n: int, L: int, lds: int, starts, ends, batch: int, out, ld: int, stride: int, m: FnnDistModel, device: int = 0,
               on_device: bool = False):
    """One range-distance call on raw addresses (seq, starts, ends: host memory, the bounds int64; out: host memory, or device
    memory with on_device); m=None passes NULL.  Returns the stats (FnnRangeStats)."""
    st = FnnRangeStats()
    fn = a.alignment_distances_ranges_device_f64 if on_device else a.alignment_distances_ranges_f64
    a.check(fn(seq, n, L, lds, starts, ends, batch, dist_model_ref(m), device, out, ld, stride, C.byref(st)))
    return st


def run_pair_counts_ranges(a: Api, seq, n: int, L: int, lds: int, starts, ends, batch: int, out, ld: int, stride: int, device: int = 0,
                           on_device: bool = False):
    """One pair-count call over ranges on raw addresses (out: int64, 16 per (i, j)).  Returns the stats (FnnRangeStats)."""
    st = FnnRangeStats()
    fn = a.alignment_pair_counts_ranges_device_i64 if on_device else a.alignment_pair_counts_ranges_i64
    a.check(fn(seq, n, L, lds, starts, ends, batch, device, out, ld, stride, C.byref(st)))
    return st


class FnnScanStats(C.Structure):
    _fields_ = [("boot", FnnBootStats), ("n_windows", C.c_int64), ("n_site_blocks", C.c_int64), ("n_site_blocks_dense", C.c_int64),
                ("n_host_chunks", C.c_int64), ("reserved", C.c_int64 * 4)]

    def as_dict(self):
        return dict(self.boot.as_dict(), n_windows=self.n_windows, n_site_blocks=self.n_site_blocks, n_site_blocks_dense=self.n_site_blocks_dense,
                    n_host_chunks=self.n_host_chunks)


_SCAN_ARGS = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_uint64, C.c_int64, C.POINTER(FnnDistModel),
              C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(FnnScanStats)]


def bind_scan(a: Api) -> Api:
    """The bootscan entry points of include/fastnn.h (bootstrap replicates inside every site range) on `a`."""
    a._fn("bootscan_counts", C.c_int32, [C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_uint64, C.c_int64, C.c_int64, C.c_void_p])
    a._fn("bootscan_distances_f64", C.c_int32, _SCAN_ARGS)
    a._fn("bootscan_distances_device_f64", C.c_int32, _SCAN_ARGS)
    a._fn("bootscan_pair_counts_i64", C.c_int32, _SCAN_ARGS)
    a._fn("bootscan_pair_counts_device_i64", C.c_int32, _SCAN_ARGS)
    return a


def run_bootscan_counts(a: Api, L: int, starts, ends, replicates: int, seed: int, lead: int = 0, first: int = 0, count=None) -> np.ndarray:
    """Rows first ... first + count - 1 (count=None: to the last) of the counts a bootscan stands for: uint16 (count, L)."""
    starts, ends = np.ascontiguousarray(starts, dtype=np.int64), np.ascontiguousarray(ends, dtype=np.int64)
    if starts.ndim != 1 or starts.shape != ends.shape:
        raise ValueError("starts and ends must be one-dimensional and of the same length")
    if count is None:
        count = len(starts) * (replicates + lead) - first
    counts = np.zeros((max(count, 0), max(L, 0)), dtype=np.uint16)
    a.check(a.bootscan_counts(L, starts.ctypes.data, ends.ctypes.data, len(starts), replicates, lead, seed & 0xFFFFFFFFFFFFFFFF, first, count,
                              counts.ctypes.data))
    return counts


def run_scan(a: Api, seq, n: int, L: int, lds: int, starts, ends, windows: int, replicates: int, seed: int, lead: int, out, ld: int, stride: int,
             m: FnnDistModel, device: int = 0, on_device: bool = False, tables: bool = False):
    """One bootscan call on raw addresses (seq, starts, ends: host memory, the bounds int64; out: host memory, or device memory
    with on_device; tables: the pair-count entries, out int64, 16 per (i, j)); m=None passes NULL.  Returns the stats
    (FnnScanStats)."""
    st = FnnScanStats()
    if tables:
        fn = a.bootscan_pair_counts_device_i64 if on_device else a.bootscan_pair_counts_i64
    else:
        fn = a.bootscan_distances_device_f64 if on_device else a.bootscan_distances_f64
    a.check(fn(seq, n, L, lds, starts, ends, windows, replicates, seed & 0xFFFFFFFFFFFFFFFF, lead, dist_model_ref(m), device, out, ld, stride, C.byref(st)))
    return st


class FnnSupportStats(C.Structure):
    _fields_ = [("n_problems", C.c_int64), ("n_records", C.c_int64), ("n_splits", C.c_int64),
                ("words", C.c_int32), ("route", C.c_int32), ("hash_retries", C.c_int32), ("chunks", C.c_int32),
                ("table_slots", C.c_int64), ("t_upload_s", C.c_double), ("t_kernel_s", C.c_double), ("t_total_s", C.c_double),
                ("reserved", C.c_int64 * 4)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


SUPPORT_ROUTES = ("kernel", "host")
_SUPPORT_ARGS = [C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_double, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                 C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(FnnSupportStats)]


def bind_support(a: Api) -> Api:
    """The split-support entry points of include/fastnn.h (the distinct splits of many problems, tallied) on `a`."""
    a._fn("split_support_max_n", C.c_int32, [])
    a._fn("split_support_min_work", C.c_int64, [])
    a._fn("split_support_f64", C.c_int32, _SUPPORT_ARGS)
    a._fn("split_support_device_f64", C.c_int32, _SUPPORT_ARGS)
    a._fn("split_keys", C.c_int32, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p])
    return a


def support_words(n: int) -> int:
    return (n + 63) // 64


def run_support(a: Api, n: int, batch: int, orders, weights, threshold: float, lead: int, capacity: int, device: int = 0,
                on_device: bool = False, fill: int = 0):
    """One split-support call on raw addresses (orders: host memory; weights: host memory, or device memory with on_device).
    The output arrays hold `capacity` rows and are filled with `fill` bytes first.  Returns (table, S, stats): the table's
    arrays keep all `capacity` rows; on failure FnnError carries them as `.table`."""
    words = support_words(max(n, 1))
    byte = np.uint8(fill & 0xFF)
    table = {"keys": np.full((capacity, words * 8), byte, dtype=np.uint8).view(np.uint64).reshape(capacity, words),
             "first_b": np.full((capacity, 8), byte, dtype=np.uint8).view(np.int64).reshape(capacity),
             "first_k": np.full((capacity, 8), byte, dtype=np.uint8).view(np.int64).reshape(capacity),
             "count": np.full((capacity, 8), byte, dtype=np.uint8).view(np.int64).reshape(capacity),
             "weight_sum": np.full((capacity, 8), byte, dtype=np.uint8).view(np.float64).reshape(capacity)}
    S = C.c_int64(-1)
    st = FnnSupportStats()
    fn = a.split_support_device_f64 if on_device else a.split_support_f64
    rc = fn(n, batch, orders, weights, threshold, lead, device, *(table[k].ctypes.data for k in ("keys", "first_b", "first_k", "count", "weight_sum")),
            capacity, C.addressof(S), C.byref(st))
    try:
        a.check(rc)
    except FnnError as e:
        e.table = table
        raise
    return table, S.value, st


def run_split_keys(a: Api, n: int, order, ks) -> np.ndarray:
    order = np.ascontiguousarray(order, dtype=np.int32)
    ks = np.ascontiguousarray(ks, dtype=np.int64)
    out = np.zeros((len(ks), support_words(max(n, 1))), dtype=np.uint64)
    a.check(a.split_keys(n, order.ctypes.data, ks.ctypes.data, len(ks), out.ctypes.data))
    return out


_lp = C.POINTER(C.c_int64)
_RAGGED_ARGS =[C.c_void_p, _lp, _ip, _lp, C.c_int64, C.POINTER(FnnOpts), _ip, C.c_void_p, _ip, C.POINTER(FnnBatchStats)]
_SPLITS_RAGGED_ARGS = [C.c_void_p, _lp, _ip, _lp, C.c_int64, _ip, C.c_int32, _dp, C.POINTER(FnnSwStats), C.POINTER(FnnSwBatchStats)]


def bind_ragged(a: Api) -> Api:
    """The ragged entry points of include/fastnn.h (problems of different sizes in one call) on `a`."""
    a._fn("canonical_order_ragged_f64", C.c_int32, _RAGGED_ARGS)
    a._fn("canonical_order_ragged_device_f64", C.c_int32, _RAGGED_ARGS)
    a._fn("split_weights_ragged_f64", C.c_int32, _SPLITS_RAGGED_ARGS)
    a._fn("split_weights_ragged_device_f64", C.c_int32, _SPLITS_RAGGED_ARGS)
    return a


def ragged_layout(offsets, ns, lds):
    """(offsets, n, ld) as the contiguous int64 / int32 / int64 arrays the ragged calls take; lds may be None."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    ns = np.ascontiguousarray(ns, dtype=np.int32)
    lds = None if lds is None else np.ascontiguousarray(lds, dtype=np.int64)
    if offsets.shape != ns.shape or offsets.ndim != 1 or (lds is not None and lds.shape != ns.shape):
        raise ValueError("offsets, n and ld must be one-dimensional arrays of one length")
    return offsets, ns, lds


def run_ragged(a: Api, D, offsets, ns, lds=None, validate: bool = False, device: int = 0, events: bool = False,
               on_device: bool = False, fill: int = 0):
    """One ragged order call; D = the base address (host memory, or device memory with on_device), problem b at
    D + 8 * offsets[b] with row stride lds[b] (None: ns[b]).  Returns (orders, events or None, nevents[batch], stats): orders and
    events are lists of per-problem views of the concatenated arrays; on failure FnnError carries the untouched
    concatenated output array as `.orders` (filled with `fill`)."""
    offsets, ns, lds = ragged_layout(offsets, ns, lds)
    batch = len(ns)
    pos = np.maximum(ns.astype(np.int64), 0)
    oo = np.concatenate([[0], np.cumsum(pos + 1)])
    eo = np.concatenate([[0], np.cumsum(pos)])
    orders = np.full(max(int(oo[-1]), 1), fill, dtype=np.int32)
    ev = np.zeros(max(int(eo[-1]), 1), dtype=EVENT_DTYPE) if events else None
    nev = np.full(batch, fill, dtype=np.int32)
    opts = FnnOpts()
    opts.device = device
    opts.validate = 1 if validate else 0
    st = FnnBatchStats()
    fn = a.canonical_order_ragged_device_f64 if on_device else a.canonical_order_ragged_f64
    rc = fn(D, offsets.ctypes.data_as(_lp), ns.ctypes.data_as(_ip), None if lds is None else lds.ctypes.data_as(_lp), batch,
            C.byref(opts), orders.ctypes.data_as(_ip), ev.ctypes.data if events else None, nev.ctypes.data_as(_ip), C.byref(st))
    try:
        a.check(rc)
    except FnnError as e:
        e.orders = orders
        raise
    return ([orders[oo[b]:oo[b + 1]] for b in range(batch)],
            [ev[eo[b]:eo[b + 1]] for b in range(batch)] if events else None, nev, st)


def run_splits_ragged(a: Api, D, offsets, ns, orders, lds=None, device: int = 0, on_device: bool = False,
                      allow_inexact: bool = False, fill: float = 0.0):
    """One ragged split-weight call; layout as run_ragged's, orders = one int32 array of ns[b] + 1 entries per problem.
    Returns (weights: list of per-problem views of the concatenated array, per-problem stats as a numpy record array, call
    stats); on failure FnnError carries the untouched concatenated output array as `.weights` (filled with `fill`)."""
    offsets, ns, lds = ragged_layout(offsets, ns, lds)
    batch = len(ns)
    if len(orders) != batch or any(len(o) != n + 1 for o, n in zip(orders, ns)):
        raise ValueError("orders must hold one array of n[b] + 1 entries per problem")
    cat = np.ascontiguousarray(np.concatenate([np.asarray(o, dtype=np.int32) for o in orders]) if batch else np.zeros(0, np.int32))
    pos = np.maximum(ns.astype(np.int64), 0)
    wo = np.concatenate([[0], np.cumsum(pos * (pos - 1) // 2)])
    w = np.full(max(int(wo[-1]), 1), fill, dtype=np.float64)
    sw = (FnnSwStats * max(batch, 1))()
    st = FnnSwBatchStats()
    fn = a.split_weights_ragged_device_f64 if on_device else a.split_weights_ragged_f64
    rc = fn(D, offsets.ctypes.data_as(_lp), ns.ctypes.data_as(_ip), None if lds is None else lds.ctypes.data_as(_lp), batch,
            cat.ctypes.data_as(_ip), device, w.ctypes.data_as(_dp), sw, C.byref(st))
    if rc == -7 and allow_inexact:   # FNN_EINEXACT: the weights are there; stats say which problems failed their check
        rc = 0
    try:
        a.check(rc)
    except FnnError as e:
        e.weights = w
        raise
    return [w[wo[b]:wo[b + 1]] for b in range(batch)], np.ctypeslib.as_array(sw)[:batch].copy(), st


class Handle:
    """Thin RAII wrapper over an engine handle of either library."""

    def __init__(self, api: Api, n: int, device: int = 0, validate: bool = False,
                 record_events: bool = False, force_exact_rx: bool = False, disable_screen: bool = False,
                 lookahead: int = 0, lookahead_pairs: int = 0, relaxed_seed=None, relaxed_min_active: int = 0):
        self.api = api
        self.n = int(n)
        opts = FnnOpts()
        opts.device = device
        opts.validate = 1 if validate else 0
        opts.record_events = 1 if record_events else 0
        opts.force_exact_rx = 1 if force_exact_rx else 0
        opts.disable_screen = 1 if disable_screen else 0
        opts.lookahead = lookahead
        opts.lookahead_pairs = lookahead_pairs
        if relaxed_seed is not None:  # -mode Relaxed (NeighborNetLocal) with java.util.Random(relaxed_seed)
            opts.mode = 1
            opts.relaxed_seed_lo = int(relaxed_seed) & 0xFFFFFFFF
            opts.relaxed_seed_hi = (int(relaxed_seed) >> 32) & 0xFFFFFFFF
            opts.relaxed_min_active = relaxed_min_active
        h = C.c_void_p()
        api.check(api.create(self.n, C.byref(opts), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self.api.destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- several ranks --
    def comm_init_host(self, world: int, rank: int, allgather):
        """Test transport: `allgather(send: bytes) -> list[bytes]` (one entry per rank)."""
        def _cb(ctx, send, recv, nbytes):
            try:
                parts = allgather(C.string_at(send, nbytes))
                C.memmove(recv, b"".join(parts), nbytes * world)
                return 0
            except Exception:  # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return 1
        self._cb = ALLGATHER_FN(_cb)  # keep alive
        self.api.check(self.api.comm_init_host(self._h, world, rank, self._cb, None))

    def comm_init_rccl(self, world: int, rank: int, uid: bytes, rccl_path: str | None = None):
        p = rccl_path.encode() if rccl_path else None
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        self.api.check(self.api.comm_init_rccl(self._h, world, rank, buf, p))

    # -- matrix --
    def set_matrix(self, D: np.ndarray, chunk_rows: int = 0):
        D = np.ascontiguousarray(D, dtype=np.float64)
        if D.shape != (self.n, self.n):
            raise ValueError(f"matrix must be {self.n} x {self.n}")
        step = chunk_rows if chunk_rows > 0 else max(self.n, 1)
        for r0 in range(0, self.n, step):
            cnt = min(step, self.n - r0)
            self.api.check(self.api.set_rows(self._h, r0, cnt, D[r0:].ctypes.data_as(_dp), self.n))

    def set_packed_upper(self, packed: np.ndarray):
        """DistancesAndNames.distances: the strict upper triangle, row-major (DistancesAndNames.java:24-38)."""
        packed = np.ascontiguousarray(packed, dtype=np.float64)
        if packed.shape != (self.n * (self.n - 1) // 2,):
            raise ValueError(f"packed triangle must have {self.n * (self.n - 1) // 2} entries")
        self.api.check(self.api.set_packed_upper(self._h, packed.ctypes.data_as(_dp)))

    def synth(self, seed: int, dist: str = "uniform53"):
        self.api.check(self.api.synth(self._h, seed, {"uniform53": 0, "dec4": 1}[dist]))

    # -- run --
    def run(self):
        order = np.zeros(self.n + 1, dtype=np.int32)
        st = FnnStats()
        self.api.check(self.api.run(self._h, order.ctypes.data_as(_ip), C.byref(st)))
        return order, st

    def begin(self):
        self.api.check(self.api.begin(self._h))

    def step(self):
        ev = FnnEvent()
        r = self.api.check(self.api.step(self._h, C.byref(ev)))
        return ev if r == 1 else None

    def finish(self):
        order = np.zeros(self.n + 1, dtype=np.int32)
        self.api.check(self.api.finish(self._h, order.ctypes.data_as(_ip)))
        return order

    def events(self) -> np.ndarray:
        k = self.api.get_events(self._h, None, 0)
        out = np.zeros(max(k, 1), dtype=EVENT_DTYPE)
        self.api.get_events(self._h, out.ctypes.data, k)
        return out[:k]

    def counts(self):
        m, c, nn = C.c_int32(), C.c_int32(), C.c_int32()
        self.api.check(self.api.get_counts(self._h, C.byref(m), C.byref(c), C.byref(nn)))
        return m.value, c.value, nn.value

    def nodes(self):
        m, _, _ = self.counts()
        ids = np.zeros(max(self.n, 1), np.int32)
        nbr = np.zeros(max(self.n, 1), np.int32)
        sx = np.zeros(max(self.n, 1), np.float64)
        self.api.check(self.api.get_nodes(self._h, ids.ctypes.data_as(_ip), nbr.ctypes.data_as(_ip),
                                          sx.ctypes.data_as(_dp)))
        return ids[:m], nbr[:m], sx[:m]

    def matrix(self) -> np.ndarray:
        """The resident n x n matrix (after set_matrix / synth, before run consumes it) - fnn_get_matrix."""
        out = np.empty((self.n, self.n), dtype=np.float64)
        self.api.check(self.api.get_matrix(self._h, out.ctypes.data_as(_dp), self.n))
        return out

    def live_matrix(self) -> np.ndarray:
        m, _, _ = self.counts()
        out = np.zeros((m, m), dtype=np.float64)
        self.api.check(self.api.get_live_matrix(self._h, out.ctypes.data_as(_dp)))
        return out

"""Later runs on one engine handle must equal a run on a fresh handle.

Every other parity test creates a handle, runs it once and destroys it, so it reads freshly allocated memory.  Production does
not: bench.py warms up and times on one handle, the batch calls loop their out-of-range problems over one handle, the JNI class
keeps one.  Engine::begin() (fnn_engine.h) is all that separates two runs: it rebuilds State and refills only the buffers of
buffers() with fill >= 0; Sx, the layout arrays, the chain buffers, the screening records, the window lists, the event logs, the
bf16 copy and the padding of D stay as the previous run left them, and so does some host state (screen_off, m_bound, the window
schedule).  That is safe only while no kernel reads a word it did not write in this run.

`life_cycle` takes ONE handle through input classes that leave very different leftovers (exact ties, negative entries that switch
the run to plain fp64 scans, zero distances, a run abandoned after n // 3 events, a run refused by validation, a huge outgroup),
whole runs and stepped runs, every one compared with the oracle event by event, and ends on the first matrix again: the same
bytes as the first run.  The CPU part runs it on the emulation (tests/emu), also with every allocation of the emulated backend
pre-filled with a poison byte (FNN_EMU_POISON); the GPU part runs it on the product.  The sizes are the smallest at which
windows, screening, rescans and the end game all occur once screening is forced on (FNN_SCREEN_MIN_N / FNN_SCREEN_MIN_M = 8);
one GPU sequence runs 4096 taxa at the default thresholds against the committed goldens.
"""
import contextlib
import functools
import json
import os

import numpy as np
import pytest

import inputs
from common import bits, compare_trajectory
from fastneighbornet_amd._capi import FnnError, Handle

INT_FIELDS = ("m_before", "c_before", "cx_id", "cy_id", "x_id", "y_id", "kind", "u_id", "entries")
COUNTERS = ("n_window_hits", "n_screen_events", "n_base_scans", "n_rescan_units", "n_rx_exact",
            # (the host's schedule of the base scans shows in these two: a window schedule left over from the run before stalls)
            "n_window_fails", "n_stalled_events")
SIZES = (65, 200, 300)
POISON = (None, 0x00, 0xFF, 0xA5, 0x7F)
EINVAL, ESTATE, ECAPACITY = -1, -5, -6
RELAXED_SEED, RELAXED_MIN_ACTIVE, RL_TIES = 4242, 16, 16


def is_gpu(api):
    return api.prefix == "fnn_"


@contextlib.contextmanager
def environment(**kv):
    """os.environ with the given variables set (None: removed) for the duration of the block."""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def plain_neg(api):
    """The environment in which begin() switches a run on a matrix with negative entries to plain fp64 scans (screen_off), as
    production does.  begin() keeps the screening pass for such a matrix while FNN_SCREEN_MIN_N / FNN_SCREEN_MIN_M are set (the
    backend has read their values when the handle was created; begin() only asks whether they exist), and the emulation keeps it
    unless FNN_EMU_PLAIN_NEG is set.  Without this the host state this test is about would never change."""
    if is_gpu(api):
        return environment(FNN_SCREEN_MIN_N=None, FNN_SCREEN_MIN_M=None)
    return environment(FNN_EMU_PLAIN_NEG="1")


class Ref:
    """A matrix with the oracle's result.  Computed once per (n, name), shared by every test, never written."""

    def __init__(self, D, order, ev, sum_entries):
        D.setflags(write=False)
        self.D, self.order, self.ev, self.sum_entries = D, order, ev, sum_entries


@functools.lru_cache(maxsize=None)
def refs(n):
    from oracle import nnet_oracle as O
    O.lib()
    out = {}
    for name, dist, seed in [("u1", "uniform53", 1), ("tree", "tree", 2), ("neg", "neg", 3), ("dup", "dup", 4),
                             ("u2", "uniform53", 6), ("outgroup", "outgroup", 8), ("dec4", "dec4", 9)]:
        D = inputs.make(n, dist, seed, O)
        out[name] = Ref(D, *O.run(D))
    assert (out["neg"].D < 0).any() and (out["dup"].D[np.triu_indices(n, 1)] == 0).any()
    A = inputs.make(n, "uniform53", 7, O)
    A[n // 2, n // 3] += 2.0 ** -30           # one asymmetric entry: validation refuses the run
    A.setflags(write=False)
    out["asym"] = A
    out["abandon"] = inputs.make(n, "dec4", 5, O)
    out["abandon"].setflags(write=False)
    return out


def assert_events(ev, ref_ev, tag):
    assert len(ev) == len(ref_ev), (tag, len(ev), len(ref_ev))
    for f in INT_FIELDS:
        bad = np.nonzero(ev[f] != ref_ev[f])[0]
        assert bad.size == 0, f"{tag}: {f} differs first at event {bad[0]}: {ev[f][bad[0]]} vs oracle {ref_ev[f][bad[0]]}"
    bad = np.nonzero(bits(ev["best"]) != bits(ref_ev["best"]))[0]
    assert bad.size == 0, f"{tag}: best differs first at event {bad[0]}: {ev['best'][bad[0]]!r} vs oracle {ref_ev['best'][bad[0]]!r}"


def checked_run(h, ref, tag, upload=None):
    """fnn_run on the matrix of `ref` (uploaded by `upload(h)`, default set_matrix): order, n_events, sum_entries, every field of
    every event and the bits of best as the oracle gives them; fnn_get_events holds exactly this run's events; on the GPU no
    hand-over between launch sequences was retried.  Returns (order, event bytes, stats)."""
    if upload is None:
        h.set_matrix(ref.D)
    else:
        upload(h)
    order, st = h.run()
    ev = h.events()
    assert (order == ref.order).all(), (tag, order, ref.order)
    assert h.api.get_events(h._h, None, 0) == len(ref.ev) == st.n_events, (tag, st.n_events, len(ref.ev))
    assert st.sum_entries == ref.sum_entries, (tag, st.sum_entries, ref.sum_entries)
    assert_events(ev, ref.ev, tag)
    if is_gpu(h.api):
        assert st.n_handover_retries == 0, (tag, st.n_handover_retries)
    return order, ev.tobytes(), st


def stepped_run(h, oracle, ref, tag, **stepper_kw):
    """begin / step / finish on the existing handle against the oracle's stepper, with the deep comparison (node ids, partners,
    Sx bits, live matrix bits) after every 7th event; the events the handle then holds are this run's."""
    k, order = compare_trajectory(h.api, oracle, ref.D, deep=True, deep_every=7, handle=h, **stepper_kw)
    assert k == len(ref.ev) and (order == ref.order).all(), tag
    assert_events(h.events(), ref.ev, tag)


def refuse(h, A, call):
    h.set_matrix(A)
    with pytest.raises(FnnError) as ei:
        call()
    assert ei.value.code == EINVAL, ei.value


def abandon(h, D, n):
    h.set_matrix(D)
    h.begin()
    for _ in range(n // 3):
        assert h.step() is not None
    assert len(h.events()) == 0    # begin() dropped the previous run's events; this run never finished


def counters(st):
    return {k: getattr(st, k) for k in COUNTERS}


def life_cycle(api, oracle, n, **handle_kw):
    """The sequence of the module docstring on one handle.  Returns the counters of the first and the last run."""
    gpu = is_gpu(api)
    R = refs(n)
    with Handle(api, n, record_events=True, validate=True, **handle_kw) as h:
        # 1
        order1, bytes1, st1 = checked_run(h, R["u1"], "1 uniform53")
        assert st1.n_window_hits > 0 and st1.n_screen_events > 0, "this size no longer opens windows: the test checks nothing"
        # 2-6: whole runs
        checked_run(h, R["tree"], "2 tree")
        with plain_neg(api):
            _, _, st = checked_run(h, R["neg"], "3 neg")
        assert st.n_screen_events == 0 and st.n_window_hits == 0, ("3 neg", counters(st))
        checked_run(h, R["dup"], "4 dup")
        abandon(h, R["abandon"], n)
        _, _, st = checked_run(h, R["u2"], "5 uniform53 after an abandoned run")
        assert st.n_window_hits > 0, "screen_off stuck after the run on negative entries"
        refuse(h, R["asym"], h.run)
        checked_run(h, R["outgroup"], "6 outgroup after a refused run")
        # 7: the same through begin / step / finish
        stepped_run(h, oracle, R["tree"], "7.2 tree")
        with plain_neg(api):
            stepped_run(h, oracle, R["neg"], "7.3 neg")
        stepped_run(h, oracle, R["dup"], "7.4 dup")
        abandon(h, R["abandon"], n)
        stepped_run(h, oracle, R["u2"], "7.5 uniform53 after an abandoned run")
        refuse(h, R["asym"], h.begin)
        stepped_run(h, oracle, R["outgroup"], "7.6 outgroup after a refused run")
        # 8
        order8, bytes8, st8 = checked_run(h, R["u1"], "8 uniform53 again")
        assert (order8 == order1).all() and bytes8 == bytes1
        assert st8.n_events == st1.n_events and st8.sum_entries == st1.sum_entries
        c1, c8 = counters(st1), counters(st8)
        if gpu:   # (nobody has shown that these are independent of timing on the GPU: recorded, not compared)
            print(json.dumps({"n": n, "opts": {k: bool(v) for k, v in handle_kw.items()}, "first_run": c1, "last_run": c8}))
        else:
            assert c1 == c8, (c1, c8)
        return c1, c8


def upload_routes(api, oracle, n):
    """The other ways a matrix gets into a handle that has already run: the packed upper triangle, the device generator and
    row chunks; and a run without a new matrix, which is FNN_ESTATE and leaves the handle usable."""
    R = refs(n)
    with Handle(api, n, record_events=True, validate=True) as h:
        checked_run(h, R["u1"], "full run")
        T = R["tree"]
        checked_run(h, T, "packed upper", lambda h: h.set_packed_upper(T.D[np.triu_indices(n, 1)]))

        def synth(h):
            h.synth(9, "dec4")
            assert (bits(h.matrix()) == bits(R["dec4"].D)).all()
        checked_run(h, R["dec4"], "synth", synth)
        checked_run(h, R["outgroup"], "row chunks", lambda h: h.set_matrix(R["outgroup"].D, chunk_rows=17))
        for call in (h.run, h.begin):
            with pytest.raises(FnnError) as ei:
                call()
            assert ei.value.code == ESTATE, ei.value
        checked_run(h, R["dup"], "after FNN_ESTATE")


@functools.lru_cache(maxsize=None)
def relaxed_refs(n):
    from oracle import nnet_oracle as O
    O.lib()
    out = {}
    for name, dist, seed in [("a", "uniform53", 11), ("b", "dec4", 12), ("c", "tree", 13)]:
        D = inputs.make(n, dist, seed, O)
        order, ev = O.run_relaxed(D, RELAXED_SEED, RELAXED_MIN_ACTIVE)
        out[name] = Ref(D, order, ev, int(ev["entries"].sum()))
    D18 = inputs.dupk(n, 18, 31, O)     # the refusing input of tests/test_relaxed_ties.py at this size: 17 tied row minima
    assert max(len(t) for t in inputs.first_event_ties(D18)) == RL_TIES + 1
    D18.setflags(write=False)
    out["refused"] = D18
    return out


def relaxed_life_cycle(api, oracle, n):
    R = relaxed_refs(n)
    kw = dict(relaxed_seed=RELAXED_SEED, relaxed_min_active=RELAXED_MIN_ACTIVE)
    with Handle(api, n, record_events=True, validate=True, **kw) as h:
        order1, bytes1, _ = checked_run(h, R["a"], "relaxed a")
        checked_run(h, R["b"], "relaxed b")
        h.set_matrix(R["refused"])
        with pytest.raises(FnnError) as ei:
            h.run()
        assert ei.value.code == ECAPACITY, ei.value
        checked_run(h, R["c"], "relaxed c after FNN_ECAPACITY")
        stepped_run(h, oracle, R["b"], "relaxed b stepped", **kw)
        order5, bytes5, _ = checked_run(h, R["a"], "relaxed a again")
        assert (order5 == order1).all() and bytes5 == bytes1


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the emulation, whose allocations can start poisoned.  FNN_EMU_POISON is read at every allocation, so setting it before the
# handle is created is enough.

@pytest.fixture
def poisoned(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv("FNN_EMU_POISON", raising=False)
    else:
        monkeypatch.setenv("FNN_EMU_POISON", hex(request.param))
    return request.param


poison_ids = dict(argnames="poisoned", argvalues=POISON, indirect=True, ids=lambda p: "malloc" if p is None else f"{p:#04x}")


def test_emulation_poison_reaches_the_buffers(emu_api, oracle, monkeypatch):
    """(the premise of the poisoned cases) a block from the emulated backend's allocator starts filled with the byte named."""
    import ctypes as C
    lib = emu_api.lib
    monkeypatch.setenv("FNN_EMU_POISON", "0xA5")
    for fn, res in (("emu_debug_alloc", C.c_void_p), ("emu_debug_free", None)):
        getattr(lib, fn).restype = res
    lib.emu_debug_alloc.argtypes = [C.c_size_t]
    lib.emu_debug_free.argtypes = [C.c_void_p]
    p = lib.emu_debug_alloc(4096)
    try:
        assert C.string_at(p, 4096) == b"\xA5" * 4096
    finally:
        lib.emu_debug_free(p)
    monkeypatch.setenv("FNN_EMU_POISON", "0x7F")
    p = lib.emu_debug_alloc(1)
    try:
        assert C.string_at(p, 1) == b"\x7F"
    finally:
        lib.emu_debug_free(p)


@pytest.mark.parametrize(**poison_ids)
@pytest.mark.parametrize("exact", [False, True], ids=["default", "force_exact_rx"])
@pytest.mark.parametrize("n", SIZES)
def test_emulation_life_cycle(emu_api, oracle, n, exact, poisoned):
    emu_api.set_order_mode(1 if exact else 0)    # (a fixed thread order: the counters of the first and the last run are compared)
    life_cycle(emu_api, oracle, n, force_exact_rx=exact)


@pytest.mark.parametrize(**poison_ids)
@pytest.mark.parametrize("n", SIZES[1:])
def test_emulation_relaxed_life_cycle(emu_api, oracle, n, poisoned):
    emu_api.set_order_mode(0)
    relaxed_life_cycle(emu_api, oracle, n)


@pytest.mark.parametrize(**poison_ids)
@pytest.mark.parametrize("n", SIZES)
def test_emulation_upload_routes(emu_api, oracle, n, poisoned):
    emu_api.set_order_mode(0)
    upload_routes(emu_api, oracle, n)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the product.  The backend reads the thresholds when the handle is created, so the environment is set before that.

@pytest.fixture
def forced_screening(monkeypatch):
    monkeypatch.setenv("FNN_SCREEN_MIN_N", "8")
    monkeypatch.setenv("FNN_SCREEN_MIN_M", "8")


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [False, True], ids=["default", "force_exact_rx"])
@pytest.mark.parametrize("n", SIZES)
def test_gpu_life_cycle(hip_api, oracle, forced_screening, n, exact):
    life_cycle(hip_api, oracle, n, force_exact_rx=exact)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES[1:])
def test_gpu_relaxed_life_cycle(hip_api, oracle, n):
    relaxed_life_cycle(hip_api, oracle, n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_gpu_upload_routes(hip_api, oracle, forced_screening, n):
    upload_routes(hip_api, oracle, n)


@pytest.mark.gpu
def test_gpu_life_cycle_at_default_thresholds(hip_api, oracle, monkeypatch):
    """4096 taxa, no environment switches: the goldens uniform53, tree, neg (plain fp64 scans), dup and uniform53 again on one
    handle.  The last run's event bytes are the first run's."""
    import time
    from test_value_range import check_against_golden, golden
    for v in ("FNN_SCREEN_MIN_N", "FNN_SCREEN_MIN_M"):
        monkeypatch.delenv(v, raising=False)
    n = 4096
    first = None
    t0 = time.perf_counter()
    with Handle(hip_api, n, record_events=True, validate=True) as h:
        for dist, seed in [("uniform53", 1), ("tree", 5), ("neg", 1), ("dup", 16), ("uniform53", 1)]:
            c, z = golden(n, dist, seed)
            D = inputs.make(n, dist, seed, oracle)
            assert inputs.sha_big(D) == c["matrix_sha256"], "the input generator drifted from the committed golden"
            h.set_matrix(D)
            del D
            order, st = h.run()
            ev = h.events()
            print(json.dumps({"n": n, "dist": dist, "seed": seed, "t_total_s": round(st.t_total_s, 3), **counters(st)}))
            check_against_golden(ev, order, st.n_events, st.sum_entries, c, z, k=0)
            assert st.n_handover_retries == 0
            if dist == "neg":
                assert st.n_screen_events == 0 and st.n_window_hits == 0
            else:
                assert st.n_screen_events > 0 and st.n_window_hits > 0, "screen_off stuck, or the default mode did not run"
            if first is None:
                first = (order, ev.tobytes())
        assert (order == first[0]).all() and ev.tobytes() == first[1]
    print(json.dumps({"n": n, "sequence_s": round(time.perf_counter() - t0, 2)}))

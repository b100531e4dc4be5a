"""The batched circular split weights (fnn_small_splits.h) on the CPU: the per-thread phase bodies run
for tid = 0 ... nthreads-1, phase by phase, by tests/emu/fnn_splits_batch_emu.cpp under the product's own sequence and host
logic; and the stand-alone AddressSanitizer / UBSan program over the same driver.  The driver has no one-problem solver
behind it, so every case here is solved by the kernel's own method or fails."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import splits_batch_common as sc
from fastneighbornet_amd import _capi


@pytest.fixture(scope="module")
def a():
    return sc.emu_api()


@pytest.fixture(autouse=True)
def kernel_route(monkeypatch):
    """Every case here is for the kernel's method, also below the batch from which the call takes it by default."""
    monkeypatch.setenv("FNN_SW_BATCH_ROUTE", "kernel")


@pytest.fixture(scope="module")
def call(a):
    return lambda D, orders, **kw: sc.run(a, np.ascontiguousarray(D), orders, **kw)


def test_max_n(a):
    assert a.split_weights_batch_max_n() >= 140   # fnn_batch_lds_max_n(): test_python_entry_fails_loudly_without_device compares the two
    assert [a.split_weights_batch_min_batch(n) for n in (2, 32, 33, 64, 96, 128, 140)] == [1, 1, 4, 4, 8, 16, 32]


def test_default_route_below_the_crossover(a, call, monkeypatch):
    """Fewer problems than fnn_split_weights_batch_min_batch(n) go to the one-problem solver, which the CPU driver lacks."""
    monkeypatch.delenv("FNN_SW_BATCH_ROUTE")
    D, orders = sc.synth_batch(64, 4)
    _, _, st = call(D, orders)
    assert st.n_kernel == 4 and st.n_fallback == 0
    with pytest.raises(_capi.FnnError) as ei:
        call(D[:3], orders[:3])
    assert ei.value.code == -6 and "problem 0:" in str(ei.value)
    monkeypatch.setenv("FNN_SW_BATCH_ROUTE", "loop")
    with pytest.raises(_capi.FnnError) as ei:
        call(D, orders)
    assert ei.value.code == -6


@pytest.mark.parametrize("n", [2, 3, 4, 5, 9, 33, 64, 65, "max_n"])
def test_parity(a, call, n):
    pytest.importorskip("scipy")
    mx = a.split_weights_batch_max_n()
    sc.check_parity(call, mx if n == "max_n" else n, mx)


def test_closed_form_route(call):
    sc.check_closed_form(call)


def test_zeros_to_find(call):
    sc.check_zeros_to_find(call)


@pytest.mark.parametrize("n", [16, 64])
def test_tree_metric_with_degenerate_multipliers(call, n):
    sc.check_tree_metric(call, n)


def test_capacity_give_up(a, call, monkeypatch):
    """FNN_SW_BATCH_CAP=8 at n = 12: problems whose free set outgrows 8 splits give up; without a one-problem solver the call
    fails with FNN_ECAPACITY naming the lowest of them, outputs untouched."""
    D, orders = sc.synth_batch(12, 6)
    w0, sw0, _ = call(D, orders)
    need = sw0["free_set_peak"] > 8
    assert need.any(), sw0["free_set_peak"]
    monkeypatch.setenv("FNN_SW_BATCH_CAP", "8")
    with pytest.raises(_capi.FnnError) as ei:
        call(D, orders, fill=sc.SENTINEL)
    monkeypatch.delenv("FNN_SW_BATCH_CAP")
    assert ei.value.code == -6, ei.value
    assert f"problem {int(np.flatnonzero(need)[0])}:" in str(ei.value), (ei.value, need)
    assert (ei.value.weights == sc.SENTINEL).all()
    got = (C.c_int32 * 6)()
    assert a.split_weights_batch_giveups(got, 6) == 6
    assert [g == sc.GIVEUP_CAPACITY for g in got] == need.tolist(), (list(got), need)


@pytest.mark.parametrize("n", [9, 64])
def test_padding_is_never_read(a, n):
    def a_run(buf, n_, ld, stride, B, orders):
        return _capi.run_splits_batch(a, buf.ctypes.data, n_, ld, stride, B, orders)
    sc.check_padding(a_run, n, a.split_weights_batch_max_n())


@pytest.mark.parametrize("n", [9, 65])
def test_chunking(call, n, monkeypatch):
    sc.check_chunking(call, n, monkeypatch)


def test_determinism(call):
    sc.check_determinism(call, 33)


def test_in_place_entry(a, call):
    D, orders = sc.synth_batch(33, 6)
    w0, _, _ = call(D, orders)
    w1, _, st = call(D, orders, on_device=True)
    assert w0.tobytes() == w1.tobytes() and st.n_fallback == 0


def test_arguments(a, call):
    n, B = 10, 4
    D, orders = sc.synth_batch(n, B)
    w, sw, st = sc.run(a, np.zeros((0, n, n)), np.zeros((0, n + 1), dtype=np.int32))       # batch == 0 is FNN_OK
    assert w.shape == (0, n * (n - 1) // 2) and st.n_problems == 0
    with pytest.raises(_capi.FnnError) as ei:                                                # n = 1
        sc.run(a, np.zeros((2, 1, 1)), np.tile(np.arange(2, dtype=np.int32), (2, 1)))
    assert ei.value.code == -1
    with pytest.raises(_capi.FnnError) as ei:                                                # ld < n
        _capi.run_splits_batch(a, np.ascontiguousarray(D).ctypes.data, n, n - 1, n * n, B, orders)
    assert ei.value.code == -1
    bad = orders.copy()
    bad[2, 4] = bad[2, 5]                                                                    # a repeated taxon in problem 2 of 4
    with pytest.raises(_capi.FnnError) as ei:
        call(D, bad, fill=sc.SENTINEL)
    assert ei.value.code == -1 and "problem 2:" in str(ei.value), ei.value
    assert (ei.value.weights == sc.SENTINEL).all()
    E = D.copy()
    i, j = int(orders[2, 3]) - 1, int(orders[2, 7]) - 1                                      # a selected entry of problem 2: the upper
    E[2, min(i, j), max(i, j)] = E[2, max(i, j), min(i, j)] = np.nan                         # or the lower copy, whichever the order reads
    with pytest.raises(_capi.FnnError) as ei:
        call(E, orders, fill=sc.SENTINEL)
    assert ei.value.code == -1 and "problem 2:" in str(ei.value), ei.value
    assert (ei.value.weights == sc.SENTINEL).all()
    E = D.copy()
    E[:, np.arange(n), np.arange(n)] = np.nan                                                # the diagonal is never selected
    w1, _, _ = call(E, orders)
    w0, _, _ = call(D, orders)
    assert w0.tobytes() == w1.tobytes()


def test_python_entry_fails_loudly_without_device():
    """No CPU fallback: without a HIP device the product's batch call fails with FNN_EHIP; arguments are checked first."""
    import fastneighbornet_amd as fa
    api = fa.api()
    assert api.split_weights_batch_max_n() >= api.batch_lds_max_n()
    D, orders = sc.synth_batch(9, 6)
    w, st = fa.split_weights_batch(np.zeros((0, 9, 9)), np.zeros((0, 10), dtype=np.int32))
    assert w.shape == (0, 36) and st["call"]["n_problems"] == 0
    if api.device_count() < 1:
        with pytest.raises(_capi.FnnError) as ei:
            fa.split_weights_batch(D, orders)
        assert ei.value.code == -3


def test_standalone_program_under_asan_ubsan(a):
    """tests/emu/fnn_splits_batch_emu_main.cpp with -fsanitize=address,undefined, as a program of its own (no sanitizer runtime
    is loaded into the interpreter), over n = 4, 33, 64 and the limit."""
    exe = os.path.join(sc.EMU_DIR, "build", "fnn_splits_batch_emu_main_asan")
    srcs = [os.path.join(sc.EMU_DIR, "fnn_splits_batch_emu_main.cpp")] + sc.EMU_SRCS
    if sc.newer(exe, srcs):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g", "-O1", "-o", exe, srcs[0], srcs[1]])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, "4", "33", "64", str(a.split_weights_batch_max_n())], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.startswith("ok: ")


# ---- the safety net, through the test switches (splits_batch_common) ----------------------------------------------------

@pytest.fixture(scope="module")
def solve(a):
    return sc.emu_solver(a)


def test_switches_ignore_values_outside_their_range(call, monkeypatch):
    D, orders = sc.synth_batch(12, 6)
    w0, sw0, _ = call(D, orders)
    for dep, steps in (("0", "0"), ("1", "-3"), ("-0.5", "x"), ("nan", ""), ("1e-9", str(40 * 12 + 1000))):
        monkeypatch.setenv("FNN_SW_BATCH_DEP", dep)
        monkeypatch.setenv("FNN_SW_BATCH_STEPS", steps)
        w, sw, _ = call(D, orders)
        assert w.tobytes() == w0.tobytes() and (sw["outer_iterations"] == sw0["outer_iterations"]).all(), (dep, steps)


def test_set_aside_release_and_recheck(solve, monkeypatch):
    pytest.importorskip("scipy")
    n_solved, n_all, total = sc.check_set_aside(solve, None, monkeypatch)
    assert (n_solved, n_all) == (35, 40), (n_solved, n_all)   # the share the GPU case compares with


def test_give_up_by_steps(a, solve, monkeypatch):
    D, orders, steps = sc.check_step_limit(solve, None, monkeypatch)
    # every limit below a problem's own step count, so that the limit falls on a pick and on a ratio step (both sites count)
    b = 2
    w0, sw0, _ = sc.run(a, D[b: b + 1], orders[b: b + 1])
    assert sw0["departed"][0] > 0 and sw0["reserved"][0][2] == steps[b]
    for L in range(1, int(steps[b]) + 1):
        monkeypatch.setenv("FNN_SW_BATCH_STEPS", str(L))
        w, sw, g = sc.emu_solve(a, D[b: b + 1], orders[b: b + 1])
        assert g[0] == (sc.GIVEUP_STEPS if L < steps[b] else 0), (L, g)
        assert L < steps[b] or w.tobytes() == w0.tobytes()


def test_give_up_uncertified(solve, monkeypatch):
    pytest.importorskip("scipy")
    sc.check_uncertified_end(solve, None, monkeypatch)


@pytest.mark.parametrize("n", [8, 33, 64, 65, 96, 97, "max_n"])
def test_input_classes(a, call, n):
    pytest.importorskip("scipy")
    sc.check_classes(call, a.split_weights_batch_max_n() if n == "max_n" else n)


@pytest.mark.parametrize("n", [33, 65])
def test_foreign_orderings(call, n):
    pytest.importorskip("scipy")
    sc.check_foreign_orderings(call, n)


@pytest.mark.parametrize("n", [2, 3, 8, 65])
def test_constant_and_zero_matrices(call, n):
    sc.check_flat(call, n)


@pytest.mark.parametrize("n", [33, 65])
def test_power_of_two_scaling_is_exact(call, n):
    sc.check_power_of_two(call, n)

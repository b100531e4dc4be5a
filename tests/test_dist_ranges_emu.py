"""Alignment distances over site ranges (fnn_dist_ranges.h) on the CPU: the cases of
tests/dist_ranges_common.py through tests/emu/fnn_dist_ranges_emu.cpp, which runs the per-lane steps for lane = 0 ... 63 of every
wave under the product's host logic, bitwise against the existing references on the 0/1 counts of the ranges and against the
driver's own counts entries; the argument checks also against the product library (they need no device); the Python wrappers'
checks; and the stand-alone AddressSanitizer / UBSan program."""
import inspect
import os
import subprocess

import numpy as np
import pytest

import dist_common as dc
import dist_ranges_common as rc

GRID = [pytest.param(m, s, id=name) for (m, s), name in zip(rc.GRID_MODELS, rc.GRID_MODEL_NAMES)]


@pytest.fixture(scope="module")
def a():
    return rc.emu_dist_ranges_api()


@pytest.fixture(scope="module", params=["driver", "product"])
def either(request):
    if request.param == "driver":
        return rc.emu_dist_ranges_api()
    import fastneighbornet_amd as fa
    return fa.api()


def test_range_operand_every_k(a):
    rc.check_operand(a, also_counts=True)


@pytest.mark.parametrize("model,shape", GRID)
@pytest.mark.parametrize("missing", [False, True])
@pytest.mark.parametrize("k", range(len(rc.GRIDS)), ids=rc.GRID_NAMES)
def test_grids(a, k, missing, model, shape):
    rc.check_grid(a, k, missing, model, shape)


@pytest.mark.parametrize("model,shape", [GRID[0], GRID[2], GRID[8], GRID[9]])
def test_grid_against_the_counts_entry(a, model, shape):
    rc.check_grid(a, 0, True, model, shape, also_counts=True)


def test_order_and_spans(a):
    rc.check_order_and_spans(a, also_counts=True)


def test_long_walk(a):
    rc.check_long_walk(a)


def test_failures(either):
    rc.check_failures(either, also_counts=either.prefix != "fnn_")


@pytest.mark.parametrize("in_place", [False, True])
def test_layout(a, in_place):
    rc.check_layout(a, in_place, also_counts=True)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("model", ["k2p", "tn93"])
def test_chunking(a, monkeypatch, model, in_place):
    rc.check_chunking(a, monkeypatch, model, in_place)


def test_arguments_without_a_device(either):
    rc.check_arguments(either)


def test_struct_matches_header(tmp_path):
    rc.check_struct(tmp_path)


def test_python_without_a_device():
    """window_ranges' values and errors; the wrappers refuse bad keywords before any device use; empty batches."""
    import fastneighbornet_amd as fa
    from fastneighbornet_amd import _capi
    s, e = fa.window_ranges(10, 4, 3)
    assert s.dtype == e.dtype == np.int64 and s.tolist() == [0, 3, 6] and e.tolist() == [4, 7, 10]
    s, e = fa.window_ranges(10, 10)
    assert s.tolist() == [0] and e.tolist() == [10]
    s, e = fa.window_ranges(7, 1)
    assert s.tolist() == list(range(7)) and (e - s == 1).all()
    assert fa.window_ranges(1000000, 1000, 250)[0].shape == (3997,)
    for bad in ((10, 0, 1), (10, 11, 1), (10, 4, 0), (10, -2, 1)):
        with pytest.raises(ValueError):
            fa.window_ranges(*bad)
    seq = fa.encode_alignment(["ACGTN", "ACGTR", "AYGTT"], missing="-")
    starts, ends = np.array([0, 1]), np.array([5, 4])
    for model in ("jc69", "k2p", "f81", "felsenstein84", "tn93"):
        for shape in (0.0, -2.0, float("inf"), float("nan")):
            with pytest.raises(_capi.FnnError) as ei:
                fa.range_distances(seq, starts, ends, model=model, gamma_shape=shape)
            assert ei.value.code == -1 and "shape" in str(ei.value)
    for model in ("p", "logdet"):
        with pytest.raises(_capi.FnnError) as ei:
            fa.range_distances(seq, starts, ends, model=model, gamma_shape=0.5)
        assert ei.value.code == -1 and "gamma" in str(ei.value)
    with pytest.raises(_capi.FnnError) as ei:
        fa.range_distances(seq, starts, ends, model="k2p", on_saturation="cap")
    assert ei.value.code == -1 and "cap" in str(ei.value)
    with pytest.raises(_capi.FnnError) as ei:
        fa.range_distances(seq, [0, 2], [5, 6])
    assert ei.value.code == -1 and "range 1:" in str(ei.value)
    with pytest.raises(_capi.FnnError) as ei:
        fa.pair_counts_ranges(seq, [3, 2], [2, 4])
    assert ei.value.code == -1 and "range 0:" in str(ei.value)
    with pytest.raises(ValueError):
        fa.range_distances(seq, [0, 1], [5])
    with pytest.raises(ValueError):
        fa.range_distances(seq, starts, ends, out="cupy")
    with pytest.raises(ValueError):
        fa.pair_counts_ranges(seq, starts, ends, out="cupy")
    with pytest.raises(KeyError):
        fa.range_networks(seq, starts, ends, model="f84")
    with pytest.raises(ValueError):
        fa.sliding_windows(seq, 6, 1)
    keywords = ("device", "model", "states", "on_saturation", "cap", "gamma_shape")
    for fn in (fa.range_distances, fa.range_networks, fa.sliding_windows):
        p = inspect.signature(fn).parameters
        assert all(k in p for k in keywords) and p["gamma_shape"].default is None and p["model"].default == "p"
        assert [p[k].default for k in keywords] == [inspect.signature(fa.alignment_distances_batch).parameters[k].default for k in keywords]
    assert "out" in inspect.signature(fa.range_distances).parameters and "out" in inspect.signature(fa.pair_counts_ranges).parameters
    assert inspect.signature(fa.range_networks).parameters["weights"].default is True
    D, st = fa.range_distances(seq, [], [], model="tn93", gamma_shape=0.5)
    assert D.shape == (0, 3, 3) and st["n_problems"] == 0 and st["n_site_blocks"] == 0
    F, st = fa.pair_counts_ranges(seq, [], [])
    assert F.shape == (0, 3, 3, 4, 4) and F.dtype == np.int64 and st["n_problems"] == 0


def test_standalone_program_under_asan_ubsan():
    """tests/emu/fnn_dist_ranges_emu_main.cpp with -fsanitize=address,undefined, as a program of its own (no sanitizer runtime is
    loaded into the interpreter): the cases of this suite on heap blocks of exactly the declared sizes, each range entry against
    the counts entry on the 0/1 counts of its ranges."""
    exe = os.path.join(dc.EMU_DIR, "build", "fnn_dist_ranges_emu_main_asan")
    srcs = [os.path.join(dc.EMU_DIR, "fnn_dist_ranges_emu_main.cpp")] + rc.EMU_SRCS
    if dc.newer(exe, srcs):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g", "-O2",
                               "-o", exe, srcs[0], srcs[1]])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for k in ("FNN_BATCH_CHUNK", "FNN_DIST_FORCE_MISSING", "FNN_DIST_FORCE_DIGITS", "FNN_DRAW_ROUTE"):
        env.pop(k, None)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.startswith("ok: ")

"""Gamma-distributed rates for the corrected alignment distances (fnn_dist_model.h) on the CPU: dist_expm1
against its Python restatement and against math.expm1; the cases of tests/dist_gamma_common.py through
tests/emu/fnn_dist_gamma_emu.cpp, which runs the per-lane steps for lane = 0 ... 63 of every wave under the product's host logic,
bitwise against the reference; the argument checks also against the product library (they need no device); and the stand-alone
AddressSanitizer / UBSan program."""
import os
import subprocess

import pytest

import dist_common as dc
import dist_gamma_common as gc

MODELS = gc.MODELS


@pytest.fixture(scope="module")
def a():
    return gc.emu_dist_gamma_api()


@pytest.fixture(scope="module", params=["driver", "product"])
def either(request):
    if request.param == "driver":
        return gc.emu_dist_gamma_api()
    import fastneighbornet_amd as fa
    return fa.api()


def test_expm1_bits_and_error(a):
    """emug_dist_expm1 equals the restatement bit for bit over the threshold neighbourhoods and the random list, in both signs, and
    lies within 2 ulp of math.expm1 (fdlibm's stated < 1 ulp and one for math.expm1 itself); the largest distance seen is the
    figure recorded in DESIGN.md section 19."""
    worst = gc.check_expm1(a)
    print("largest distance from math.expm1:", worst, "ulp")
    assert worst <= gc.EXPM1_BOUND_ULP


def test_reference_of_equal_rates_is_the_existing_one():
    gc.check_reference_of_equal_rates()


def test_thresholds_reach_every_positive_path():
    gc.check_thresholds_reach_every_positive_path()


@pytest.mark.parametrize("name", sorted(gc.EXPM1_THRESHOLDS))
def test_expm1_thresholds_through_jc69_distances(a, name):
    gc.check_threshold(a, name)


@pytest.mark.parametrize("shape", gc.SHAPES)
@pytest.mark.parametrize("missing", [False, True])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("k", range(len(gc.GRID_SHAPES)), ids=gc.GRID_NAMES)
def test_every_model_with_gamma(a, k, model, missing, shape):
    gc.check_grid(a, k, model, missing, shape)


@pytest.mark.parametrize("missing", [False, True])
@pytest.mark.parametrize("cmax,passes", gc.DIGIT_CASES)
@pytest.mark.parametrize("model", MODELS)
def test_digit_planes(a, model, cmax, passes, missing):
    gc.check_digits(a, model, cmax, passes, missing)


@pytest.mark.parametrize("model", MODELS)
def test_overflow_is_saturation(a, model):
    gc.check_overflow(a, model)


@pytest.mark.parametrize("in_place", [False, True])
def test_equal_rates_through_the_struct(a, in_place):
    gc.check_equal_rates_through_the_struct(a, in_place)


@pytest.mark.parametrize("model", MODELS)
def test_both_draw_routes_agree_with_the_counts_entry(a, monkeypatch, model):
    gc.check_bootstrap_entry(a, monkeypatch, model)


def test_arguments_without_a_device(either):
    gc.check_arguments(either)


def test_struct_matches_header(tmp_path):
    gc.check_struct(tmp_path)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("model", ["k2p", "tn93"])
def test_chunking(a, monkeypatch, model, in_place):
    gc.check_chunking(a, monkeypatch, model, in_place)


def test_python_keywords_without_a_device():
    """The four wrappers take gamma_shape; a wrong one is refused before any device use, with the field named."""
    import numpy as np
    import fastneighbornet_amd as fa
    from fastneighbornet_amd import _capi
    seq = fa.encode_alignment(["ACGTN", "ACGTR", "AYGTT"], missing="-")
    counts = np.ones((2, 5), dtype=np.uint16)
    for model in MODELS:
        for shape in (0.0, -2.0, float("inf"), float("nan")):
            with pytest.raises(_capi.FnnError) as ei:
                fa.alignment_distances_batch(seq, counts, model=model, gamma_shape=shape)
            assert ei.value.code == -1 and "shape" in str(ei.value)
            with pytest.raises(_capi.FnnError) as ei:
                fa.bootstrap_distances(seq, 2, 7, lead=1, model=model, gamma_shape=shape)
            assert ei.value.code == -1 and "shape" in str(ei.value)
    for model in ("p", "logdet"):
        with pytest.raises(_capi.FnnError) as ei:
            fa.alignment_distances_batch(seq, counts, model=model, gamma_shape=0.5)
        assert ei.value.code == -1 and "gamma" in str(ei.value)
        with pytest.raises(_capi.FnnError) as ei:
            fa.bootstrap_distances(seq, 2, 7, model=model, gamma_shape=0.5)
        assert ei.value.code == -1 and "gamma" in str(ei.value)
    import inspect
    for fn in (fa.alignment_distances_batch, fa.bootstrap_distances, fa.bootstrap, fa.bootstrap_support):
        assert inspect.signature(fn).parameters["gamma_shape"].default is None
    D, st = fa.alignment_distances_batch(seq, counts[:0], model="tn93", gamma_shape=0.5)
    assert D.shape == (0, 3, 3) and st["n_problems"] == 0


def test_standalone_program_under_asan_ubsan():
    """tests/emu/fnn_dist_gamma_emu_main.cpp with -fsanitize=address,undefined, as a program of its own (no sanitizer runtime is
    loaded into the interpreter): the five models at several shapes under both policies, both draw routes among the calls, on
    buffers of exactly the declared sizes."""
    exe = os.path.join(dc.EMU_DIR, "build", "fnn_dist_gamma_emu_main_asan")
    srcs = [os.path.join(dc.EMU_DIR, "fnn_dist_gamma_emu_main.cpp")] + gc.EMU_SRCS
    if dc.newer(exe, srcs):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g", "-O1",
                               "-o", exe, srcs[0], srcs[1]])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for k in ("FNN_BATCH_CHUNK", "FNN_DIST_FORCE_MISSING", "FNN_DIST_FORCE_DIGITS", "FNN_DRAW_ROUTE"):
        env.pop(k, None)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.startswith("ok: ")

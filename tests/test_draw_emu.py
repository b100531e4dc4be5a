"""Bootstrap replicates drawn on the device (fnn_draw.h) on the CPU: the cases of tests/draw_common.py
through tests/emu/fnn_draw_emu.cpp, which runs k_draw's per-lane steps for tid = 0 ... 255 of every row and the distance kernels'
for every lane under the product's host logic, bitwise against the reference; the argument checks also against the product
library (they need no device); and the stand-alone AddressSanitizer / UBSan program."""
import os
import subprocess

import pytest

import dist_common as dc
import draw_common as wc


@pytest.fixture(scope="module")
def a():
    return wc.emu_draw_api()


@pytest.fixture(scope="module", params=["driver", "product"])
def either(request):
    if request.param == "driver":
        return wc.emu_draw_api()
    import fastneighbornet_amd as fa
    return fa.api()


@pytest.mark.parametrize("L,batch,seed,lead,digits", wc.PLANE_CASES)
def test_drawn_planes(a, L, batch, seed, lead, digits):
    wc.check_planes(a, L, batch, seed, lead, digits)


def test_drawn_planes_of_a_later_chunk(a):
    wc.check_planes(a, 65, 3, 7, 1, 2, first=3)
    wc.check_planes(a, 130, 64, wc.M64, 0, 1, first=64)


def test_single_counts_through_matrices(a):
    wc.check_single_counts(a)


def test_shapes_hold_every_value():
    assert {s[0] for s in wc.SHAPES} == {1, 2, 5, 17, 33}
    assert {s[1] for s in wc.SHAPES} == {1, 15, 16, 17, 63, 64, 65, 130, 200}
    assert {s[2] for s in wc.SHAPES} == {1, 15, 16, 17, 63, 64, 65, 70}
    assert {s[3] for s in wc.SHAPES} == {0, 7, 2 ** 64 - 1}


@pytest.mark.parametrize("missing", [False, True])
@pytest.mark.parametrize("model", wc.MODELS)
@pytest.mark.parametrize("k", range(len(wc.SHAPES)), ids=wc.SHAPE_IDS)
def test_shapes(a, k, model, missing):
    wc.check_shape(a, k, model, missing)


def test_k2p_with_three_forced_planes(a, monkeypatch):
    wc.check_k2p_three_planes(a, monkeypatch)


@pytest.mark.parametrize("model", wc.MODELS)
def test_lead(a, model):
    wc.check_lead(a, model)


@pytest.mark.parametrize("model", wc.MODELS)
def test_forced_digits(a, monkeypatch, model):
    wc.check_forced_digits(a, monkeypatch, model)


@pytest.mark.parametrize("in_place", [False, True])
def test_layout(a, in_place):
    wc.check_layout(a, in_place)


@pytest.mark.parametrize("in_place", [False, True])
def test_chunking(a, monkeypatch, in_place):
    wc.check_chunking(a, monkeypatch, in_place)


@pytest.mark.parametrize("above", [False, True], ids=["at-the-limit", "above"])
def test_site_limit(a, monkeypatch, above):
    wc.check_limit(a, monkeypatch, above)


def test_forced_device_route_above_the_limit_without_a_device(either, monkeypatch):
    wc.check_forced_device_above_the_limit(either, monkeypatch)


@pytest.mark.parametrize("model", wc.MODELS)
def test_forced_host_route(a, monkeypatch, model):
    wc.check_forced_host(a, monkeypatch, model)


def test_empty_pair_in_a_drawn_replicate(a):
    wc.check_empty_pair(a)


def test_saturated_pair_in_a_drawn_replicate(a):
    wc.check_saturated_pair(a)


def test_arguments_without_a_device(either, monkeypatch):
    wc.check_arguments(either, monkeypatch)


def test_struct_matches_header(tmp_path):
    wc.check_struct_sizes(tmp_path)


def test_python_keywords_without_a_device():
    """The wrappers refuse a wrong keyword before any device use."""
    import numpy as np
    import fastneighbornet_amd as fa
    from fastneighbornet_amd import _capi
    seq = fa.encode_alignment(["ACGTN", "ACGTR", "AYGTT"], missing="-")
    with pytest.raises(_capi.FnnError) as ei:
        fa.bootstrap_distances(seq, 3, 7, model="jc69", states=4)
    assert ei.value.code == -1 and "distinct" in str(ei.value)
    with pytest.raises(ValueError):
        fa.bootstrap_distances(seq, 3, 7, lead=2)
    with pytest.raises(ValueError):
        fa.bootstrap(seq, 3, 7, draw="elsewhere")
    with pytest.raises(ValueError):
        fa.bootstrap_support(seq, 3, 7, draw="elsewhere")
    D, st = fa.bootstrap_distances(seq, 0, 7)
    assert D.shape == (0, 3, 3) and st["n_problems"] == 0
    assert fa.api().bootstrap_draw_max_sites() == wc.emu_draw_api().bootstrap_draw_max_sites() >= 30000
    assert isinstance(np.asarray(D), np.ndarray)


def test_standalone_program_under_asan_ubsan():
    """tests/emu/fnn_draw_emu_main.cpp with -fsanitize=address,undefined, as a program of its own (no sanitizer runtime is
    loaded into the interpreter): the histogram in a block of exactly the launch's LDS bytes, the planes in blocks of exactly the
    sizes the host logic asks for."""
    exe = os.path.join(dc.EMU_DIR, "build", "fnn_draw_emu_main_asan")
    srcs = [os.path.join(dc.EMU_DIR, "fnn_draw_emu_main.cpp")] + wc.EMU_SRCS
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

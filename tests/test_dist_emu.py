"""The alignment-distance path (fnn_dist.h) on the CPU: the per-lane steps run for lane = 0 ... 63 of
every wave, with the tile product as loops written from the stated lane maps, by tests/emu/fnn_dist_emu.cpp under the product's
own host logic, bitwise against the numpy reference of tests/dist_common.py; the argument checks and the count generator
also against the product library (they need no device); and the stand-alone AddressSanitizer / UBSan program."""
import ctypes as C
import os
import subprocess

import pytest

import dist_common as dc
from fastneighbornet_amd import _capi


@pytest.fixture(scope="module")
def a():
    return dc.emu_dist_api()


@pytest.fixture(scope="module", params=["driver", "product"])
def either(request):
    if request.param == "driver":
        return dc.emu_dist_api()
    import fastneighbornet_amd as fa
    return fa.api()


@pytest.mark.parametrize("where", sorted(dc.LANE_MAP_SITES))
def test_lane_and_tile_maps(a, where):
    dc.check_lane_maps(a, where)


@pytest.mark.parametrize("k", range(len(dc.SHAPES)), ids=[f"n{n}-L{L}-B{B}" for n, L, B in dc.SHAPES])
def test_shape_edges(a, k):
    dc.check_shape(a, k)


def test_shape_list_holds_every_value():
    assert {s[0] for s in dc.SHAPES} == {1, 2, 3, 5, 6, 7, 17, 33, 65}
    assert {s[1] for s in dc.SHAPES} == {1, 15, 16, 17, 63, 64, 65, 130}
    assert {s[2] for s in dc.SHAPES} == {1, 15, 16, 17, 33}


@pytest.mark.parametrize("missing", [False, True])
@pytest.mark.parametrize("cmax,passes", dc.DIGIT_CASES)
def test_digit_planes(a, cmax, passes, missing):
    dc.check_digits(a, cmax, passes, missing)


def test_missing_data(a, monkeypatch):
    dc.check_missing(a, monkeypatch)


@pytest.mark.parametrize("also_an_empty_replicate", [False, True])
def test_pair_without_a_common_site(a, also_an_empty_replicate):
    dc.check_empty_pair(a, also_an_empty_replicate)


@pytest.mark.parametrize("in_place", [False, True])
def test_layout(a, in_place):
    dc.check_layout(a, in_place)


@pytest.mark.parametrize("in_place", [False, True])
def test_chunking(a, monkeypatch, in_place):
    dc.check_chunking(a, monkeypatch, in_place)


def test_arguments_without_a_device(either):
    dc.check_arguments(either)


@pytest.mark.parametrize("L,B,seed", dc.BOOTSTRAP_CASES)
def test_bootstrap_counts(either, L, B, seed):
    dc.check_bootstrap_counts(either, L, B, seed)


def test_bootstrap_counts_arguments(either):
    assert either.bootstrap_counts(0, 1, 0, None) == -1
    assert either.bootstrap_counts(5, -1, 0, None) == -1
    assert either.bootstrap_counts(5, 2, 0, None) == -1
    assert either.bootstrap_counts(5, 0, 0, None) == 0
    import numpy as np
    buf = np.zeros(1, dtype=np.uint16)
    assert either.bootstrap_counts(1, 1, 0, buf.ctypes.data) == 0 and buf[0] == 1


def test_python_wrappers_without_a_device():
    import numpy as np
    import fastneighbornet_amd as fa
    enc = fa.encode_alignment(["acg-T", "ACNXt", "A?GTT"])
    assert enc.dtype == np.uint8 and enc.shape == (3, 5)
    assert enc.tolist() == [[65, 67, 71, 255, 84], [65, 67, 255, 255, 84], [65, 255, 71, 84, 84]]
    assert fa.encode_alignment(["ab-"], missing="b").tolist() == [[65, 255, 45]]
    with pytest.raises(ValueError):
        fa.encode_alignment(["AC", "A"])
    c = fa.bootstrap_counts(7, 5, 1)
    assert (c.astype(np.int64) == dc.ref_bootstrap_counts(7, 5, 1)).all()
    if fa.api().device_count() < 1:   # no CPU fallback
        with pytest.raises(_capi.FnnError) as ei:
            fa.alignment_distances_batch(enc, np.ones((2, 5), dtype=np.uint16))
        assert ei.value.code == -3


def test_stats_struct_matches_header(tmp_path):
    """sizeof(fnn_dist_stats) as the C compiler sees it against the ctypes mirror (tests/test_abi.py checks the symbols)."""
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "fastnn.h"\nint main(void) { printf("%zu %d %d\\n", sizeof(fnn_dist_stats), '
                   'FNN_SITE_MISSING, (int)FNN_DIST_P); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(dc.ROOT, "include"), "-o", str(exe), str(src)])
    size, missing, model = (int(x) for x in subprocess.check_output([str(exe)], text=True).split())
    assert size == C.sizeof(_capi.FnnDistStats) == 3 * 8 + 4 * 4 + 3 * 8 + 4 * 8
    assert (missing, model) == (_capi.SITE_MISSING, _capi.DIST_P) == (255, 0)


def test_standalone_program_under_asan_ubsan():
    """tests/emu/fnn_dist_emu_main.cpp with -fsanitize=address,undefined, as a program of its own (no sanitizer runtime is
    loaded into the interpreter): the shape, digit, missing-data and layout cases on buffers of exactly the declared sizes."""
    exe = os.path.join(dc.EMU_DIR, "build", "fnn_dist_emu_main_asan")
    srcs = [os.path.join(dc.EMU_DIR, "fnn_dist_emu_main.cpp")] + dc.EMU_SRCS
    if dc.newer(exe, srcs):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g", "-O1",
                               "-o", exe, srcs[0], srcs[1]])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("FNN_BATCH_CHUNK", None)
    env.pop("FNN_DIST_FORCE_MISSING", None)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.startswith("ok: ")

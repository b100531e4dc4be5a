"""Bootscan - bootstrap replicates inside every site range (fnn_scan.h) - on the CPU: the cases of
tests/bootscan_common.py through tests/emu/fnn_bootscan_emu.cpp, which runs the per-lane steps of k_draw_ranges, k_dist_scan and
k_dist_scan_pairs for every thread of every workgroup under the product's host logic, bitwise against the driver's own counts and
bootstrap entries on the counts of the definition; the definition and the argument checks also against the product library (they
need no device); the Python wrappers' checks; and the stand-alone AddressSanitizer / UBSan program."""
import inspect
import os
import subprocess

import numpy as np
import pytest

import bootscan_common as bc
import dist_common as dc

GRID = [pytest.param(m, s, id=name) for (m, s), name in zip(bc.GRID_MODELS, bc.GRID_MODEL_NAMES)]


@pytest.fixture(scope="module")
def a():
    return bc.emu_bootscan_api()


@pytest.fixture(scope="module", params=["driver", "product"])
def either(request):
    if request.param == "driver":
        return bc.emu_bootscan_api()
    import fastneighbornet_amd as fa
    return fa.api()


@pytest.mark.parametrize("case", range(len(bc.DEFINITION_CASES)))
def test_definition_without_a_device(either, case):
    bc.check_definition(either, *bc.DEFINITION_CASES[case])


def test_compact_planes_and_row_words(a):
    bc.check_planes(a)
    bc.check_planes(a, R=2, lead=0, seed=bc.M64)


def test_every_boundary_through_the_entries(a):
    bc.check_plane_windows(a)


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("P", bc.GROUP_P)
def test_column_groups(a, P, lead):
    bc.check_groups(a, P, lead)


@pytest.mark.parametrize("model,shape", GRID)
@pytest.mark.parametrize("missing", [False, True])
@pytest.mark.parametrize("k", range(len(bc.WINDOW_SETS)))
def test_grid(a, k, missing, model, shape):
    bc.check_grid(a, k, missing, model, shape)


def test_one_window_is_the_bootstrap_entry(a):
    bc.check_whole_alignment(a)


@pytest.mark.parametrize("model", ["k2p", "tn93", "tables"])
def test_routes(a, monkeypatch, model):
    bc.check_routes(a, monkeypatch, model)


@pytest.mark.parametrize("above", [False, True])
def test_limit(a, monkeypatch, above):
    bc.check_limit(a, monkeypatch, above)


def test_forced_device_above_the_limit(either, monkeypatch):
    bc.check_forced_device_above_the_limit(either, monkeypatch)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("model", ["k2p", "tn93", "tables"])
def test_chunking(a, monkeypatch, model, in_place):
    bc.check_chunking(a, monkeypatch, model, in_place)


def test_empty_window(either):
    bc.check_empty_window(either, device=either.prefix != "fnn_")


def test_empty_pair_inside_one_replicate(a):
    bc.check_empty_pair(a)


def test_saturated_replicate(a):
    bc.check_saturated(a)


def test_arguments_without_a_device(either, monkeypatch):
    bc.check_arguments(either, monkeypatch)


def test_struct_matches_header(tmp_path):
    bc.check_struct(tmp_path)


def test_python_without_a_device():
    """The wrappers' values and errors before any device use; empty calls."""
    import fastneighbornet_amd as fa
    from fastneighbornet_amd import _capi
    c = fa.bootscan_counts(10, [0, 2], [10, 6], 3, 7, lead=1)
    assert c.shape == (8, 10) and c.dtype == np.uint16 and (c == bc.ref_counts(10, [0, 2], [10, 6], 3, 7, 1)).all()
    assert (fa.bootscan_counts(10, [0, 2], [10, 6], 3, 7, lead=1, first=3, count=2) == c[3:5]).all()
    assert (fa.bootscan_counts(10, [0, 2], [10, 6], 3, 7)[:3] == c[1:4]).all()   # (lead = 0: the same replicates)
    seq = fa.encode_alignment(["ACGTN", "ACGTR", "AYGTT"], missing="-")
    with pytest.raises(_capi.FnnError) as ei:
        fa.bootscan_distances(seq, [0, 2], [5, 6], 2, 1)
    assert ei.value.code == -1 and "window 1:" in str(ei.value)
    with pytest.raises(_capi.FnnError) as ei:
        fa.bootscan_counts(5, [3], [2], 2, 1)
    assert ei.value.code == -1 and "window 0:" in str(ei.value)
    with pytest.raises(_capi.FnnError) as ei:
        fa.bootscan_distances(seq, [0, 1], [5, 4], 2, 1, model="tn93", gamma_shape=-1.0)
    assert ei.value.code == -1 and "shape" in str(ei.value)
    for bad in (dict(lead=2), dict(out="cupy")):
        with pytest.raises(ValueError):
            fa.bootscan_distances(seq, [0, 1], [5, 4], 2, 1, **bad)
    with pytest.raises(ValueError):
        fa.bootscan_distances(seq, [0, 1], [5], 2, 1)
    with pytest.raises(ValueError):
        fa.bootscan_pair_counts(seq, [0, 1], [5, 4], -1, 1)
    with pytest.raises(ValueError):
        fa.bootscan(seq, 6, 1, 2, 1)
    with pytest.raises(KeyError):
        fa.bootscan_networks(seq, [0], [5], 2, 1, model="f84")
    keywords = ("device", "model", "states", "on_saturation", "cap", "gamma_shape")
    for fn in (fa.bootscan_distances, fa.bootscan_networks, fa.bootscan):
        p = inspect.signature(fn).parameters
        assert [p[k].default for k in keywords] == [inspect.signature(fa.alignment_distances_batch).parameters[k].default for k in keywords]
    assert inspect.signature(fa.bootscan_distances).parameters["lead"].default == 1
    D, st = fa.bootscan_distances(seq, [], [], 4, 1, model="tn93", gamma_shape=0.5)
    assert D.shape == (0, 5, 3, 3) and st["n_problems"] == 0 and st["n_windows"] == 0 and st["n_host_chunks"] == 0
    D, st = fa.bootscan_distances(seq, [0, 1], [5, 4], 0, 1, lead=0)
    assert D.shape == (2, 0, 3, 3) and st["n_problems"] == 0 and st["n_windows"] == 2
    F, st = fa.bootscan_pair_counts(seq, [], [], 2, 1)
    assert F.shape == (0, 3, 3, 3, 4, 4) and F.dtype == np.int64


def test_standalone_program_under_asan_ubsan():
    """tests/emu/fnn_bootscan_emu_main.cpp with -fsanitize=address,undefined, as a program of its own (no sanitizer runtime is loaded
    into the interpreter): cases of this suite on heap blocks of exactly the declared sizes, each bootscan entry against the counts
    entry on the rows of fnn_bootscan_counts."""
    exe = os.path.join(dc.EMU_DIR, "build", "fnn_bootscan_emu_main_asan")
    srcs = [os.path.join(dc.EMU_DIR, "fnn_bootscan_emu_main.cpp")] + bc.EMU_SRCS
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

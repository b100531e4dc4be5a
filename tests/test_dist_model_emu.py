"""The corrected alignment distances (fnn_dist_model.h) on the CPU: dist_log1p against its Python
restatement and against math.log1p; the cases of tests/dist_model_common.py through tests/emu/fnn_dist_model_emu.cpp, which runs
the per-lane steps for lane = 0 ... 63 of every wave under the product's host logic, bitwise against the reference; the
argument checks also against the product library (they need no device); and the stand-alone AddressSanitizer / UBSan
program."""
import math
import os
import subprocess

import pytest

import dist_common as dc
import dist_model_common as mc

MODELS = ["jc69", "k2p"]


@pytest.fixture(scope="module")
def a():
    return mc.emu_dist_model_api()


@pytest.fixture(scope="module", params=["driver", "product"])
def either(request):
    if request.param == "driver":
        return mc.emu_dist_model_api()
    import fastneighbornet_amd as fa
    return fa.api()


def test_log1p_bits_and_error(a):
    """emu_dist_log1p equals the restatement bit for bit; both are at most 2 ulp from math.log1p (each is below 1 ulp from
    the true value; 1 is the largest seen)."""
    xs = mc.log1p_arguments()
    assert len(xs) > 8000 and -0.0 in xs
    worst = 0
    for x in xs:
        got, want = a.dist_log1p(x), mc.ref_log1p(x)
        assert mc.bits(got) == mc.bits(want), (x, got, want)
        worst = max(worst, mc.ulps_apart(got, math.log1p(x)))
    print("largest distance from math.log1p:", worst, "ulp")
    assert worst <= 2
    assert mc.bits(a.dist_log1p(-0.0)) == mc.bits(-0.0) and mc.bits(a.dist_log1p(0.0)) == 0
    assert a.dist_log1p(-0.5) == -0.6931471805599453
    for x in (-1.0, -1.5, float("nan"), float("inf")):
        assert math.isnan(a.dist_log1p(x)) and math.isnan(mc.ref_log1p(x))


@pytest.mark.parametrize("x", [1e-300, 2.0 ** -40, 1e-3, 0.4, 0.5, 1.0, 3.0, 1e10, 2.0 ** 60])
def test_log1p_positive_arguments(a, x):
    """(no distance needs them: the paths of the algorithm that negative arguments do not reach)"""
    got = a.dist_log1p(x)
    assert mc.bits(got) == mc.bits(mc.ref_log1p(x)) and mc.ulps_apart(got, math.log1p(x)) <= 2


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("where", sorted(dc.LANE_MAP_SITES))
def test_transition_byte_and_lane_maps(a, where, model):
    mc.check_lane_maps(a, where, model)


@pytest.mark.parametrize("n", [2, 5])
@pytest.mark.parametrize("model", MODELS)
def test_prescribed_ratios(a, model, n):
    mc.check_ratios(a, model, n)


def test_shape_subset_holds_every_value():
    shapes = [dc.SHAPES[k] for k in mc.SHAPE_IDS]
    assert {s[0] for s in shapes} >= {1, 2, 3, 17, 33, 65}
    assert {s[1] for s in shapes} == {1, 15, 16, 17, 63, 64, 65, 130}
    assert {s[2] for s in shapes} == {1, 15, 16, 17, 33}


@pytest.mark.parametrize("missing", [False, True])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("k", mc.SHAPE_IDS, ids=["n%d-L%d-B%d" % dc.SHAPES[k] for k in mc.SHAPE_IDS])
def test_shape_edges(a, k, model, missing):
    mc.check_shape(a, k, model, missing)


@pytest.mark.parametrize("missing", [False, True])
@pytest.mark.parametrize("cmax,passes", mc.DIGIT_CASES)
def test_digit_planes_with_three_accumulator_sets(a, cmax, passes, missing):
    mc.check_digits(a, cmax, passes, missing)


def test_recoding(a):
    mc.check_recoding(a)


def test_too_many_states_without_a_device(either):
    mc.check_too_many_states(either)


@pytest.mark.parametrize("kind", sorted(mc.SATURATION_KINDS))
def test_saturation(a, kind):
    mc.check_saturation(a, kind)


@pytest.mark.parametrize("kind", sorted(mc.SATURATION_KINDS))
def test_lowest_empty_or_saturated_pair_is_named(a, kind):
    mc.check_saturation_order(a, kind)


@pytest.mark.parametrize("in_place", [False, True])
def test_p_distance_through_the_model_entries(a, in_place):
    mc.check_p_equals_old_entry(a, dc.emu_dist_api(), in_place)


def test_arguments_without_a_device(either):
    mc.check_arguments(either)


def test_structs_match_header(tmp_path):
    mc.check_struct_sizes(tmp_path)


@pytest.mark.parametrize("in_place", [False, True])
def test_layout(a, in_place):
    mc.check_layout(a, in_place)


@pytest.mark.parametrize("in_place", [False, True])
def test_chunking(a, monkeypatch, in_place):
    mc.check_chunking(a, monkeypatch, in_place)


def test_python_keywords_without_a_device():
    """The wrappers take the model keywords and hand them to the model entries: a wrong one is refused before any device use."""
    import numpy as np
    import fastneighbornet_amd as fa
    from fastneighbornet_amd import _capi
    seq = fa.encode_alignment(["ACGTN", "ACGTR", "AYGTT"], missing="-")
    counts = np.ones((2, 5), dtype=np.uint16)
    with pytest.raises(_capi.FnnError) as ei:
        fa.alignment_distances_batch(seq, counts, model="jc69", states=4)
    assert ei.value.code == -1 and "distinct" in str(ei.value)
    with pytest.raises(_capi.FnnError) as ei:
        fa.alignment_distances_batch(seq, counts, model="k2p", on_saturation="cap")
    assert ei.value.code == -1 and "cap" in str(ei.value)
    with pytest.raises(KeyError):
        fa.alignment_distances_batch(seq, counts, model="f84")


def test_standalone_program_under_asan_ubsan():
    """tests/emu/fnn_dist_model_emu_main.cpp with -fsanitize=address,undefined, as a program of its own (no sanitizer runtime is
    loaded into the interpreter): shapes, digit planes, recoding and saturation on buffers of exactly the declared sizes."""
    exe = os.path.join(dc.EMU_DIR, "build", "fnn_dist_model_emu_main_asan")
    srcs = [os.path.join(dc.EMU_DIR, "fnn_dist_model_emu_main.cpp")] + mc.EMU_SRCS
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

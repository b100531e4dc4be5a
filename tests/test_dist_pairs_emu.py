"""The 4 x 4 tables of state pairs and F81, F84, TN93 and LogDet on them (fnn_dist_pairs.h, fnn_dist_model.h, DESIGN.md section
18) on the CPU: dist_log against its Python restatement and against math.log; the cases of tests/dist_pairs_common.py through
tests/emu/fnn_dist_pairs_emu.cpp, which runs the per-lane steps for lane = 0 ... 63 of every wave under the product's host
logic, bitwise against the reference; the argument checks also against the product library (they need no device); and the
stand-alone AddressSanitizer / UBSan program."""
import math
import os
import subprocess

import pytest

import dist_common as dc
import dist_model_common as mc
import dist_pairs_common as pc

MODELS = pc.MODELS
SHAPE_NAMES = ["n%d-L%d-B%d" % dc.SHAPES[k] for k in mc.SHAPE_IDS]


@pytest.fixture(scope="module")
def a():
    return pc.emu_dist_pairs_api()


@pytest.fixture(scope="module", params=["driver", "product"])
def either(request):
    if request.param == "driver":
        return pc.emu_dist_pairs_api()
    import fastneighbornet_amd as fa
    return fa.api()


def test_log_bits_and_error(a):
    """emup_dist_log equals the restatement bit for bit; the largest distance from math.log over the fixed list is the figure
    recorded in DESIGN.md section 18, and the bound is that figure plus one ulp for math.log's own error."""
    xs = pc.log_arguments()
    assert len(xs) > 16000
    worst = 0
    for x in xs:
        got, want = a.dist_log(x), pc.ref_log(x)
        assert mc.bits(got) == mc.bits(want), (x, got, want)
        worst = max(worst, mc.ulps_apart(got, math.log(x)))
    print("largest distance from math.log:", worst, "ulp")
    assert worst <= pc.LOG_WORST_ULP_RECORDED + 1
    assert mc.bits(a.dist_log(1.0)) == 0 and a.dist_log(0.5) == -0.6931471805599453 and a.dist_log(2.0) == 0.6931471805599453
    for x in (0.0, -0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert math.isnan(a.dist_log(x)) and math.isnan(pc.ref_log(x))


def test_counts_and_lane_maps(a):
    pc.check_counts_lane_maps(a)


def test_shape_subset_holds_every_value():
    shapes = [dc.SHAPES[k] for k in mc.SHAPE_IDS]
    assert {s[0] for s in shapes} >= {2, 5, 17, 33}
    assert {s[1] for s in shapes} >= {1, 63, 64, 65, 130}
    assert {s[2] for s in shapes} == {1, 15, 16, 17, 33}
    # B = 16 RT + 1 for the replicate tiles per wave in use: 2 with one digit plane, 1 with more
    assert 16 * 2 + 1 in {s[2] for s in shapes} and pc.digit_case(128, 2, False)[1].shape[0] == 16 * 1 + 1


@pytest.mark.parametrize("missing", [False, True])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("k", mc.SHAPE_IDS, ids=SHAPE_NAMES)
def test_shape_edges(a, k, model, missing):
    pc.check_shape(a, k, model, missing)


@pytest.mark.parametrize("missing", [False, True])
@pytest.mark.parametrize("k", mc.SHAPE_IDS, ids=SHAPE_NAMES)
def test_shape_edges_of_the_tables(a, k, missing):
    pc.check_shape_counts(a, k, missing)


@pytest.mark.parametrize("missing", [False, True])
@pytest.mark.parametrize("cmax,passes", pc.DIGIT_CASES)
def test_digit_planes(a, cmax, passes, missing):
    pc.check_digits(a, cmax, passes, missing)


@pytest.mark.parametrize("n", [2, 5])
def test_unequal_frequencies(a, n):
    pc.check_skewed(a, n)


@pytest.mark.parametrize("n", [2, 5])
def test_log_through_logdet_distances(a, n):
    pc.check_logdet_ratios(a, n)


def test_f81_saturates_like_jc69_on_equal_marginals(a):
    pc.check_f81_saturates_like_jc69(a)


@pytest.mark.parametrize("model", MODELS)
def test_bootstrap_entry_takes_the_models(a, monkeypatch, model):
    pc.check_bootstrap_entry(a, monkeypatch, model)


@pytest.mark.parametrize("kind", sorted(pc.SATURATED_KINDS))
def test_saturation_through_each_logarithm(a, kind):
    pc.check_saturated_kind(a, kind)


@pytest.mark.parametrize("model", MODELS)
def test_degenerate_pair(a, model):
    pc.check_degenerate(a, model)


@pytest.mark.parametrize("model", MODELS)
def test_lowest_pair_is_named_with_its_kind(a, model):
    pc.check_kind_order(a, model)


def test_recoding(a):
    pc.check_recoding(a)


def test_arguments_without_a_device(either):
    pc.check_arguments(either)


@pytest.mark.parametrize("which", ["driver", "product"])
def test_p_entries_refuse_the_models_without_a_device(which):
    if which == "driver":
        pc.check_p_entries_refuse_the_models(dc.emu_dist_api())
    else:
        import fastneighbornet_amd as fa
        pc.check_p_entries_refuse_the_models(fa.api())


def test_enums_match_header(tmp_path):
    pc.check_enums(tmp_path)


@pytest.mark.parametrize("in_place", [False, True])
def test_layout(a, in_place):
    pc.check_layout(a, in_place)


@pytest.mark.parametrize("in_place", [False, True])
def test_chunking(a, monkeypatch, in_place):
    pc.check_chunking(a, monkeypatch, in_place)


def test_python_keywords_without_a_device():
    """The wrappers know the four names and `pair_counts_batch` exists; a wrong argument is refused before any device use."""
    import numpy as np
    import fastneighbornet_amd as fa
    from fastneighbornet_amd import _capi
    seq = fa.encode_alignment(["ACGTN", "ACGTR", "AYGTT"], missing="-")
    counts = np.ones((2, 5), dtype=np.uint16)
    for model in MODELS:
        with pytest.raises(_capi.FnnError) as ei:
            fa.alignment_distances_batch(seq, counts, model=model, on_saturation="cap")
        assert ei.value.code == -1 and "cap" in str(ei.value)
        with pytest.raises(_capi.FnnError) as ei:
            fa.bootstrap_distances(seq, 2, 7, lead=1, model=model, on_saturation="cap", cap=-1.0)
        assert ei.value.code == -1 and "cap" in str(ei.value)
    with pytest.raises(ValueError):
        fa.pair_counts_batch(seq, counts, out="cupy")
    with pytest.raises(ValueError):
        fa.pair_counts_batch(seq, counts[:, :4])
    F, st = fa.pair_counts_batch(seq, counts[:0])
    assert F.shape == (0, 3, 3, 4, 4) and F.dtype == np.int64 and st["n_problems"] == 0


def test_standalone_program_under_asan_ubsan():
    """tests/emu/fnn_dist_pairs_emu_main.cpp with -fsanitize=address,undefined, as a program of its own (no sanitizer runtime is
    loaded into the interpreter): shape, digit-plane and kind cases on buffers of exactly the declared sizes."""
    exe = os.path.join(dc.EMU_DIR, "build", "fnn_dist_pairs_emu_main_asan")
    srcs = [os.path.join(dc.EMU_DIR, "fnn_dist_pairs_emu_main.cpp")] + pc.EMU_SRCS
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

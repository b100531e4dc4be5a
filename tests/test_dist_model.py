"""The corrected alignment distances (k_dist_model of fnn_dist.hip) on the GPU: the cases of
tests/dist_model_common.py through the product, bitwise against its reference of exact integers and Python floats; the device
entry and the bootstrap pipeline with a model in a process of its own (torch has to be imported before the product's library
is loaded for the two to share one HIP runtime)."""
import os
import subprocess
import sys

import pytest

import dist_common as dc
import dist_model_common as mc

pytestmark = pytest.mark.gpu

MODELS = ["jc69", "k2p"]


@pytest.fixture(scope="module")
def a(hip_api):
    assert hip_api.device_count() >= 1
    return hip_api


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("where", sorted(dc.LANE_MAP_SITES))
def test_transition_byte_and_lane_maps(a, where, model):
    mc.check_lane_maps(a, where, model)


@pytest.mark.parametrize("n", [2, 5])
@pytest.mark.parametrize("model", MODELS)
def test_prescribed_ratios(a, model, n):
    """The device's dist_log1p through the stored distances: 1 / v, (v - 1) / v and both sides of every branch threshold."""
    mc.check_ratios(a, model, n)


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


def test_too_many_states(a):
    mc.check_too_many_states(a)


@pytest.mark.parametrize("kind", sorted(mc.SATURATION_KINDS))
def test_saturation(a, kind):
    mc.check_saturation(a, kind)


@pytest.mark.parametrize("kind", sorted(mc.SATURATION_KINDS))
def test_lowest_empty_or_saturated_pair_is_named(a, kind):
    mc.check_saturation_order(a, kind)


def test_p_distance_through_the_model_entries(a):
    mc.check_p_equals_old_entry(a, a)


def test_arguments(a):
    mc.check_arguments(a)


def test_layout(a):
    mc.check_layout(a)


def test_chunking(a, monkeypatch):
    mc.check_chunking(a, monkeypatch)


DEVICE_CHILD = r'''
import os, sys
sys.path.insert(0, os.environ["FNN_ROOT"]); sys.path.insert(0, os.path.join(os.environ["FNN_ROOT"], "tests"))
import numpy as np
import torch                       # first: torch's HIP runtime then serves the product's library too (as in bench.py)
import fastneighbornet_amd as fa
import dist_common as dc
import dist_model_common as mc

class Env:                          # (monkeypatch's two calls)
    def setenv(self, k, v): os.environ[k] = v
    def delenv(self, k): del os.environ[k]

a = fa.api()
# the device entry: layout with sentinels in every padding, chunking, the p-distance through it, and the wrapper's tensor
mc.check_layout(a, in_place="torch")
mc.check_chunking(a, Env(), in_place="torch")
mc.check_p_equals_old_entry(a, a, in_place="torch")
seq, counts, D_k2p = mc.pipeline_case("k2p")
T, st = fa.alignment_distances_batch(seq, counts, out="torch", model="k2p")
assert T.is_cuda and T.dtype == torch.float64 and dc.same_bits(T.cpu().numpy(), D_k2p)
N, st = fa.alignment_distances_batch(seq, counts, model="k2p")
assert dc.same_bits(N, D_k2p) and st["n_recoded"] == 0 and st["n_saturated_problems"] == 0 and st["has_missing"] == 0
# the defaults are the p-distance of before
P0, st0 = fa.alignment_distances_batch(seq, counts)
assert dc.same_bits(P0, dc.pipeline_case()[2]) and "n_recoded" not in st0
# the pipeline: orders and weights are those of the reference's K2P matrices (bit-identical input, same routes)
orders, W, stats = fa.bootstrap(seq, 20, 7, model="k2p")
o_ref = fa.canonical_order_batch(np.array(D_k2p))
w_ref, s_ref = fa.split_weights_batch(np.array(D_k2p), o_ref)
assert (orders == o_ref).all()
assert W.tobytes() == w_ref.tobytes()
assert (stats["splits"]["route"] == s_ref["route"]).all()
# bootstrap_support with JC69: problem 0 is the original alignment (every site once); its rows against a host tally
_, _, D_jc = mc.pipeline_case("jc69")
D0 = mc.ref_clean(seq, np.ones((1, 200), dtype=np.uint16), "jc69")
Dall = np.concatenate([D0, D_jc])
order, w0, table, sst = fa.bootstrap_support(seq, 20, 7, model="jc69", states=4)
o_all = fa.canonical_order_batch(Dall)
w_all, _ = fa.split_weights_batch(Dall, o_all)
assert (order == o_all[0]).all() and w0.tobytes() == w_all[0].tobytes()
ks = np.flatnonzero(w_all[0] > 1e-6)
rows = np.flatnonzero(table["first_b"] == 0)
assert len(rows) == len(ks) and (table["first_k"][rows] == ks).all()
keys0 = fa.split_keys(o_all[0], ks)
assert (table["keys"][rows] == keys0).all()
keys_b = [fa.split_keys(o_all[b], np.flatnonzero(w_all[b] > 1e-6)) for b in range(1, 21)]
for r, key in zip(rows, keys0):    # how many of the 20 replicates hold that split above the threshold
    cnt = sum(int((kb == key).all(axis=1).any()) for kb in keys_b)
    assert table["count"][r] == cnt and table["support"][r] == cnt / 20.0
assert sst["distances"]["n_problems"] == 21
print("DIST_MODEL_DEVICE_OK")
'''


def test_device_entry_and_pipeline():
    """n = 33, L = 200, B = 20, seed 7: bootstrap(model="k2p") returns the orders of canonical_order_batch and, bit for bit, the
    weights of split_weights_batch on the reference's K2P matrices; bootstrap_support(model="jc69") agrees with a host tally on
    the original network's rows; before that the device entry on padded layouts and in chunks."""
    env = dict(os.environ, FNN_ROOT=dc.ROOT)
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DIST_MODEL_DEVICE_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]

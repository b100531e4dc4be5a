"""Gamma-distributed rates for the corrected alignment distances (the epilogues of k_dist_model and k_dist_pairs, fnn_dist.hip,
DESIGN.md section 19) on the GPU: the cases of tests/dist_gamma_common.py through the product, bitwise against its reference of
exact integers and Python floats; the device's dist_expm1 is reached through stored JC69 distances whose shape puts expm1's
argument on either side of every threshold; the device entries and the bootstrap pipeline with a shape in a process of its own
(torch has to be imported before the product's library is loaded for the two to share one HIP runtime)."""
import os
import subprocess
import sys

import pytest

import dist_common as dc
import dist_gamma_common as gc

pytestmark = pytest.mark.gpu

MODELS = gc.MODELS


@pytest.fixture(scope="module")
def a(hip_api):
    assert hip_api.device_count() >= 1
    return hip_api


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


def test_equal_rates_through_the_struct(a):
    gc.check_equal_rates_through_the_struct(a)


@pytest.mark.parametrize("model", MODELS)
def test_both_draw_routes_agree_with_the_counts_entry(a, monkeypatch, model):
    gc.check_bootstrap_entry(a, monkeypatch, model)


def test_arguments(a):
    gc.check_arguments(a)


@pytest.mark.parametrize("model", ["k2p", "tn93"])
def test_chunking(a, monkeypatch, model):
    gc.check_chunking(a, monkeypatch, model)


DEVICE_CHILD = r'''
import os, sys
sys.path.insert(0, os.environ["FNN_ROOT"]); sys.path.insert(0, os.path.join(os.environ["FNN_ROOT"], "tests"))
import numpy as np
import torch                       # first: torch's HIP runtime then serves the product's library too (as in bench.py)
import fastneighbornet_amd as fa
import dist_common as dc
import dist_gamma_common as gc

class Env:                          # (monkeypatch's two calls)
    def setenv(self, k, v): os.environ[k] = v
    def delenv(self, k): del os.environ[k]

a = fa.api()
# the device entries: chunks of 3 at B = 7 into a padded tensor, equal rates through the struct; the wrappers' tensors
for model in ("k2p", "tn93"):
    gc.check_chunking(a, Env(), model, in_place="torch")
gc.check_equal_rates_through_the_struct(a, in_place="torch")
seq, counts, D_ref = gc.pipeline_case("tn93", 0.5)
T, st = fa.alignment_distances_batch(seq, counts, out="torch", model="tn93", gamma_shape=0.5)
assert T.is_cuda and T.dtype == torch.float64 and dc.same_bits(T.cpu().numpy(), D_ref)
N, st = fa.alignment_distances_batch(seq, counts, model="tn93", gamma_shape=0.5)
assert dc.same_bits(N, D_ref) and st["n_saturated_problems"] == 0 and st["has_missing"] == 0
for route in ("device", "host"):    # bootstrap_distances draws the same replicates itself, on the device and on the host
    os.environ["FNN_DRAW_ROUTE"] = route
    B, bst = fa.bootstrap_distances(seq, 20, 7, model="tn93", gamma_shape=0.5)
    del os.environ["FNN_DRAW_ROUTE"]
    assert dc.same_bits(B, D_ref) and bst["draw_route"] == route
# the pipeline: orders and weights are those of the batch calls on the reference's matrices (bit-identical input, same routes)
o_ref = fa.canonical_order_batch(np.array(D_ref))
w_ref, s_ref = fa.split_weights_batch(np.array(D_ref), o_ref)
for draw in ("device", "host"):
    orders, W, stats = fa.bootstrap(seq, 20, 7, model="tn93", gamma_shape=0.5, draw=draw)
    assert (orders == o_ref).all()
    assert W.tobytes() == w_ref.tobytes()
    assert (stats["splits"]["route"] == s_ref["route"]).all()
# bootstrap_support: problem 0 is the original alignment (every site once) under the same shape
D0 = gc.ref_clean(seq, np.ones((1, 200), dtype=np.uint16), "tn93", 0.5)
Dall = np.concatenate([D0, D_ref])
order, w0, table, sst = fa.bootstrap_support(seq, 20, 7, model="tn93", gamma_shape=0.5)
o_all = fa.canonical_order_batch(Dall)
w_all, _ = fa.split_weights_batch(Dall, o_all)
assert (order == o_all[0]).all() and w0.tobytes() == w_all[0].tobytes() and sst["distances"]["n_problems"] == 21
print("DIST_GAMMA_DEVICE_OK")
'''


def test_device_entries_and_pipeline():
    """n = 33, L = 200, B = 20, seed 7: bootstrap(model="tn93", gamma_shape=0.5) returns the orders of canonical_order_batch and, bit
    for bit, the weights of split_weights_batch on the reference's gamma TN93 matrices, on both draw routes; bootstrap_support
    takes the shape for the original data too; before that the device entries in chunks and on padded layouts."""
    env = dict(os.environ, FNN_ROOT=dc.ROOT)
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DIST_GAMMA_DEVICE_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]

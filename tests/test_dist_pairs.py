"""The 4 x 4 tables of state pairs and F81, F84, TN93 and LogDet on them (k_dist_pairs of fnn_dist.hip) on
the GPU: the cases of tests/dist_pairs_common.py through the product, bitwise against its reference of exact integers and Python
floats; the device entries and the bootstrap pipeline with a model in a process of its own (torch has to be imported before the
product's library is loaded for the two to share one HIP runtime)."""
import os
import subprocess
import sys

import pytest

import dist_common as dc
import dist_model_common as mc
import dist_pairs_common as pc

pytestmark = pytest.mark.gpu

MODELS = pc.MODELS
SHAPE_NAMES = ["n%d-L%d-B%d" % dc.SHAPES[k] for k in mc.SHAPE_IDS]


@pytest.fixture(scope="module")
def a(hip_api):
    assert hip_api.device_count() >= 1
    return hip_api


def test_counts_and_lane_maps(a):
    pc.check_counts_lane_maps(a)


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
    """The device's dist_log through the stored distances: r_A / v on both sides of every branch threshold and within 2^-20 of 1."""
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


def test_arguments(a):
    pc.check_arguments(a)
    pc.check_p_entries_refuse_the_models(a)


def test_layout(a):
    pc.check_layout(a)


def test_chunking(a, monkeypatch):
    pc.check_chunking(a, monkeypatch)


DEVICE_CHILD = r'''
import os, sys
sys.path.insert(0, os.environ["FNN_ROOT"]); sys.path.insert(0, os.path.join(os.environ["FNN_ROOT"], "tests"))
import numpy as np
import torch                       # first: torch's HIP runtime then serves the product's library too (as in bench.py)
import fastneighbornet_amd as fa
import dist_common as dc
import dist_pairs_common as pc

class Env:                          # (monkeypatch's two calls)
    def setenv(self, k, v): os.environ[k] = v
    def delenv(self, k): del os.environ[k]

a = fa.api()
# the device entries: layout with sentinels in every padding and chunking, for TN93 and for the tables; the wrappers' tensors
pc.check_layout(a, in_place="torch")
pc.check_chunking(a, Env(), in_place="torch")
seq, counts, D_tn93 = pc.pipeline_case("tn93")
T, st = fa.alignment_distances_batch(seq, counts, out="torch", model="tn93")
assert T.is_cuda and T.dtype == torch.float64 and dc.same_bits(T.cpu().numpy(), D_tn93)
N, st = fa.alignment_distances_batch(seq, counts, model="tn93")
assert dc.same_bits(N, D_tn93) and st["n_recoded"] == 0 and st["n_saturated_problems"] == 0 and st["has_missing"] == 0
F, fst = fa.pair_counts_batch(seq, counts, out="torch")
assert F.is_cuda and F.dtype == torch.int64 and (F.cpu().numpy() == pc.want_tables(seq, counts)).all()
Fn, _ = fa.pair_counts_batch(seq, counts)
assert (Fn == pc.want_tables(seq, counts)).all() and fst["n_pairs"] == 33 * 32 // 2
for model in pc.MODELS:             # bootstrap_distances draws the same replicates itself, on the device and on the host
    Dm = pc.pipeline_case(model)[2]
    for route in ("device", "host"):
        os.environ["FNN_DRAW_ROUTE"] = route
        B, bst = fa.bootstrap_distances(seq, 20, 7, model=model)
        del os.environ["FNN_DRAW_ROUTE"]
        assert dc.same_bits(B, Dm) and bst["draw_route"] == route
# the pipeline: orders and weights are those of the reference's TN93 matrices (bit-identical input, same routes)
orders, W, stats = fa.bootstrap(seq, 20, 7, model="tn93")
o_ref = fa.canonical_order_batch(np.array(D_tn93))
w_ref, s_ref = fa.split_weights_batch(np.array(D_tn93), o_ref)
assert (orders == o_ref).all()
assert W.tobytes() == w_ref.tobytes()
assert (stats["splits"]["route"] == s_ref["route"]).all()
# bootstrap_support with LogDet: problem 0 is the original alignment (every site once); its rows against a host tally
_, _, D_ld = pc.pipeline_case("logdet")
D0 = pc.ref_clean(seq, np.ones((1, 200), dtype=np.uint16), "logdet")
Dall = np.concatenate([D0, D_ld])
order, w0, table, sst = fa.bootstrap_support(seq, 20, 7, model="logdet")
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
print("DIST_PAIRS_DEVICE_OK")
'''


def test_device_entries_and_pipeline():
    """n = 33, L = 200, B = 20, seed 7 (every taxon holds all four bases, the reference is clean): bootstrap(model="tn93") returns
    the orders of canonical_order_batch and, bit for bit, the weights of split_weights_batch on the reference's TN93 matrices;
    bootstrap_support(model="logdet") agrees with a host tally on the original network's rows; before that the device entries
    on padded layouts and in chunks, and bootstrap_distances for every model on both draw routes."""
    env = dict(os.environ, FNN_ROOT=dc.ROOT)
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DIST_PAIRS_DEVICE_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]

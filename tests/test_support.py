"""The split-support stage (fnn_support.hip) on the GPU: the cases of tests/support_common.py through the
product, bytewise against its plain-Python reference; the device entry on a tensor and the whole bootstrap pipeline in a
process of its own (torch has to be imported before the product's library is loaded for the two to share one HIP runtime)."""
import os
import subprocess
import sys

import pytest

import support_common as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def a(hip_api):
    assert hip_api.device_count() >= 1
    return hip_api


@pytest.mark.parametrize("n,B", sc.WORD_EDGES, ids=[f"n{n}-B{B}" for n, B in sc.WORD_EDGES])
def test_word_edges(a, n, B):
    sc.check_word_edge(a, n, B)


def test_both_sides_of_the_fold(a):
    sc.check_fold(a)


def test_order_of_the_sum(a):
    sc.check_sum_order(a)


@pytest.mark.parametrize("lead", sc.LEADS)
def test_lead(a, lead):
    sc.check_lead(a, lead)


def test_threshold(a):
    sc.check_threshold(a)


def test_capacity(a):
    sc.check_capacity(a)


def test_chunking_and_carry(a):
    sc.check_chunking(a)


def test_routes(a):
    sc.check_routes(a)


def test_sparse_keys_do_not_collide(a):
    sc.check_sparse_keys(a)


def test_determinism(a):
    """n = 140, B = 17 twice on the kernel route: other slots, other places inside the segments, the same bytes."""
    orders, W = sc.random_case(140, 17, 1140)
    with sc.switches(route="kernel"):
        t1, S1, st1, _ = sc.call(a, orders, W)
        t2, S2, st2, _ = sc.call(a, orders, W)
    assert S1 == S2 and st1.route == st2.route == 0
    for k in t1:
        assert t1[k].tobytes() == t2[k].tobytes(), k
    sc.assert_table(t1, S1, sc.random_ref(140, 17, 1140))


def test_arguments(a):
    sc.check_arguments(a)
    sc.check_keys(a)


DEVICE_CHILD = r'''
import os, sys
sys.path.insert(0, os.environ["FNN_ROOT"]); sys.path.insert(0, os.path.join(os.environ["FNN_ROOT"], "tests"))
import numpy as np
import torch                       # first: torch's HIP runtime then serves the product's library too (as in bench.py)
import fastneighbornet_amd as fa
import support_common as sc
import dist_common as dc

a = fa.api()
# the device entry: capacity with sentinels, chunks and the carry, both routes (the host route downloads the weights)
sc.check_capacity(a, in_place="torch")
sc.check_chunking(a, in_place="torch")
orders, W = sc.random_case(140, 17, 1140)
for route in ("kernel", "host"):
    sc.check_against(a, orders, W, sc.random_ref(140, 17, 1140), in_place="torch", route=route)
# the pipeline: the table of bootstrap_support is the reference's table of the 21 reference matrices' orders and weights
seq, counts, _ = dc.pipeline_case()
all_counts = np.concatenate([np.ones((1, 200), dtype=np.uint16), counts])
assert (fa.bootstrap_counts(200, 20, 7) == counts).all()
D_ref = dc.ref_dist(seq, all_counts)
o_ref = fa.canonical_order_batch(D_ref)
w_ref, _ = fa.split_weights_batch(D_ref, o_ref)
ref = sc.ref_arrays(sc.ref_table(o_ref, w_ref, 1e-6, 1), 33)
with sc.switches(route="kernel"):
    order, weights, table, stats = fa.bootstrap_support(seq, 20, 7)
assert (order == o_ref[0]).all() and weights.tobytes() == w_ref[0].tobytes()
assert stats["support"]["method"] == "kernel" and stats["support"]["n_problems"] == 21
sc.assert_table(table, stats["support"]["n_splits"], ref)
# the rows with first_b == 0 are exactly the reference network's weights above 1e-6, in ascending k
k0 = np.nonzero(w_ref[0] > 1e-6)[0]
own = table["first_b"] == 0
assert own[:len(k0)].all() and not own[len(k0):].any() and (table["first_k"][:len(k0)] == k0).all()
assert (table["support"] == table["count"] / 20.0).all() and table["count"].max() <= 20
assert fa.split_keys(order, k0).tobytes() == table["keys"][:len(k0)].tobytes()
# W as a tensor on the GPU and as numpy give the same table; so does the default route
for route in ("kernel", None):
    with sc.switches(route=route):
        t_np, s_np = fa.split_support(o_ref, w_ref, lead=1)
        t_gpu, s_gpu = fa.split_support(o_ref, torch.from_numpy(w_ref).to("cuda:0"), lead=1)
    for k in t_np:
        assert t_np[k].tobytes() == t_gpu[k].tobytes() == table[k].tobytes(), k
assert torch.cuda.current_device() == 0
print("SUPPORT_DEVICE_OK")
'''


def test_device_entry_and_pipeline():
    """n = 33, L = 200, B = 20: bootstrap_support returns the table that the Python reference computes from
    canonical_order_batch / split_weights_batch on the 21 reference matrices; before that the device entry on a tensor."""
    env = dict(os.environ, FNN_ROOT=sc.ROOT)
    for k in sc.SWITCHES:
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SUPPORT_DEVICE_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]

"""Bootstrap replicates drawn on the device (k_draw of fnn_dist.hip) on the GPU: the cases of
tests/draw_common.py through the product, bitwise against the reference of Python integers and floats; the device entry and the
bootstrap pipeline over both draw routes in a process of its own (torch has to be imported before the product's library is
loaded for the two to share one HIP runtime)."""
import os
import subprocess
import sys

import pytest

import dist_common as dc
import draw_common as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def a(hip_api):
    assert hip_api.device_count() >= 1
    return hip_api


def test_single_counts_through_matrices(a):
    wc.check_single_counts(a)


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


def test_layout(a):
    wc.check_layout(a)


def test_chunking(a, monkeypatch):
    wc.check_chunking(a, monkeypatch)


@pytest.mark.parametrize("above", [False, True], ids=["at-the-limit", "above"])
def test_site_limit(a, monkeypatch, above):
    wc.check_limit(a, monkeypatch, above)


def test_forced_device_route_above_the_limit(a, monkeypatch):
    wc.check_forced_device_above_the_limit(a, monkeypatch)


@pytest.mark.parametrize("model", wc.MODELS)
def test_forced_host_route(a, monkeypatch, model):
    wc.check_forced_host(a, monkeypatch, model)


def test_empty_pair_in_a_drawn_replicate(a):
    wc.check_empty_pair(a)


def test_saturated_pair_in_a_drawn_replicate(a):
    wc.check_saturated_pair(a)


def test_arguments(a, monkeypatch):
    wc.check_arguments(a, monkeypatch)


def test_two_calls_give_the_same_bytes(a):
    """The histogram is made with integer atomic adds in no fixed order: the bytes must not depend on it."""
    n, L, B, seed = wc.SHAPES[7]
    seq, ref = wc.shape_case(7, "k2p", True)
    outs = [wc.call(a, seq, B, seed, model="k2p")[1].tobytes() for _ in range(2)]
    assert outs[0] == outs[1] and dc.same_bits(wc.call(a, seq, B, seed, model="k2p")[0], ref)


DEVICE_CHILD = r'''
import os, sys
sys.path.insert(0, os.environ["FNN_ROOT"]); sys.path.insert(0, os.path.join(os.environ["FNN_ROOT"], "tests"))
import numpy as np
import torch                       # first: torch's HIP runtime then serves the product's library too (as in bench.py)
import fastneighbornet_amd as fa
import dist_common as dc
import dist_model_common as mc
import draw_common as wc

class Env:                          # (monkeypatch's two calls)
    def setenv(self, k, v): os.environ[k] = v
    def delenv(self, k): del os.environ[k]

a = fa.api()
# the device entry: layout with sentinels in every padding, chunks of three, an empty pair named
wc.check_layout(a, in_place="torch")
wc.check_chunking(a, Env(), in_place="torch")
wc.check_empty_pair(a, in_place="torch")
# the wrapper: a tensor on the GPU, the numpy array, lead = 1, both equal to the counts route and to the reference
seq, counts, D_p = dc.pipeline_case()
T, st = fa.bootstrap_distances(seq, 20, 7, out="torch")
assert T.is_cuda and T.dtype == torch.float64 and dc.same_bits(T.cpu().numpy(), D_p)
assert st["draw_route"] == "device" and st["max_count"] == int(counts.max()) and st["n_problems"] == 20 and st["digit_passes"] == 1
N, st = fa.bootstrap_distances(seq, 20, 7, lead=1, model="k2p")
lead_counts = np.concatenate([np.ones((1, 200), dtype=np.uint16), counts])
assert N.shape == (21, 33, 33) and dc.same_bits(N, mc.ref_clean(seq, lead_counts, "k2p"))
assert dc.same_bits(N, fa.alignment_distances_batch(seq, lead_counts, model="k2p")[0])
# the pipeline: equal orders and bit-equal weights on both draw routes, and those of the reference's matrices
o_dev, W_dev, s_dev = fa.bootstrap(seq, 20, 7, draw="device")
o_host, W_host, s_host = fa.bootstrap(seq, 20, 7, draw="host")
assert (o_dev == o_host).all() and W_dev.tobytes() == W_host.tobytes()
assert (o_dev == fa.canonical_order_batch(np.array(D_p))).all()
assert s_dev["distances"]["draw_route"] == "device" and set(s_host["distances"]) <= set(s_dev["distances"])
# bootstrap_support: byte-equal tables
r_dev = fa.bootstrap_support(seq, 20, 7, draw="device")
r_host = fa.bootstrap_support(seq, 20, 7, draw="host")
assert (r_dev[0] == r_host[0]).all() and r_dev[1].tobytes() == r_host[1].tobytes()
assert sorted(r_dev[2]) == sorted(r_host[2])
for key in r_dev[2]:
    assert r_dev[2][key].tobytes() == r_host[2][key].tobytes(), key
assert r_dev[3]["distances"]["n_problems"] == 21 and r_dev[3]["distances"]["draw_route"] == "device"
print("DRAW_DEVICE_OK")
'''


def test_device_entry_and_pipeline():
    """n = 33, L = 200, B = 20, seed 7: bootstrap(draw="device") and bootstrap(draw="host") return equal orders and bit-equal
    weights, bootstrap_support byte-equal tables; before that the device entry on padded layouts and in chunks."""
    env = dict(os.environ, FNN_ROOT=dc.ROOT)
    for k in ("FNN_BATCH_CHUNK", "FNN_DIST_FORCE_DIGITS", "FNN_DRAW_ROUTE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DRAW_DEVICE_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]

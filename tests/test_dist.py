"""The alignment-distance path (fnn_dist.hip) on the GPU: the cases of tests/dist_common.py through the
product, bitwise against its numpy reference; the device entry and the whole bootstrap pipeline in a process of its own
(torch has to be imported before the product's library is loaded for the two to share one HIP runtime)."""
import os
import subprocess
import sys

import pytest

import dist_common as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def a(hip_api):
    assert hip_api.device_count() >= 1
    return hip_api


@pytest.mark.parametrize("where", sorted(dc.LANE_MAP_SITES))
def test_lane_and_tile_maps(a, where):
    dc.check_lane_maps(a, where)


@pytest.mark.parametrize("k", range(len(dc.SHAPES)), ids=[f"n{n}-L{L}-B{B}" for n, L, B in dc.SHAPES])
def test_shape_edges(a, k):
    dc.check_shape(a, k)


@pytest.mark.parametrize("missing", [False, True])
@pytest.mark.parametrize("cmax,passes", dc.DIGIT_CASES)
def test_digit_planes(a, cmax, passes, missing):
    dc.check_digits(a, cmax, passes, missing)


def test_missing_data(a, monkeypatch):
    dc.check_missing(a, monkeypatch)


@pytest.mark.parametrize("also_an_empty_replicate", [False, True])
def test_pair_without_a_common_site(a, also_an_empty_replicate):
    dc.check_empty_pair(a, also_an_empty_replicate)


def test_layout(a):
    dc.check_layout(a)


def test_chunking(a, monkeypatch):
    dc.check_chunking(a, monkeypatch)


def test_arguments(a):
    dc.check_arguments(a)


DEVICE_CHILD = r'''
import os, sys
sys.path.insert(0, os.environ["FNN_ROOT"]); sys.path.insert(0, os.path.join(os.environ["FNN_ROOT"], "tests"))
import numpy as np
import torch                       # first: torch's HIP runtime then serves the product's library too (as in bench.py)
import fastneighbornet_amd as fa
import dist_common as dc

class Env:                          # (monkeypatch's two calls)
    def setenv(self, k, v): os.environ[k] = v
    def delenv(self, k): del os.environ[k]

a = fa.api()
# the device entry: layout with sentinels in every padding, chunking, and the wrapper's tensor
dc.check_layout(a, in_place="torch")
dc.check_chunking(a, Env(), in_place="torch")
seq, counts, D_ref = dc.pipeline_case()
T, st = fa.alignment_distances_batch(seq, counts, out="torch")
assert T.is_cuda and T.dtype == torch.float64 and tuple(T.shape) == D_ref.shape
assert dc.same_bits(T.cpu().numpy(), D_ref)
N, _ = fa.alignment_distances_batch(seq, counts)
assert dc.same_bits(N, D_ref) and st["digit_passes"] == 1 and st["has_missing"] == 0
assert torch.cuda.current_device() == 0
# the pipeline: orders and weights are those of the reference's numpy matrices (bit-identical input, same routes)
assert (fa.bootstrap_counts(200, 20, 7) == counts).all()
orders, W, stats = fa.bootstrap(seq, 20, 7)
o_ref = fa.canonical_order_batch(np.array(D_ref))
w_ref, s_ref = fa.split_weights_batch(np.array(D_ref), o_ref)
assert (orders == o_ref).all()
assert W.tobytes() == w_ref.tobytes()
assert (stats["splits"]["route"] == s_ref["route"]).all()
o2, W2, _ = fa.bootstrap(seq, 20, 7, weights=False)
assert W2 is None and (o2 == o_ref).all()
print("DIST_DEVICE_OK")
'''


def test_device_entry_and_pipeline():
    """n = 33, L = 200, B = 20: bootstrap() returns the orders of canonical_order_batch and, bit for bit, the weights of
    split_weights_batch on the reference's matrices; before that the device entry on padded layouts and in chunks."""
    env = dict(os.environ, FNN_ROOT=dc.ROOT)
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DIST_DEVICE_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]

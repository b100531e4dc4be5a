"""Alignment distances over site ranges (k_dist_ranges and k_dist_ranges_pairs, fnn_dist.hip) on the GPU: the
cases of tests/dist_ranges_common.py through the product, bitwise against the existing references on the 0/1 counts of the ranges
and, in addition, against the product's own counts entries on those counts; the device entries and the sliding-window pipeline in a
process of its own (torch has to be imported before the product's library is loaded for the two to share one HIP runtime)."""
import os
import subprocess
import sys

import pytest

import dist_common as dc
import dist_ranges_common as rc

pytestmark = pytest.mark.gpu

GRID = [pytest.param(m, s, id=name) for (m, s), name in zip(rc.GRID_MODELS, rc.GRID_MODEL_NAMES)]


@pytest.fixture(scope="module")
def a(hip_api):
    assert hip_api.device_count() >= 1
    return hip_api


def test_range_operand_every_k(a):
    rc.check_operand(a, also_counts=True)


@pytest.mark.parametrize("model,shape", GRID)
@pytest.mark.parametrize("missing", [False, True])
@pytest.mark.parametrize("k", range(len(rc.GRIDS)), ids=rc.GRID_NAMES)
def test_grids(a, k, missing, model, shape):
    rc.check_grid(a, k, missing, model, shape, also_counts=True)


def test_order_and_spans(a):
    rc.check_order_and_spans(a, also_counts=True)


def test_long_walk(a):
    rc.check_long_walk(a, also_counts=True)


def test_failures(a):
    rc.check_failures(a, also_counts=True)


def test_layout(a):
    rc.check_layout(a, also_counts=True)


@pytest.mark.parametrize("model", ["k2p", "tn93"])
def test_chunking(a, monkeypatch, model):
    rc.check_chunking(a, monkeypatch, model)


def test_arguments(a):
    rc.check_arguments(a)


DEVICE_CHILD = r'''
import os, sys
sys.path.insert(0, os.environ["FNN_ROOT"]); sys.path.insert(0, os.path.join(os.environ["FNN_ROOT"], "tests"))
import numpy as np
import torch                       # first: torch's HIP runtime then serves the product's library too (as in bench.py)
import fastneighbornet_amd as fa
import dist_common as dc
import dist_ranges_common as rc
import dist_pairs_common as pc

class Env:                          # (monkeypatch's two calls)
    def setenv(self, k, v): os.environ[k] = v
    def delenv(self, k): del os.environ[k]

a = fa.api()
# the device entries: chunks of 3 at B = 7 into a padded tensor; padded layouts in place
for model in ("k2p", "tn93"):
    rc.check_chunking(a, Env(), model, in_place="torch")
rc.check_layout(a, in_place="torch")
# the wrappers' tensors
seq, starts, ends, D_ref = rc.pipeline_case()
T, st = fa.range_distances(seq, starts, ends, out="torch", model="tn93")
assert T.is_cuda and T.dtype == torch.float64 and dc.same_bits(T.cpu().numpy(), D_ref)
N, st = fa.range_distances(seq, starts, ends, model="tn93")
assert dc.same_bits(N, D_ref) and st["n_saturated_problems"] == 0 and st["has_missing"] == 0 and st["n_site_blocks"] == rc.tile_blocks(starts, ends)
F, _ = fa.pair_counts_ranges(seq, starts, ends, out="torch")
assert F.is_cuda and F.dtype == torch.int64 and (F.cpu().numpy() == pc.want_tables(seq, rc.counts_of(starts, ends, 330))).all()
# the pipeline: orders and weights are those of the batch calls on the reference's matrices (bit-identical input, same routes)
o_ref = fa.canonical_order_batch(np.array(D_ref))
w_ref, s_ref = fa.split_weights_batch(np.array(D_ref), o_ref)
s, e, orders, W, stats = fa.sliding_windows(seq, 128, 6, model="tn93")
assert (s == starts).all() and (e == ends).all() and orders.shape == (len(starts), 34)
assert (orders == o_ref).all()
assert W.tobytes() == w_ref.tobytes()
assert (stats["splits"]["route"] == s_ref["route"]).all() and stats["distances"]["n_problems"] == len(starts)
o2, W2, _ = fa.range_networks(seq, starts[:5], ends[:5], weights=False, model="tn93")
assert W2 is None and (o2 == o_ref[:5]).all()
print("DIST_RANGES_DEVICE_OK")
'''


def test_device_entries_and_pipeline():
    """n = 33, L = 330: sliding_windows(seq, 128, 6, model="tn93") returns the orders of canonical_order_batch and, bit for bit, the
    weights of split_weights_batch on the reference's matrices; before that the device entries in chunks and on padded layouts and
    the wrappers' tensors."""
    env = dict(os.environ, FNN_ROOT=dc.ROOT)
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DIST_RANGES_DEVICE_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]

"""Bootscan - bootstrap replicates inside every site range (k_draw_ranges, k_dist_scan and k_dist_scan_pairs, fnn_dist.hip, DESIGN.md
section 21) - on the GPU: the cases of tests/bootscan_common.py through the product, bitwise against the product's own counts
entries on fnn_bootscan_counts and its bootstrap entry on every window's slice; the routes against each other; the device entries
and the bootscan pipeline in a process of its own (torch has to be imported before the product's library is loaded for the two to
share one HIP runtime)."""
import os
import subprocess
import sys

import pytest

import bootscan_common as bc
import dist_common as dc

pytestmark = pytest.mark.gpu

GRID = [pytest.param(m, s, id=name) for (m, s), name in zip(bc.GRID_MODELS, bc.GRID_MODEL_NAMES)]


@pytest.fixture(scope="module")
def a(hip_api):
    assert hip_api.device_count() >= 1
    return hip_api


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


def test_forced_device_above_the_limit(a, monkeypatch):
    bc.check_forced_device_above_the_limit(a, monkeypatch)


@pytest.mark.parametrize("model", ["k2p", "tn93", "tables"])
def test_chunking(a, monkeypatch, model):
    bc.check_chunking(a, monkeypatch, model)


def test_empty_window(a):
    bc.check_empty_window(a)


def test_empty_pair_inside_one_replicate(a):
    bc.check_empty_pair(a)


def test_saturated_replicate(a):
    bc.check_saturated(a)


def test_arguments(a, monkeypatch):
    bc.check_arguments(a, monkeypatch)


DEVICE_CHILD = r'''
import os, sys
sys.path.insert(0, os.environ["FNN_ROOT"]); sys.path.insert(0, os.path.join(os.environ["FNN_ROOT"], "tests"))
import numpy as np
import torch                       # first: torch's HIP runtime then serves the product's library too (as in bench.py)
import fastneighbornet_amd as fa
import bootscan_common as bc

class Env:                          # (monkeypatch's two calls)
    def setenv(self, k, v): os.environ[k] = v
    def delenv(self, k): del os.environ[k]

a = fa.api()
# the device entries: chunks of 3 at P = 5 into a padded tensor
for model in ("k2p", "tn93", "tables"):
    bc.check_chunking(a, Env(), model, in_place="torch")
# the wrappers' tensors against the counts route's
seq, width, step, R, seed = bc.pipeline_case()
starts, ends = fa.window_ranges(seq.shape[1], width, step)
W, P, n = len(starts), R + 1, seq.shape[0]
counts = fa.bootscan_counts(seq.shape[1], starts, ends, R, seed, lead=1)
D_ref, _ = fa.alignment_distances_batch(seq, counts, model="tn93")
T, st = fa.bootscan_distances(seq, starts, ends, R, seed, out="torch", model="tn93")
assert T.is_cuda and T.dtype == torch.float64 and tuple(T.shape) == (W, P, n, n) and T.cpu().numpy().tobytes() == D_ref.tobytes()
N, st = fa.bootscan_distances(seq, starts, ends, R, seed, model="tn93")
assert N.tobytes() == D_ref.tobytes() and st["n_windows"] == W and st["n_host_chunks"] == 0 and st["draw_route"] == "device"
assert st["n_site_blocks"] == bc.group_blocks(starts, ends, P)
F, _ = fa.bootscan_pair_counts(seq, starts, ends, R, seed, out="torch")
F_ref, _ = fa.pair_counts_batch(seq, counts)
assert F.is_cuda and F.dtype == torch.int64 and tuple(F.shape) == (W, P, n, n, 4, 4) and F.cpu().numpy().tobytes() == F_ref.tobytes()
# the pipeline: orders, weights and support tables are those of the batch calls on the counts route's matrices
o_ref = fa.canonical_order_batch(np.array(D_ref))
w_ref, _ = fa.split_weights_batch(np.array(D_ref), o_ref)
s, e, orders, Wt, tables, stats = fa.bootscan(seq, width, step, R, seed, model="tn93")
assert (s == starts).all() and (e == ends).all() and orders.shape == (W, n + 1) and len(tables) == W
assert (orders == o_ref[::P]).all() and Wt.tobytes() == w_ref[::P].tobytes()
for w in range(W):
    t_ref, _ = fa.split_support(o_ref[w * P:(w + 1) * P], w_ref[w * P:(w + 1) * P], lead=1)
    assert sorted(t_ref) == sorted(tables[w]) and len(t_ref["count"]) > 0
    for k in t_ref:
        assert np.asarray(tables[w][k]).tobytes() == np.asarray(t_ref[k]).tobytes(), (w, k)
assert stats["distances"]["n_problems"] == W * P and len(stats["support"]) == W
print("BOOTSCAN_DEVICE_OK")
'''


def test_device_entries_and_pipeline():
    """n = 12, L = 384: bootscan(seq, 128, 64, R=5, seed, model="tn93") returns the orders of canonical_order_batch, bit for bit the
    weights of split_weights_batch and the tables of split_support on the counts route's matrices; before that the device entries
    in chunks on padded layouts and the wrappers' tensors."""
    env = dict(os.environ, FNN_ROOT=dc.ROOT)
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "BOOTSCAN_DEVICE_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]

"""The batched circular split weights on the GPU (k_small_splits) through
fastneighbornet_amd.split_weights_batch, with orders from canonical_order_batch: the cases of tests/test_splits_batch_emu.py
on the real kernel, the comparison with the one-problem solver, the fallback behind the kernel, the device entry and the
whole batched pipeline."""
import types

import numpy as np
import pytest

import common
import inputs
import splits_batch_common as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa(hip_api):
    import fastneighbornet_amd
    return fastneighbornet_amd


@pytest.fixture(scope="module")
def max_n(hip_api):
    return hip_api.split_weights_batch_max_n()


@pytest.fixture(autouse=True)
def kernel_route(monkeypatch):
    """Every case here is for the kernel, also below the batch from which the call takes it by default."""
    monkeypatch.setenv("FNN_SW_BATCH_ROUTE", "kernel")


def caller(fa):
    def call(D, orders, **kw):
        w, s = fa.split_weights_batch(D, orders, **kw)
        st = types.SimpleNamespace(**s["call"])
        st.as_dict = lambda: s["call"]
        return w, s, st
    return call


def test_limits(hip_api, max_n):
    assert max_n >= hip_api.batch_lds_max_n() >= 140
    assert [hip_api.split_weights_batch_min_batch(n) for n in (32, 64, 96, 128, max_n)] == [1, 4, 8, 16, 32]


def test_default_route_below_the_crossover(fa, monkeypatch):
    """Without the switch, fewer problems than fnn_split_weights_batch_min_batch(n) go through the one-problem solver."""
    monkeypatch.delenv("FNN_SW_BATCH_ROUTE")
    D, orders = sc.synth_batch(64, 4)
    w4, s4 = fa.split_weights_batch(D, orders)
    w3, s3 = fa.split_weights_batch(D[:3], orders[:3])
    assert s4["call"]["n_kernel"] == 4 and s4["call"]["n_fallback"] == 0
    assert s3["call"]["n_kernel"] == 0 and s3["call"]["n_fallback"] == 3
    assert np.abs(w3 - w4[:3]).max() <= 1e-6 * max(1.0, np.abs(w4).max())


@pytest.mark.parametrize("n", [4, 5, 33, 64, 65, 128, "max_n"])
def test_parity(fa, max_n, n):
    pytest.importorskip("scipy")
    n = max_n if n == "max_n" else n
    w, sw, st = sc.check_parity(caller(fa), n, max_n, orders_of=fa.canonical_order_batch)
    if n <= 64:   # the optimum is unique: the kernel's method and the one-problem solver must meet
        D, orders = sc.synth_batch(n, sc.batch_size(n, max_n))
        for b in range(D.shape[0]):
            one, _ = fa.split_weights(D[b], orders[b])
            assert np.abs(w[b] - one).max() <= 1e-6 * max(1.0, np.abs(one).max()), (n, b, np.abs(w[b] - one).max())


def test_closed_form_route(fa):
    sc.check_closed_form(caller(fa))


def test_zeros_to_find(fa):
    sc.check_zeros_to_find(caller(fa))


@pytest.mark.parametrize("n", [16, 64])
def test_tree_metric_with_degenerate_multipliers(fa, n):
    sc.check_tree_metric(caller(fa), n, orders_of=fa.canonical_order_batch)


@pytest.mark.parametrize("n", [9, 64])
def test_padding_is_never_read(fa, max_n, n):
    def a_run(buf, n_, ld, stride, B, orders):
        view = np.lib.stride_tricks.as_strided(buf, shape=(B, n_, n_), strides=(stride * 8, ld * 8, 8), writeable=False)
        return caller(fa)(view, orders)
    sc.check_padding(a_run, n, max_n)


@pytest.mark.parametrize("n", [9, 65])
def test_chunking(fa, n, monkeypatch):
    sc.check_chunking(caller(fa), n, monkeypatch)


def test_determinism(fa):
    sc.check_determinism(caller(fa), 33)


def test_fallback_behind_the_kernel(fa, monkeypatch):
    """FNN_SW_BATCH_CAP=8 at n = 12: the problems whose free set outgrows 8 splits go through the one-problem solver."""
    D, orders = sc.synth_batch(12, 6)
    monkeypatch.setenv("FNN_SW_BATCH_CAP", "8")
    w, s = fa.split_weights_batch(D, orders)
    monkeypatch.delenv("FNN_SW_BATCH_CAP")
    assert s["call"]["n_fallback"] > 0 and s["call"]["n_fallback"] + s["call"]["n_kernel"] + s["call"]["n_closed_form"] == 6
    assert s["call"]["capacity"] == 8
    for b in range(6):
        one, _ = fa.split_weights(D[b], orders[b])
        assert np.abs(w[b] - one).max() <= 1e-6 * max(1.0, np.abs(one).max()), (b, np.abs(w[b] - one).max())
    assert (s["certified"] == 1).all()


def test_above_the_limit_goes_through_the_one_problem_solver(fa, max_n):
    n = max_n + 1
    D, orders = sc.synth_batch(n, 2)
    w, s = fa.split_weights_batch(D, orders)
    assert s["call"]["n_fallback"] == 2 and s["call"]["n_kernel"] == 0 and s["call"]["chunks"] == 0
    for b in range(2):
        assert common.kkt_violation(D[b], orders[b], w[b]) < 1e-9


DEVICE_ENTRY_CHILD = r'''
import os, sys
sys.path.insert(0, os.environ["FNN_ROOT"]); sys.path.insert(0, os.path.join(os.environ["FNN_ROOT"], "tests"))
import numpy as np
import torch                       # first: torch's HIP runtime then serves the product's library too (as in bench.py)
import fastneighbornet_amd as fa
import splits_batch_common as sc
for n in (33, 64):                 # odd n, even n
    D, orders = sc.synth_batch(n, 4)
    T = torch.from_numpy(np.array(D)).to("cuda:0")
    assert T.dtype == torch.float64
    w0, s0 = fa.split_weights_batch(np.array(D), orders)
    w1, s1 = fa.split_weights_batch(T, orders)
    assert w0.tobytes() == w1.tobytes(), n
    assert s1["call"]["n_fallback"] == 0 and (s1["certified"] == 1).all() and (s1["route"] == s0["route"]).all()
    o = fa.canonical_order_batch(T)  # the pipeline on the device: orders from the order batch's device entry
    assert (o == orders).all()
    w2, _ = fa.split_weights_batch(T, torch.from_numpy(np.array(o)))
    assert w2.tobytes() == w0.tobytes()
print("DEVICE_ENTRY_OK")
'''


def test_device_entry():
    """A torch.float64 tensor on the GPU (odd n, even n) gives the bits of the host entry.  In a process of its own: torch has
    to be imported before the product's library is loaded for the two to share one HIP runtime (as tests/test_batch.py does)."""
    import os
    import subprocess
    import sys
    env = dict(os.environ, FNN_ROOT=sc.ROOT)
    r = subprocess.run([sys.executable, "-c", DEVICE_ENTRY_CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DEVICE_ENTRY_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_whole_batched_pipeline(fa, oracle):
    """canonical_order_batch then split_weights_batch on 16 tree-like problems of 48 taxa."""
    D = np.stack([inputs.make(48, "treenoise", 20 + b, oracle) for b in range(16)])
    orders = fa.canonical_order_batch(D)
    w, s = fa.split_weights_batch(D, orders)
    assert (s["certified"] == 1).all() and s["call"]["n_fallback"] == 0
    assert (w >= 0).all()
    for b in (0, 15):
        assert common.kkt_violation(D[b], orders[b], w[b]) < 1e-9


# ---- the safety net, through the test switches (splits_batch_common); which problems give up says the CPU driver -------

@pytest.fixture(scope="module")
def emu():
    return sc.emu_api()


@pytest.fixture(scope="module")
def hip_call(hip_api):
    return lambda D, orders, **kw: sc.run(hip_api, np.ascontiguousarray(D), orders, **kw)


@pytest.fixture(scope="module")
def solve(hip_api, emu):
    return sc.product_solver(hip_api, emu)


@pytest.fixture(scope="module")
def single(fa):
    return lambda D, order: fa.split_weights(D, order)[0]


def test_set_aside_release_and_recheck(solve, single, monkeypatch):
    """The kernel itself certified 35 of the 40 problems on the CPU driver (tests/test_splits_batch_emu.py); the GPU has to
    agree, problem by problem, and the five others come back through the one-problem solver."""
    pytest.importorskip("scipy")
    n_solved, n_all, total = sc.check_set_aside(solve, single, monkeypatch)
    assert (n_solved, n_all) == (35, 40), (n_solved, n_all)


def test_give_up_by_steps(solve, single, monkeypatch):
    sc.check_step_limit(solve, single, monkeypatch)


def test_give_up_uncertified(solve, single, monkeypatch):
    pytest.importorskip("scipy")
    sc.check_uncertified_end(solve, single, monkeypatch)


@pytest.mark.parametrize("n", [8, 33, 64, 65, 96, 97, "max_n"])
def test_input_classes(hip_call, max_n, n):
    pytest.importorskip("scipy")
    sc.check_classes(hip_call, max_n if n == "max_n" else n)


@pytest.mark.parametrize("n", [33, 65])
def test_foreign_orderings(hip_call, n):
    pytest.importorskip("scipy")
    sc.check_foreign_orderings(hip_call, n)


@pytest.mark.parametrize("n", [2, 3, 8, 65])
def test_constant_and_zero_matrices(hip_call, n):
    sc.check_flat(hip_call, n)


@pytest.mark.parametrize("n", [33, 65])
def test_power_of_two_scaling_is_exact(hip_call, n):
    sc.check_power_of_two(hip_call, n)

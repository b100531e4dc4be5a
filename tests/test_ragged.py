"""The ragged batch calls on the GPU (k_small_ragged, k_small_splits_ragged): the cases of
tests/test_ragged_emu.py against the product through the host entry, the same through the device entry (a torch tensor's
pointer, in a process of its own), the problems outside the kernels' range, and the Python entry."""
import os
import subprocess
import sys

import numpy as np
import pytest

import batch_common as bc
import ragged_common as rc
import splits_batch_common as sc
from fastneighbornet_amd import _capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa(hip_api):
    import fastneighbornet_amd
    return fastneighbornet_amd


@pytest.fixture(scope="module")
def drv(hip_api):
    return rc.Driver(hip_api)


@pytest.fixture(autouse=True)
def kernel_route(monkeypatch):
    """The weight cases are for the kernel, also below the batch from which the call takes it by default."""
    monkeypatch.setenv("FNN_SW_BATCH_ROUTE", "kernel")


def same_calls(api):
    """The product's same-size calls: orders with events, and the weights of the kernel route."""
    return (lambda D: bc.run(api, D, events=True)[:3]), \
        (lambda D, o: sc.run(api, np.ascontiguousarray(D), np.ascontiguousarray(o, dtype=np.int32))[0])


def test_mixed_sizes_in_one_call(drv, hip_api):
    rc.check_mixed(drv, hip_api.batch_lds_max_n())


def test_outputs_follow_the_callers_numbering(drv, hip_api):
    rc.check_numbering(drv, hip_api.batch_lds_max_n())


def test_equal_sizes_give_the_same_size_calls_bytes(drv, hip_api):
    rc.check_equal_sizes(drv, *same_calls(hip_api))


def test_chunking(drv, monkeypatch):
    rc.check_chunking(drv, monkeypatch)


def test_validation(drv):
    rc.check_validation(drv)


def test_weights_of_the_mixed_batch(drv, hip_api):
    pytest.importorskip("scipy")
    rc.check_weights(drv, hip_api.split_weights_batch_max_n(), same_calls(hip_api)[1])


def test_safety_net_in_one_mixed_call(drv, fa, hip_api, monkeypatch):
    pytest.importorskip("scipy")
    emu = sc.emu_api()
    rc.check_safety_net(drv, rc.emu_api(), sc.product_solver(hip_api, emu), lambda D, o: fa.split_weights(D, o)[0], monkeypatch)


@pytest.mark.parametrize("streams", ["1", "2", "4"])
def test_stream_count_does_not_show(drv, hip_api, monkeypatch, streams):
    """The classes of a chunk spread over one, two or four streams give the same results, orders and weights."""
    monkeypatch.setenv("FNN_RAGGED_STREAMS", streams)
    rc.check_mixed(drv, hip_api.batch_lds_max_n())
    mats, refs = rc.mixed((5, 9, 33, 65, 8, 97, 64, 12))
    w, sw, _ = drv.weights(rc.Layout(mats), [r[0] for r in refs])
    assert (sw["certified"] == 1).all()
    monkeypatch.delenv("FNN_RAGGED_STREAMS")
    w0, _, _ = drv.weights(rc.Layout(mats), [r[0] for r in refs])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(w, w0))


def out_of_range_orders(drv, fa, lds_max_n, oracle):
    mats, refs = rc.mixed(rc.mixed_sizes(lds_max_n))
    large = [oracle.synth(n, 60 + k, "uniform53") for k, n in enumerate((150, lds_max_n + 1, 150, 150, lds_max_n + 1, 150))]
    where = (2, 5, 9, 9, 14, 20)                       # spread over the batch
    allm, expect = list(mats), [r[0] for r in refs]
    for pos, D in zip(where, large):
        allm.insert(pos, D)
        expect.insert(pos, fa.canonical_order(D))
    orders, ev, nev, st = drv.orders(rc.Layout(allm, nan_below=4), events=True)
    assert st.n_fallback == 2 and st.n_global == 4 and st.n_lds == sum(1 for m in mats if m.shape[0] >= 4), st.as_dict()
    assert st.n_problems == len(allm)
    for b, want in enumerate(expect):
        assert (orders[b] == want).all(), (b, allm[b].shape[0])
        assert 0 <= nev[b] < max(allm[b].shape[0], 1)


def test_orders_outside_the_kernel_range(drv, fa, hip_api, oracle):
    """Two problems of lds_max_n + 1 taxa (the one-problem engine) and four of 150 (the global-memory kernel) among the mixed
    batch: grouped by size and handed to the same-size entry, every result back at the caller's index."""
    out_of_range_orders(drv, fa, hip_api.batch_lds_max_n(), oracle)


def out_of_range_weights(drv, fa, max_n, setenv, delenv):
    D, so = sc.synth_batch(12, 6)
    big, big_o = sc.synth_batch(max_n + 1, 1)
    probs = [rc.problem(5, 1), (big[0], (big_o[0],)), rc.problem(4, 0), (D[0], (so[0],)), rc.problem(7, 2)]
    mats, orders = [p[0] for p in probs], [p[1][0] for p in probs]
    setenv("FNN_SW_BATCH_CAP", "8")                    # the 12-taxon problem outgrows 8 splits (tests/test_ragged_emu.py); 4, 5 and 7 taxa do not
    w, sw, st = drv.weights(rc.Layout(mats), orders)
    delenv("FNN_SW_BATCH_CAP")
    assert st.n_fallback == 2 and st.n_kernel + st.n_closed_form == 3 and st.n_problems == 5, st.as_dict()
    assert (sw["certified"] == 1).all()
    for b in (1, 3):
        one, _ = fa.split_weights(mats[b], orders[b])
        assert w[b].tobytes() == one.tobytes(), (b, np.abs(w[b] - one).max())


def test_weights_outside_the_kernel_range(drv, fa, hip_api, monkeypatch):
    """One problem above the kernel's limit and one that gives up in its workgroup: both through the one-problem solver."""
    out_of_range_weights(drv, fa, hip_api.split_weights_batch_max_n(), monkeypatch.setenv, monkeypatch.delenv)


def test_default_route_counts_the_kernel_range(fa, monkeypatch):
    """Without the switch the kernel is taken from fnn_split_weights_batch_min_batch(largest n in range) problems on."""
    monkeypatch.delenv("FNN_SW_BATCH_ROUTE")
    D, so = sc.synth_batch(64, 4)
    mats, orders = [D[b] for b in range(4)] + [rc.problem(9, 3)[0]], [so[b] for b in range(4)] + [rc.problem(9, 3)[1][0]]
    _, s5 = fa.split_weights_ragged(mats, orders)                 # five in range, the largest of 64 taxa: the kernel from 4 on
    _, s3 = fa.split_weights_ragged(mats[2:], orders[2:])         # three
    assert s5["call"]["n_fallback"] == 0 and s5["call"]["n_kernel"] + s5["call"]["n_closed_form"] == 5
    assert s3["call"]["n_fallback"] == 3 and s3["call"]["chunks"] == 0


def test_python_entry(fa, oracle):
    """canonical_order_ragged then split_weights_ragged on eight matrices of 5 ... 140 taxa: what canonical_order and
    split_weights give for each matrix: the orders exactly, the weights within the tolerance tests/test_splits_batch.py uses
    between the kernel and the one-problem solver (1e-6 * max(1, largest weight)), and certified by the host's own check."""
    sizes = (5, 140, 33, 64, 97, 12, 65, 20)
    mats = [oracle.synth(n, 80 + k, ("uniform53", "dec4")[k % 2]) for k, n in enumerate(sizes)]
    orders, ev, nev = fa.canonical_order_ragged(mats, events=True)
    w, s = fa.split_weights_ragged(mats, orders)
    assert (s["certified"] == 1).all() and s["call"]["n_fallback"] == 0 and s["call"]["n_problems"] == 8
    import common
    for b, D in enumerate(mats):
        assert (orders[b] == fa.canonical_order(D)).all(), b
        assert len(ev[b]) == nev[b] and 1 <= nev[b] < sizes[b]
        one, _ = fa.split_weights(D, orders[b])
        print(f"n = {sizes[b]}: max |w - one-problem solver| = {np.abs(w[b] - one).max():.3e}, max weight {np.abs(one).max():.3e}")
        assert np.abs(w[b] - one).max() <= 1e-6 * max(1.0, np.abs(one).max()), (b, np.abs(w[b] - one).max())
        assert common.kkt_violation(D, orders[b], w[b]) < 1e-9


DEVICE_ENTRY_CHILD = r'''
import os, sys
sys.path.insert(0, os.environ["FNN_ROOT"]); sys.path.insert(0, os.path.join(os.environ["FNN_ROOT"], "tests"))
import numpy as np
import torch                       # first: torch's HIP runtime then serves the product's library too (as in bench.py)
import fastneighbornet_amd as fa
import ragged_common as rc
import test_ragged as tr
from oracle import nnet_oracle
os.environ["FNN_SW_BATCH_ROUTE"] = "kernel"

class Env:
    def setenv(self, k, v): os.environ[k] = v
    def delenv(self, k): os.environ.pop(k, None)

def place(buf):                    # the buffer on the GPU, NaN gaps and all; the producer synchronised
    t = torch.from_numpy(np.array(buf)).to("cuda:0")
    torch.cuda.synchronize()
    return t.data_ptr(), t

api = fa.api()
drv = rc.Driver(api, on_device=True, place=place)
lds_max_n, max_n = api.batch_lds_max_n(), api.split_weights_batch_max_n()
rc.check_mixed(drv, lds_max_n)
rc.check_numbering(drv, lds_max_n)
rc.check_equal_sizes(drv, *tr.same_calls(api))
rc.check_chunking(drv, Env())
rc.check_validation(drv)
rc.check_weights(drv, max_n, tr.same_calls(api)[1])
tr.out_of_range_orders(drv, fa, lds_max_n, nnet_oracle)
tr.out_of_range_weights(drv, fa, max_n, Env().setenv, Env().delenv)
# the Python entry with tensors on the GPU: the bits of the host entry
mats = [nnet_oracle.synth(n, 90 + n, "uniform53") for n in (9, 64, 33, 100)]
o0 = fa.canonical_order_ragged(mats)
w0, _ = fa.split_weights_ragged(mats, o0)
T = [torch.from_numpy(m).to("cuda:0") for m in mats]
o1 = fa.canonical_order_ragged(T)
w1, s1 = fa.split_weights_ragged(T, o1)
assert all((a == b).all() for a, b in zip(o0, o1)) and all(a.tobytes() == b.tobytes() for a, b in zip(w0, w1))
assert s1["call"]["n_fallback"] == 0
print("DEVICE_ENTRY_OK")
'''


def test_device_entry():
    """Every case above through the device entries (the matrices read in place on the GPU: odd offsets by element loads, dense
    aligned problems by 16-byte loads).  In a process of its own: torch has to be imported before the product's library is
    loaded for the two to share one HIP runtime (as tests/test_batch.py does)."""
    env = dict(os.environ, FNN_ROOT=bc.ROOT)
    r = subprocess.run([sys.executable, "-c", DEVICE_ENTRY_CHILD], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DEVICE_ENTRY_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]

"""The batched path above the LDS limit on the GPU (k_small_global in fnn_batch.hip): one workgroup per
problem, the matrix in a working copy in global memory, against the oracle event by event; the routing between the LDS
kernel, this kernel and the engine loop; the host logic around it (chunking, padding, validation, the device entry).  The
same cases run on the CPU driver in tests/test_batch_global_emu.py."""
import numpy as np
import pytest

import batch_common as bc
import batch_global_common as bg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def a(hip_api):
    return hip_api


def test_limits(a):
    assert a.batch_lds_max_n() < a.batch_global_max_n() <= 1024
    assert all(a.batch_global_min_batch(n) >= 4 for n in (141, 256, 512, 1024))


@pytest.mark.parametrize("n", bg.FORCED_SIZES)
def test_parity_on_the_forced_route(a, n, monkeypatch):
    bg.check_forced_parity(a, n, monkeypatch)


@pytest.mark.parametrize("threads", [256, 1024])
def test_thread_counts(a, threads, monkeypatch):
    bg.check_threads(a, threads, monkeypatch)


def test_default_route_and_engine_override(a, monkeypatch):
    D, orders, ev, nev = bg.check_default_route(a, monkeypatch)
    monkeypatch.setenv("FNN_BATCH_ROUTE", "engine")     # the parent commit's only path for these sizes
    o2, e2, n2, st = bc.run(a, D, events=True)
    assert st.n_fallback == 8 and st.n_global == 0
    assert (o2 == orders).all() and (n2 == nev).all() and e2.tobytes() == ev.tobytes()


def test_engine_route_on_mixed_classes(a, monkeypatch):
    """FNN_BATCH_ROUTE=engine: the seven input classes run one after another on the fallback's single engine handle (`fallback`
    in fnn_batch.hip), so each problem but the first starts in the buffers the previous class left behind - exact ties, zero
    distances, negative entries (plain fp64 scans), an outgroup.  Against the oracle event by event.  (The CPU drivers of the
    batch routes have no engine route: tests/test_batch_global_emu.py::test_engine_override.)"""
    monkeypatch.setenv("FNN_BATCH_ROUTE", "engine")
    D, refs = bc.class_batch(150)
    orders, ev, nev, st = bc.run(a, D, events=True)
    assert st.n_fallback == len(bc.CLASSES) == 7 and st.n_global == 0 and st.n_lds == 0, st.as_dict()
    bc.assert_matches_oracle(orders, ev, nev, refs, ("engine route", 150))


def test_cap(a, monkeypatch):
    bg.check_cap(a, monkeypatch)


def test_above_the_cap_goes_to_the_engine(a, monkeypatch):
    monkeypatch.delenv("FNN_BATCH_ROUTE", raising=False)
    D = bg.above_cap_batch(a)
    B, n = D.shape[0], D.shape[1]
    orders, _, _, st = bc.run(a, D)
    assert st.n_fallback == B and st.n_global == 0 and st.n_lds == 0
    assert (np.sort(orders[:, 1:], axis=1) == np.arange(1, n + 1)[None, :]).all()


def test_more_workgroups_than_fit(a, monkeypatch):
    bg.check_many(a, monkeypatch)


@pytest.mark.parametrize("n", [9, 141])
def test_padding_is_never_read_and_nothing_written(a, n, monkeypatch):
    bg.check_padding(a, n, monkeypatch)


def test_validation(a, monkeypatch):
    bg.check_validation(a, monkeypatch)


def test_asymmetric_input_as_in_the_lds_route(a, monkeypatch):
    bg.check_asymmetric_like_lds(a, a, monkeypatch)


DEVICE_ENTRY_CHILD = r'''
import os, sys
sys.path.insert(0, os.environ["FNN_ROOT"]); sys.path.insert(0, os.path.join(os.environ["FNN_ROOT"], "tests"))
import numpy as np
import torch                       # first: torch's HIP runtime then serves the engine's library too (as in bench.py)
import fastneighbornet_amd as fa
import batch_common as bc
n, B = 141, 8
D, refs = bc.dec4_batch(n, B, seed0=1100)
T = torch.from_numpy(np.array(D)).to("cuda:0")
assert T.dtype == torch.float64 and tuple(T.shape) == (B, n, n)
keep = T.clone()
orders, ev, nev = fa.canonical_order_batch(T, events=True, validate=True)
bc.assert_matches_oracle(orders, ev, nev, refs, "device entry")
assert torch.equal(T.view(torch.int64), keep.view(torch.int64))      # the caller's tensor is never written
orders2 = fa.canonical_order_batch(T)                                 # ... so a second call finds the same matrices
assert (orders2 == orders).all()
big = np.full((B, n + 7, n + 3), np.nan)     # a strided view goes through ld and stride, not through a copy
big[:, :n, :n] = D
assert (fa.canonical_order_batch(big[:, :n, :n]) == orders).all()
print("DEVICE_ENTRY_OK")
'''


def test_device_entry_and_python_wrapper():
    """A torch.float64 tensor on the GPU goes to the device entry, which copies each problem into a working buffer of its own.
    In a process of its own, as in tests/test_batch.py."""
    import os
    import subprocess
    import sys
    env = dict(os.environ, FNN_ROOT=bc.ROOT)
    env.pop("FNN_BATCH_ROUTE", None)
    r = subprocess.run([sys.executable, "-c", DEVICE_ENTRY_CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DEVICE_ENTRY_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]

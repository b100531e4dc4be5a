"""The batched small-problem path on the GPU (k_small in fnn_batch.hip): one workgroup per problem, out
of LDS, against the oracle event by event; the host logic around it (identities, chunking, padding, validation, the
fallback above the LDS limit, the device entry).  The same cases run on the CPU driver in tests/test_batch_emu.py."""
import ctypes as C

import numpy as np
import pytest

import batch_common as bc
from fastneighbornet_amd import _capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def a(hip_api):
    return hip_api


@pytest.mark.parametrize("n", bc.SMALL_SIZES + ("lds_max_n",))
def test_parity_with_oracle(a, n):
    bc.check_parity(a, a.batch_lds_max_n() if n == "lds_max_n" else n)


def test_identities_without_a_launch(a):
    bc.check_identities(a)


def test_many_problems(a):
    bc.check_many(a)


@pytest.mark.parametrize("n", [9, 64])
def test_padding_is_never_read(a, n):
    bc.check_padding(a, n)


@pytest.mark.parametrize("n", [9, 65])
def test_chunking(a, n, monkeypatch):
    bc.check_chunking(a, n, monkeypatch)


def test_validation(a, monkeypatch):
    bc.check_validation(a, monkeypatch)


def test_fallback_above_the_lds_limit(a, oracle):
    n, B = a.batch_lds_max_n() + 1, 3
    D, refs = bc.dec4_batch(n, B, seed0=800)
    orders, ev, nev, st = bc.run(a, D, events=True)
    assert st.n_fallback == 3 and st.n_lds == 0
    bc.assert_matches_oracle(orders, ev, nev, refs, "fallback")
    opts = _capi.FnnOpts()
    for b in range(B):
        one = np.zeros(n + 1, dtype=np.int32)
        a.check(a.canonical_order_f64(D[b].ctypes.data_as(C.POINTER(C.c_double)), n, n, C.byref(opts),
                                      one.ctypes.data_as(C.POINTER(C.c_int32)), None))
        assert (one == orders[b]).all(), b


def test_cross_check_with_the_engine(a):
    """n = 64, B = 8: the batch's events are the events of the one-problem engine."""
    D, _ = bc.dec4_batch(64, 8, seed0=900)
    orders, ev, nev, _ = bc.run(a, D, events=True)
    for b in range(8):
        with _capi.Handle(a, 64, record_events=True) as h:
            h.set_matrix(D[b])
            o, _ = h.run()
            bc.assert_same_events(ev[b], int(nev[b]), h.events(), b)
        assert (o == orders[b]).all()


DEVICE_ENTRY_CHILD = r'''
import os, sys
sys.path.insert(0, os.environ["FNN_ROOT"]); sys.path.insert(0, os.path.join(os.environ["FNN_ROOT"], "tests"))
import numpy as np
import torch                       # first: torch's HIP runtime then serves the engine's library too (as in bench.py)
import fastneighbornet_amd as fa
import batch_common as bc
D, refs = bc.class_batch(33)
T = torch.from_numpy(np.array(D[:6])).to("cuda:0")
assert T.dtype == torch.float64 and tuple(T.shape) == (6, 33, 33)
o_dev = fa.canonical_order_batch(T)
o_host = fa.canonical_order_batch(T.cpu().numpy())
assert (o_dev == o_host).all()
for b in range(6):
    assert (o_dev[b] == refs[b][0]).all(), b
o2, ev, nev = fa.canonical_order_batch(T, events=True, validate=True)
bc.assert_matches_oracle(o2, ev, nev, refs[:6], "device entry")
big = np.full((6, 40, 36), np.nan)          # a strided view goes through ld and stride, not through a copy
big[:, :33, :33] = D[:6]
assert (fa.canonical_order_batch(big[:, :33, :33]) == o_host).all()
D64, refs64 = bc.class_batch(64)             # even n on the device: the 16-byte loads
o64 = fa.canonical_order_batch(torch.from_numpy(np.array(D64)).to("cuda:0"))
for b in range(len(refs64)):
    assert (o64[b] == refs64[b][0]).all(), b
print("DEVICE_ENTRY_OK")
'''


def test_device_entry_and_python_wrapper():
    """A torch.float64 tensor on the GPU goes to the device entry.  In a process of its own: torch has to be imported before
    the engine's library is loaded for the two to share one HIP runtime (tests/test_multi_rank.py does the same)."""
    import os
    import subprocess
    import sys
    env = dict(os.environ, FNN_ROOT=bc.ROOT)
    r = subprocess.run([sys.executable, "-c", DEVICE_ENTRY_CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DEVICE_ENTRY_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]

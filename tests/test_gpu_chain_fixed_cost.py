"""GPU: the exact sequential sum after the cut of its fixed costs (DPP scans, one scan of the waves' totals, a walk that
enters only lane groups with an event, the short form below CH_SHORT_M addends) must still equal the scalar loop bit for
bit - on the adversarial inputs of the CPU model test and at every size at which the new code takes another path.

fnn_test_chain_sum hands the kernel a buffer of whole super-chunks whose tail behind the m addends holds NaN: a load or a
lane that is not masked by m shows in the sum."""
import ctypes as C

import numpy as np
import pytest

from test_chain_sum import chain_cases

pytestmark = pytest.mark.gpu

EDGE_SIZES = (1, 2, 31, 32, 33, 63, 64, 65,      # thread and wave edges
              2047, 2048, 2049,                  # lane-group edge of the walk (64 threads x 32 addends)
              32767, 32768, 32769)               # super-chunk edge; 32769: second iteration, masked tail


def serial_sum(v):
    s = 0.0
    for x in v.tolist():
        s += x
    return s


def edge_cases(short_m):
    rng = np.random.default_rng(11)
    cases = {}
    for m in sorted(set(EDGE_SIZES + (short_m - 1, short_m, short_m + 1))):  # ... and the short form's threshold
        cases[f"uniform_{m}"] = rng.random(m) + 2.0 ** -10
        cases[f"dec4_{m}"] = np.floor(rng.random(m) * 1e4 + 1) / 1e4
    return cases


@pytest.fixture(scope="module")
def short_m(hip_api):
    """The library's own threshold (fnn_hip.hip: CH_SHORT_M): sums of fewer addends take the short form."""
    fn = hip_api._fn("test_chain_short_below", C.c_int32, [])
    m = fn()
    assert 1 < m <= 64 * 32  # one wave, one 32-addend chunk per lane
    return m


@pytest.fixture(scope="module")
def all_cases(short_m):
    cases = dict(chain_cases())
    cases.update(edge_cases(short_m))
    return [(name, np.ascontiguousarray(v, dtype=np.float64), serial_sum(v)) for name, v in cases.items()]


@pytest.mark.parametrize("guard", [22, 0])
def test_chain_sum_is_bit_exact_at_every_path(hip_api, all_cases, short_m, guard):
    seen = np.zeros(4, dtype=np.int64)
    for name, v, ref in all_cases:
        out = C.c_double(0.0)
        st = (C.c_int32 * 4)()
        hip_api.check(hip_api.test_chain_sum(0, v.ctypes.data_as(C.POINTER(C.c_double)), len(v), guard, 32, C.byref(out), st))
        a = np.array([out.value]).view(np.int64)[0]
        b = np.array([ref]).view(np.int64)[0]
        assert a == b or (np.isnan(out.value) and np.isnan(ref)), (name, out.value, ref, list(st))
        if len(v) < short_m:
            assert list(st) == [0, 0, 0, 0], (name, list(st))  # the short form: no records, no runs
        seen += np.array(list(st))
    assert seen[0] > 0 and seen[1] > 0

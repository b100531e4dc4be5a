"""The batched path above the LDS limit (fnn_small_global.h) on the CPU: the per-thread phase bodies
run for tid = 0 ... nthreads-1, phase by phase, by tests/emu/fnn_batch_global_emu.cpp under the product's own host logic,
against the oracle event by event; and the stand-alone AddressSanitizer / UBSan program over the same driver."""
import os
import subprocess

import numpy as np
import pytest

import batch_common as bc
import batch_global_common as bg
from fastneighbornet_amd import _capi


@pytest.fixture(scope="module")
def a():
    return bg.emu_global_api()


def test_limits(a):
    assert a.batch_lds_max_n() < a.batch_global_max_n() <= 1024
    assert all(a.batch_global_min_batch(n) >= 4 for n in (141, 256, 512, 1024))
    st = _capi.FnnBatchStats()
    assert _capi.FnnBatchStats.n_global.offset == _capi.FnnBatchStats.t_total_s.offset + 8 and st.n_global == 0


def test_existing_driver_still_binds():
    """The CPU driver of the LDS route exports neither of the new functions and binds as before."""
    b = bc.emu_batch_api()
    assert not hasattr(b, "batch_global_max_n") and b.batch_lds_max_n() >= 128


@pytest.mark.parametrize("n", bg.FORCED_SIZES)
def test_parity_on_the_forced_route(a, n, monkeypatch):
    bg.check_forced_parity(a, n, monkeypatch)


@pytest.mark.parametrize("threads", [256, 1024])
def test_thread_counts(a, threads, monkeypatch):
    bg.check_threads(a, threads, monkeypatch)


def test_default_route(a, monkeypatch):
    bg.check_default_route(a, monkeypatch)


def test_below_the_minimum_batch_needs_the_engine(a, monkeypatch):
    monkeypatch.delenv("FNN_BATCH_ROUTE", raising=False)
    with pytest.raises(_capi.FnnError) as ei:   # (3 problems of 141 taxa stay on the engine loop, which this driver lacks)
        bc.run(a, np.zeros((3, 141, 141)))
    assert ei.value.code == -1


def test_engine_override(a, monkeypatch):
    monkeypatch.setenv("FNN_BATCH_ROUTE", "engine")
    with pytest.raises(_capi.FnnError) as ei:
        bc.run(a, np.zeros((8, 141, 141)))
    assert ei.value.code == -1


def test_cap(a, monkeypatch):
    bg.check_cap(a, monkeypatch)


def test_above_the_cap_needs_the_engine(a, monkeypatch):
    monkeypatch.delenv("FNN_BATCH_ROUTE", raising=False)
    D = bg.above_cap_batch(a)
    for route in (None, "global"):
        if route:
            monkeypatch.setenv("FNN_BATCH_ROUTE", route)
        with pytest.raises(_capi.FnnError) as ei:
            bc.run(a, D)
        assert ei.value.code == -1


def test_more_workgroups_than_fit(a, monkeypatch):
    bg.check_many(a, monkeypatch)


@pytest.mark.parametrize("n", [9, 141])
def test_padding_is_never_read_and_nothing_written(a, n, monkeypatch):
    bg.check_padding(a, n, monkeypatch)


@pytest.mark.parametrize("n", [9, 141])
def test_in_place_entry_twice(a, n, monkeypatch):
    """The device entry's route: each matrix is copied, through ld and stride, into a working copy.  Twice on one buffer: the
    buffer is unchanged and the results are equal (a kernel that updated the caller's matrix would fail the second run)."""
    monkeypatch.setenv("FNN_BATCH_ROUTE", "global")
    D, refs = bc.class_batch(n)
    buf, ld, stride = bg.padded(D)
    before = buf.tobytes()
    r1 = _capi.run_batch(a, buf.ctypes.data, n, ld, stride, D.shape[0], events=True, validate=True, on_device=True)
    r2 = _capi.run_batch(a, buf.ctypes.data, n, ld, stride, D.shape[0], events=True, validate=True, on_device=True)
    assert buf.tobytes() == before
    assert (r1[0] == r2[0]).all() and r1[1].tobytes() == r2[1].tobytes() and (r1[2] == r2[2]).all()
    bc.assert_matches_oracle(r1[0], r1[1], r1[2], refs, ("in place", n))
    assert r1[3].n_global == D.shape[0] and r1[3].t_upload_s == 0


def test_validation(a, monkeypatch):
    bg.check_validation(a, monkeypatch)


def test_asymmetric_input_as_in_the_lds_route(a, monkeypatch):
    bg.check_asymmetric_like_lds(a, bc.emu_batch_api(), monkeypatch)


def test_standalone_program_under_asan_ubsan(a, tmp_path):
    """tests/emu/fnn_batch_global_emu_main.cpp with -fsanitize=address,undefined, as a program of its own (no sanitizer runtime
    is loaded into the interpreter): its generated list, and the parity cases for n <= 65 and 141 with the oracle's orders."""
    exe = os.path.join(bc.EMU_DIR, "build", "fnn_batch_global_emu_main_asan")
    srcs = [os.path.join(bc.EMU_DIR, "fnn_batch_global_emu_main.cpp")] + bg.EMU_SRCS
    if bc.newer(exe, srcs):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g", "-O1", "-o", exe, srcs[0], srcs[1]])
    sizes = [n for n in bg.FORCED_SIZES if n <= 65] + [141]
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        f.write(np.int32(len(sizes)).tobytes())
        for n in sizes:
            D, refs = bc.class_batch(n)
            f.write(np.array([n, D.shape[0]], dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(D).tobytes())
            f.write(np.stack([o for o, _ in refs]).astype(np.int32).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("FNN_BATCH_ROUTE", None)   # (the program sets the route itself)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.startswith("ok: ")

"""The batched small-problem path (fnn_small.h) on the CPU: the per-thread phase bodies run for
tid = 0 ... nthreads-1, phase by phase, by tests/emu/fnn_batch_emu.cpp under the product's own host logic, against the
oracle event by event; and the stand-alone AddressSanitizer / UBSan program over the same driver."""
import os
import subprocess

import numpy as np
import pytest

import batch_common as bc
from fastneighbornet_amd import _capi


@pytest.fixture(scope="module")
def a():
    return bc.emu_batch_api()


def test_lds_max_n(a):
    assert a.batch_lds_max_n() >= 128


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


def test_above_the_lds_limit_needs_the_engine(a):
    n = a.batch_lds_max_n() + 1
    with pytest.raises(_capi.FnnError) as ei:   # (the CPU driver has no one-problem engine; the product falls back: test_batch.py)
        bc.run(a, np.zeros((1, n, n)))
    assert ei.value.code == -1


def test_in_place_entry(a):
    """The device entry's route (matrices read in place through ld and stride; odd n: element loads, even n: 16-byte loads)."""
    for n in (33, 64):
        D, refs = bc.class_batch(n)
        orders, ev, nev, _ = bc.run(a, D, events=True, on_device=True)
        bc.assert_matches_oracle(orders, ev, nev, refs, ("in place", n))


def test_cross_check_with_the_engine_emulation(a, emu_api):
    """n = 64, B = 8: the batch's events are the events of the one-problem engine (its CPU emulation here)."""
    D, _ = bc.dec4_batch(64, 8, seed0=900)
    orders, ev, nev, _ = bc.run(a, D, events=True)
    for b in range(8):
        with _capi.Handle(emu_api, 64, record_events=True) as h:
            h.set_matrix(D[b])
            o, _ = h.run()
            bc.assert_same_events(ev[b], int(nev[b]), h.events(), b)
        assert (o == orders[b]).all()


def test_batch_layout_of_numpy_arrays():
    from fastneighbornet_amd.canonical import batch_layout
    big = np.zeros((4, 10, 12))
    v = big[:, :8, :8]
    arr, ld, stride = batch_layout(v)
    assert arr is v and ld == 12 and stride == 120
    arr, ld, stride = batch_layout(big[:, :8, :8].transpose(0, 2, 1))       # column-major problems: copied
    assert arr.flags.c_contiguous and ld == 8 and stride == 64
    arr, ld, stride = batch_layout(np.zeros((3, 8, 8), dtype=np.float32))  # another type: converted
    assert arr.dtype == np.float64 and ld == 8 and stride == 64


def test_product_fails_loudly_without_device():
    """No CPU fallback: without a HIP device the batch call fails with FNN_EHIP (identities need no device)."""
    import fastneighbornet_amd as fa
    api = fa.api()
    assert api.batch_lds_max_n() >= 128
    assert (fa.canonical_order_batch(np.zeros((2, 3, 3))) == np.arange(4)).all()
    if api.device_count() < 1:
        with pytest.raises(_capi.FnnError) as ei:
            fa.canonical_order_batch(np.zeros((2, 8, 8)))
        assert ei.value.code == -3


def test_standalone_program_under_asan_ubsan(a, tmp_path):
    """tests/emu/fnn_batch_emu_main.cpp with -fsanitize=address,undefined, as a program of its own (no sanitizer runtime is
    loaded into the interpreter): its generated list, and the parity cases for n <= 65 and lds_max_n with the oracle's orders."""
    exe = os.path.join(bc.EMU_DIR, "build", "fnn_batch_emu_main_asan")
    srcs = [os.path.join(bc.EMU_DIR, "fnn_batch_emu_main.cpp")] + bc.EMU_SRCS
    if bc.newer(exe, srcs):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g", "-O1", "-o", exe, srcs[0], srcs[1]])
    sizes = [n for n in bc.SMALL_SIZES if n <= 65] + [a.batch_lds_max_n()]
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        f.write(np.int32(len(sizes)).tobytes())
        for n in sizes:
            D, refs = bc.class_batch(n)
            f.write(np.array([n, D.shape[0]], dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(D).tobytes())
            f.write(np.stack([o for o, _ in refs]).astype(np.int32).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.startswith("ok: ")

"""The ragged batch calls (problems of different sizes in one call; fnn_small.h, fnn_small_splits.h) on
the CPU: tests/emu/fnn_ragged_emu.cpp runs the per-thread phase bodies phase by phase under the product's own host logic
(size classes, descriptors, chunking, collection), against the oracle per problem and against the emulated same-size calls;
and the stand-alone AddressSanitizer / UBSan program over the same driver."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import batch_common as bc
import ragged_common as rc
import splits_batch_common as sc
from fastneighbornet_amd import _capi


@pytest.fixture(scope="module")
def a():
    return rc.emu_api()


@pytest.fixture(scope="module")
def same_size():
    return bc.emu_batch_api(), sc.emu_api()


@pytest.fixture(autouse=True)
def kernel_route(monkeypatch):
    """The weight cases are for the kernel, also below the batch from which the call takes it by default."""
    monkeypatch.setenv("FNN_SW_BATCH_ROUTE", "kernel")


@pytest.fixture(scope="module", params=["host", "in_place"])
def drv(a, request):
    return rc.Driver(a, on_device=request.param == "in_place")


def same_calls(same_size):
    ob, sb = same_size
    return (lambda D: bc.run(ob, D, events=True)[:3]), (lambda D, o: sc.run(sb, np.ascontiguousarray(D), np.ascontiguousarray(o))[0])


def test_mixed_sizes_in_one_call(drv, a):
    rc.check_mixed(drv, a.batch_lds_max_n())


def test_outputs_follow_the_callers_numbering(drv, a):
    rc.check_numbering(drv, a.batch_lds_max_n())


def test_equal_sizes_give_the_same_size_calls_bytes(drv, same_size):
    rc.check_equal_sizes(drv, *same_calls(same_size))


def test_chunking(drv, monkeypatch):
    rc.check_chunking(drv, monkeypatch)


def test_validation(drv):
    rc.check_validation(drv)


def test_above_the_lds_limit_needs_the_same_size_entry(drv, a):
    n = a.batch_lds_max_n() + 1
    with pytest.raises(_capi.FnnError) as ei:   # (the CPU driver has none; the product hands the group over: test_ragged.py)
        drv.orders(rc.Layout([np.zeros((8, 8)), np.zeros((n, n))]))
    assert ei.value.code == -1


def test_weights_of_the_mixed_batch(drv, a, same_size):
    pytest.importorskip("scipy")
    rc.check_weights(drv, a.split_weights_batch_max_n(), same_calls(same_size)[1])


def test_weight_arguments(drv):
    mats, refs = rc.mixed((5, 9, 2, 12), seed=None)
    L, orders = rc.Layout(mats), [r[0] for r in refs]
    L.ns[2] = 1                                   # n < 2
    with pytest.raises(_capi.FnnError) as ei:
        drv.weights(L, [orders[0], orders[1], np.arange(2, dtype=np.int32), orders[3]], fill=sc.SENTINEL)
    assert ei.value.code == -1 and "problem 2" in str(ei.value) and (ei.value.weights == sc.SENTINEL).all()
    L = rc.Layout(mats)
    twice = orders[3].copy()
    twice[4] = twice[5]                           # not a permutation
    with pytest.raises(_capi.FnnError) as ei:
        drv.weights(L, orders[:3] + [twice])
    assert ei.value.code == -1 and "problem 3" in str(ei.value)
    bad = [m.copy() for m in mats]
    bad[3][2, 7] = bad[3][7, 2] = np.inf          # a non-finite distance: found in the kernel, named in the caller's numbering
    bad[1][0, 4] = bad[1][4, 0] = np.nan
    with pytest.raises(_capi.FnnError) as ei:
        drv.weights(rc.Layout(bad), orders, fill=sc.SENTINEL)
    assert ei.value.code == -1 and "problem 1:" in str(ei.value) and (ei.value.weights == sc.SENTINEL).all()
    w, sw, st = drv.weights(rc.Layout([]), [])    # batch == 0 is FNN_OK
    assert w == [] and st.n_problems == 0


def test_give_up_in_the_kernel(drv, a, monkeypatch):
    """FNN_SW_BATCH_CAP=8: a problem whose free set outgrows 8 splits gives up in its workgroup.  The driver has no
    one-problem solver behind it and reports the problem as the same-size driver does; the product falls back (test_ragged.py)."""
    D, so = sc.synth_batch(12, 6)
    mats = [D[b] for b in range(6)] + [rc.problem(5, 1)[0]]
    orders = [so[b] for b in range(6)] + [rc.problem(5, 1)[1][0]]
    monkeypatch.setenv("FNN_SW_BATCH_CAP", "8")
    with pytest.raises(_capi.FnnError) as ei:
        drv.weights(rc.Layout(mats), orders, fill=sc.SENTINEL)
    monkeypatch.delenv("FNN_SW_BATCH_CAP")
    assert ei.value.code == -6 and (ei.value.weights == sc.SENTINEL).all()
    g = np.zeros(7, dtype=np.int32)
    assert a.split_weights_ragged_giveups(g.ctypes.data_as(C.POINTER(C.c_int32)), 7) == 7
    assert (g[:6] == sc.GIVEUP_CAPACITY).any() and set(g.tolist()) <= {0, sc.GIVEUP_CAPACITY} and g[6] == 0
    first = int(np.nonzero(g)[0][0])
    assert f"problem {first}:" in str(ei.value)


def test_safety_net_in_one_mixed_call(drv, a, same_size, monkeypatch):
    pytest.importorskip("scipy")
    rc.check_safety_net(drv, a, sc.emu_solver(same_size[1]), None, monkeypatch)


def test_size_classes_keep_block_size_and_residency():
    """The classes as the launches see them, through the driver's stats: a call of 64- and 65-taxon problems and one of 96- and
    97-taxon problems take two launches each (a class never straddles a block-size edge), 16 with 140 likewise (a small
    problem is not launched under the reservation of the largest), 12 with 16 one."""
    a = rc.emu_api()
    drv = rc.Driver(a)
    for sizes, launches in (((64, 65), 2), ((96, 97), 2), ((16, a.batch_lds_max_n()), 2), ((12, 16), 1), ((128, a.batch_lds_max_n()), 1)):
        mats, _ = rc.mixed(sizes)
        _, _, _, st = drv.orders(rc.Layout(mats))
        assert st.chunks == launches, (sizes, st.chunks)
        assert st.block_threads == (256 if max(sizes) <= 64 else 512 if max(sizes) <= 96 else 1024)


def test_python_layout_of_separate_arrays():
    """canonical_order_ragged's view of a list of arrays: used where they lie, copied only when they must be."""
    from fastneighbornet_amd.canonical import ragged_layout
    big = np.zeros((10, 12))
    mats = [np.ones((5, 5)), big[:8, :8], np.zeros((6, 6), dtype=np.float32), np.asfortranarray(np.arange(16.0).reshape(4, 4))]
    base, offsets, ns, lds, on_device, device, keep = ragged_layout(mats)
    assert not on_device and device is None and ns.tolist() == [5, 8, 6, 4] and lds.tolist() == [5, 12, 6, 4]
    assert keep[0] is mats[0] and keep[1] is mats[1] and keep[2] is not mats[2] and keep[3].flags.c_contiguous
    assert [base + 8 * int(o) for o in offsets] == [k.ctypes.data for k in keep] and offsets.min() == 0


def test_product_fails_loudly_without_device():
    """No CPU fallback: without a HIP device the ragged calls fail with FNN_EHIP (identities need no device)."""
    import fastneighbornet_amd as fa
    got = fa.canonical_order_ragged([np.zeros((3, 3)), np.zeros((1, 1)), np.zeros((2, 2))])
    assert [g.tolist() for g in got] == [[0, 1, 2, 3], [0, 1], [0, 1, 2]]
    if fa.api().device_count() < 1:
        with pytest.raises(_capi.FnnError) as ei:
            fa.canonical_order_ragged([np.zeros((8, 8)), np.zeros((3, 3))])
        assert ei.value.code == -3
        with pytest.raises(_capi.FnnError) as ei:
            fa.split_weights_ragged([np.zeros((4, 4))], [np.arange(5)])
        assert ei.value.code == -3


def test_standalone_program_under_asan_ubsan(a, tmp_path):
    """tests/emu/fnn_ragged_emu_main.cpp with -fsanitize=address,undefined, as a program of its own (no sanitizer runtime is
    loaded into the interpreter): the mixed batch for n <= 65 and lds_max_n in one ragged call per entry, every matrix in a heap
    block of exactly its size, with the oracle's orders; then the weights of those orders."""
    exe = os.path.join(bc.EMU_DIR, "build", "fnn_ragged_emu_main_asan")
    srcs = [os.path.join(bc.EMU_DIR, "fnn_ragged_emu_main.cpp")] + rc.EMU_SRCS
    if bc.newer(exe, srcs):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g", "-O1", "-o", exe, srcs[0], srcs[1]])
    mats, refs = rc.mixed(tuple(n for n in rc.mixed_sizes(a.batch_lds_max_n()) if n <= 65 or n == a.batch_lds_max_n()))
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        f.write(np.int32(len(mats)).tobytes())
        for D, (o, _) in zip(mats, refs):
            f.write(np.int32(D.shape[0]).tobytes())
            f.write(np.ascontiguousarray(D).tobytes())
            f.write(np.asarray(o, dtype=np.int32).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.startswith("ok: ")

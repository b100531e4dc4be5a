"""The split-support stage (fnn_support.h) on the CPU: the per-thread steps of every kernel of the
sequence run for every thread of every workgroup by tests/emu/fnn_support_emu.cpp under the product's own host logic, bytewise
against the plain-Python reference of tests/support_common.py; the argument checks and fnn_split_keys also against the
product library (they need no device); and the stand-alone AddressSanitizer / UBSan program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import support_common as sc
from fastneighbornet_amd import _capi


@pytest.fixture(scope="module")
def a():
    return sc.emu_support_api()


@pytest.fixture(scope="module", params=["driver", "product"])
def either(request):
    if request.param == "driver":
        return sc.emu_support_api()
    import fastneighbornet_amd as fa
    return fa.api()


@pytest.mark.parametrize("n,B", sc.WORD_EDGES, ids=[f"n{n}-B{B}" for n, B in sc.WORD_EDGES])
def test_word_edges(a, n, B):
    sc.check_word_edge(a, n, B)


def test_both_sides_of_the_fold(a):
    sc.check_fold(a)


def test_order_of_the_sum(a):
    sc.check_sum_order(a)


@pytest.mark.parametrize("lead", sc.LEADS)
def test_lead(a, lead):
    sc.check_lead(a, lead)


def test_threshold(a):
    sc.check_threshold(a)


@pytest.mark.parametrize("in_place", [False, True])
def test_capacity(a, in_place):
    sc.check_capacity(a, in_place)


@pytest.mark.parametrize("in_place", [False, True])
def test_chunking_and_carry(a, in_place):
    sc.check_chunking(a, in_place)


def test_routes(a):
    sc.check_routes(a)


def test_sparse_keys_do_not_collide(a):
    sc.check_sparse_keys(a)


@pytest.mark.parametrize("n,B,chunk", [(140, 17, None), (65, 17, 5), (1024, 3, None), (sc.LEAD_N, 5, 2)])
def test_independent_of_the_order_of_workgroups(a, n, B, chunk):
    """Every launch with its workgroups from the last to the first: other slots of the hash table, other places inside the
    segments, the same bytes."""
    orders, W = sc.random_case(n, B, 1000 + n) if B != 5 else sc.lead_case()
    ref = sc.random_ref(n, B, 1000 + n) if B != 5 else sc.ref_arrays(sc.ref_table(orders, W, 1e-6, 1), n)
    try:
        for rev in (0, 1):
            a.set_reverse(rev)
            st = sc.check_against(a, orders, W, ref, lead=1 if B == 5 else 0, route="kernel", chunk=chunk)
            assert st.route == 0
    finally:
        a.set_reverse(0)


def test_arguments_without_a_device(either):
    sc.check_arguments(either)


def test_split_keys(either):
    sc.check_keys(either)


def test_python_wrappers_without_a_device():
    import fastneighbornet_amd as fa
    order = sc.order_row([3, 1, 2, 5, 4])
    keys = fa.split_keys(order, [0, 4, 9])
    assert keys.dtype == np.uint64 and keys.shape == (3, 1)
    pr = sc.pairs(5)
    assert [fa.key_taxa(k) for k in keys] == [sorted(t + 1 for t in range(5) if sc.ref_key(order.tolist(), 5, *pr[k]) >> t & 1) for k in (0, 4, 9)]
    assert fa.key_taxa(np.array([1 << 63, 5], dtype=np.uint64)) == [64, 65, 67]
    # below the crossover the table comes from the host route: no device is needed
    orders, W = sc.random_case(9, 5, 77)
    with sc.switches():
        table, st = fa.split_support(orders, W, lead=1)
    ref = sc.ref_arrays(sc.ref_table(orders, W, 1e-6, 1), 9)
    sc.assert_table(table, st["n_splits"], ref)
    assert st["method"] == "host" and (table["support"] == ref["count"] / 4.0).all()
    with pytest.raises(ValueError):
        fa.split_support(orders, W[:, :-1])
    if fa.api().device_count() < 1:   # no quiet fall-back: the kernel route without a device is an error
        with sc.switches(route="kernel"), pytest.raises(_capi.FnnError) as ei:
            fa.split_support(orders, W)
        assert ei.value.code == -3


def test_stats_struct_matches_header(tmp_path):
    """sizeof(fnn_support_stats) as the C compiler sees it against the ctypes mirror (tests/test_abi.py checks the symbols)."""
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fastnn.h"\nint main(void) { printf("%zu %zu %zu %d %d\\n", '
                   'sizeof(fnn_support_stats), offsetof(fnn_support_stats, table_slots), offsetof(fnn_support_stats, t_upload_s), '
                   '(int)FNN_SUPPORT_ROUTE_KERNEL, (int)FNN_SUPPORT_ROUTE_HOST); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(sc.ROOT, "include"), "-o", str(exe), str(src)])
    size, slots, upload, kernel, host = (int(x) for x in subprocess.check_output([str(exe)], text=True).split())
    assert size == C.sizeof(_capi.FnnSupportStats) == 3 * 8 + 4 * 4 + 8 + 3 * 8 + 4 * 8
    assert slots == _capi.FnnSupportStats.table_slots.offset and upload == _capi.FnnSupportStats.t_upload_s.offset
    assert _capi.SUPPORT_ROUTES[kernel] == "kernel" and _capi.SUPPORT_ROUTES[host] == "host"


def test_standalone_program_under_asan_ubsan():
    """tests/emu/fnn_support_emu_main.cpp with -fsanitize=address,undefined, as a program of its own (no sanitizer runtime is
    loaded into the interpreter): word edges, both entries, chunks, hash repeats and reversed workgroups on buffers of exactly
    the declared sizes, against a plain loop over the definition."""
    exe = os.path.join(sc.EMU_DIR, "build", "fnn_support_emu_main_asan")
    srcs = [os.path.join(sc.EMU_DIR, "fnn_support_emu_main.cpp")] + sc.EMU_SRCS
    if sc.newer(exe, srcs):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g", "-O1",
                               "-o", exe, srcs[0], srcs[1]])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for k in sc.SWITCHES:
        env.pop(k, None)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.startswith("ok: ")

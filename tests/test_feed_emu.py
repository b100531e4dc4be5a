"""The engine's continuous feed (fnn_engine.h: agglomerate_feed) on the CPU: tests/emu/fnn_feed_emu_main.cpp is a program of its
own whose backend is the emulation's plus a mailbox in which a record becomes visible `lag` launches after it was filed.  For
every input here it runs depth in {1, 2, 16, 1024} x lag in {0, 1, depth - 1} and must get the oracle's order every time,
through the feed, with at most `depth` launch sequences behind the last event; with --unit it checks that a torn record, one
of the previous generation and a repeated sequence number are passed over.  Built plainly and with
-fsanitize=address,undefined, and run directly: nothing is loaded into the interpreter."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "fastneighbornet_amd", "csrc")
SRC = os.path.join(EMU_DIR, "fnn_feed_emu_main.cpp")
DEPS = [SRC, os.path.join(EMU_DIR, "fnn_emu.cpp"), os.path.join(CSRC, "fnn_engine.h"), os.path.join(CSRC, "fnn_core.h"),
        os.path.join(CSRC, "fnn_chain.h"), os.path.join(ROOT, "include", "fastnn.h")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
       "-fno-omit-frame-pointer", "-g", "-O1"]
BUILDS = [("fnn_feed_emu_main", ["-O2"]), ("fnn_feed_emu_main_asan", SAN)]
ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def build(name, flags):
    exe = os.path.join(EMU_DIR, "build", name)
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in DEPS):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas"] + flags + ["-o", exe, SRC])
    return exe


_FILES = {}


def input_file(oracle, tmp_path_factory, n, dist, seed):
    """Matrix and oracle order of one input, written once: int32 n, n * n doubles, n + 1 int32."""
    key = (n, dist, seed)
    if key not in _FILES:
        D = np.ascontiguousarray(inputs.make(n, dist, seed, oracle), dtype=np.float64)
        order = np.ascontiguousarray(oracle.run(D)[0], dtype=np.int32)
        assert order.shape == (n + 1,)
        path = str(tmp_path_factory.mktemp("feed") / f"{dist}_{n}_{seed}.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<i", n))
            f.write(D.tobytes())
            f.write(order.tobytes())
        _FILES[key] = path
    return _FILES[key]


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=dict(os.environ, **ENV), timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("name,flags", BUILDS)
def test_record_check(name, flags):
    assert run(build(name, flags), "--unit").startswith("ok: record check")


@pytest.mark.parametrize("name,flags", BUILDS)
@pytest.mark.parametrize("n,dist,seed", [(300, "uniform53", 2), (300, "dec4", 3), (300, "tree", 2),
                                         (601, "uniform53", 4), (601, "dec4", 5), (601, "tree", 3)])
def test_every_depth_and_lag_gives_the_oracle_order(oracle, tmp_path_factory, name, flags, n, dist, seed):
    out = run(build(name, flags), input_file(oracle, tmp_path_factory, n, dist, seed))
    m = re.match(r"ok: (\d+) runs, (\d+) stalled sequences, (\d+) window hits", out)
    assert m and int(m.group(1)) == 9, out[-1000:]
    assert int(m.group(3)) > 0, out[-1000:]  # (windows were on: the feed followed their schedule)


@pytest.mark.parametrize("name,flags", BUILDS)
def test_windows_that_give_out_early_stall_and_recover(oracle, tmp_path_factory, name, flags):
    """lookahead = 64 over 16 wanted pairs: the windows cannot serve their events for long, the sequences up to the host's next
    scheduled scan stall - about `depth` per episode - and the run still ends with the oracle's order."""
    out = run(build(name, flags), input_file(oracle, tmp_path_factory, 601, "uniform53", 4), 64, 16)
    m = re.match(r"ok: (\d+) runs, (\d+) stalled sequences, (\d+) window hits", out)
    assert m and int(m.group(1)) == 9, out[-1000:]
    assert int(m.group(2)) > 0 and int(m.group(3)) > 0, out[-1000:]


@pytest.mark.parametrize("name,flags", BUILDS)
@pytest.mark.parametrize("n", [4, 5, 8, 9, 33])
def test_runs_shorter_than_the_depth(oracle, tmp_path_factory, name, flags, n):
    """Fewer events than the feed may hold in flight, and the special finish."""
    for dist, seed in (("uniform53", 1), ("dec4", 2)):
        out = run(build(name, flags), input_file(oracle, tmp_path_factory, n, dist, seed))
        assert re.match(r"ok: 9 runs", out), out[-1000:]

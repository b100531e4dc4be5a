"""The engine's device-buffer table (fnn_engine.h: create / comm_set / destroy) on the CPU: tests/emu/fnn_engine_buffers_main.cpp
is a program of its own that instantiates the engine over a counting backend and checks, for n = 0, 3, 5, 9 and six
configurations, that nothing is live after destroy() - also when the k-th allocation fails, for every k.  It is built twice:
plainly, and with -fsanitize=address,undefined (run directly: nothing is loaded into the interpreter)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "fastneighbornet_amd", "csrc")
SRC = os.path.join(EMU_DIR, "fnn_engine_buffers_main.cpp")
DEPS = [SRC, os.path.join(CSRC, "fnn_engine.h"), os.path.join(CSRC, "fnn_core.h"), os.path.join(ROOT, "include", "fastnn.h")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
       "-fno-omit-frame-pointer", "-g", "-O1"]


def build(name, flags):
    exe = os.path.join(EMU_DIR, "build", name)
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in DEPS):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas"] + flags + ["-o", exe, SRC])
    return exe


@pytest.mark.parametrize("name,flags", [("fnn_engine_buffers_main", ["-O2"]), ("fnn_engine_buffers_main_asan", SAN)])
def test_buffers_balance_and_survive_failed_allocations(name, flags):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    exe = build(name, flags)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.match(r"ok: (\d+) runs", r.stdout)
    assert m and int(m.group(1)) >= 24 * 28, r.stdout[-1000:]
    # the allocation sequence: 24 configurations, every one with at least the 27 buffers a Canonical handle always has
    p = subprocess.run([exe, "--print"], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    heads = re.findall(r"^# .*: (\d+) allocations$", p.stdout, re.M)
    assert len(heads) == 24 and all(int(k) >= 27 for k in heads), p.stdout[:1000]

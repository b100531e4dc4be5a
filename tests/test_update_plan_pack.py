"""The packed update plan (fnn_core.h: UpdPlan) against plan_view, on the CPU: tests/emu/fnn_update_plan_main.cpp is a program
of its own that draws a few thousand well-formed plans - the four event kinds replayed by build_targets, and plans drawn field by
field over every nS / ntgt - and compares upd_plan_view(upd_plan_pack(st)) with plan_view(st) field by field.  It is built twice:
plainly, and with -fsanitize=address,undefined (run directly: nothing is loaded into the interpreter)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
SRC = os.path.join(EMU_DIR, "fnn_update_plan_main.cpp")
DEPS = [SRC, os.path.join(ROOT, "fastneighbornet_amd", "csrc", "fnn_core.h")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
       "-fno-omit-frame-pointer", "-g", "-O1"]


def build(name, flags):
    exe = os.path.join(EMU_DIR, "build", name)
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in DEPS):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas"] + flags + ["-o", exe, SRC])
    return exe


@pytest.mark.parametrize("name,flags", [("fnn_update_plan_main", ["-O2"]), ("fnn_update_plan_main_asan", SAN)])
def test_pack_then_view_equals_plan_view(name, flags):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([build(name, flags)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.match(r"ok: (\d+) plans \((\d+) replayed events", r.stdout)
    assert m, r.stdout[-1000:]
    assert int(m.group(1)) >= 3000 and int(m.group(2)) >= 2000

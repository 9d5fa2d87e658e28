"""The bounce levels' chunk rounds (option lv_round): the mapping
from a workgroup's n-th claim to a chunk, lv_round_chunk in
raytracing_rb_amd/csrc/rtx_sched.h, hands every static chunk to exactly one
claim of one workgroup, none past the static part, in increasing order.

tools/sched_check.cpp includes the header the kernels include and enumerates
chunks x workgroups x waves x round sizes x lv_static (the lists are in its
head comment).  The GPU tests compare frames (test_gpu_chunk_rounds.py)."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tools", "sched_check.cpp")
CASES = 10 * 4 * 2 * 5 * 3


def _build(tmp_path_factory, name, flags):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp(name) / "sched_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, SRC], check=True, timeout=300)
    return exe


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    f = out.stdout.split()
    return out.returncode, dict(zip(f[0::2], map(int, f[1::2]))), out.stderr


def test_rounds_hand_out_every_static_chunk_once(tmp_path_factory):
    rc, r, err = _run(_build(tmp_path_factory, "sched", ["-O2"]))
    assert rc == 0 and r["errors"] == 0 and r["cases"] == CASES and r["chunks"] > 0, (rc, r, err)


def test_rounds_check_is_clean_under_sanitizers(tmp_path_factory):
    """The same stand-alone program with the address and undefined-behaviour
    sanitizers: no report, same counts."""
    rc, r, err = _run(_build(tmp_path_factory, "sched_san",
                             ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))
    assert rc == 0 and r["errors"] == 0 and r["cases"] == CASES and "runtime error" not in err, (rc, r, err)


def test_rounds_check_has_teeth(tmp_path):
    """With the round's stride off by one workgroup the check finds errors."""
    hdr = open(os.path.join(ROOT, "raytracing_rb_amd", "csrc", "rtx_sched.h")).read()
    assert "(k * G + b) * R" in hdr
    (tmp_path / "rtx_sched.h").write_text(hdr.replace("(k * G + b) * R", "(k * (G + 1) + b) * R"))
    src = open(SRC).read().replace('"../raytracing_rb_amd/csrc/rtx_sched.h"', '"rtx_sched.h"')
    (tmp_path / "sched_check.cpp").write_text(src)
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "chk")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, str(tmp_path / "sched_check.cpp")], check=True, timeout=300)
    rc, r, _ = _run(exe)
    assert rc == 1 and r["errors"] > 0, (rc, r)

"""csrc/vrt_frame_plan.h — what kind of frame a vrt_render call is, decided once — against the predicates it replaced:
tools/check_frame_plan.cpp built as a program of its own (AddressSanitizer + UBSan in the program, nothing loaded into this
process) and run over every combination of the facts."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "check_frame_plan.cpp")


def test_plan_frame_equals_the_predicates_it_replaced(tmp_path):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.fail(f"no C++ compiler ({cxx}): the plan's check program cannot be built")
    exe = tmp_path / "check_frame_plan"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-static-libasan", "-static-libubsan", "-o", str(exe), SRC]   # (the build line of the program's header)
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"check_frame_plan: ok \((\d+) frames compared, (\d+) refused\)", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) > 10000
    # every (mode, variant) pair vrt_render accepts was compared: primary and primary + shadow with the four variants, the path trace
    pairs = {(int(a), int(b)): int(n) for a, b, n in re.findall(r"mode (\d) variant (\d): (\d+)", r.stdout)}
    assert set(pairs) == {(m_, v) for m_ in (0, 1) for v in range(4)} | {(2, 0)}
    assert all(n > 0 for n in pairs.values())


def test_the_header_needs_no_hip():
    text = open(os.path.join(ROOT, "voxelraytracing_amd", "csrc", "vrt_frame_plan.h")).read()
    assert "hip" not in re.sub(r"//.*", "", text).lower()

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


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    """The check program built and run once: its standard output."""
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.fail(f"no C++ compiler ({cxx}): the plan's check program cannot be built")
    exe = tmp_path_factory.mktemp("plan") / "check_frame_plan"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-static-libasan", "-static-libubsan", "-o", str(exe), SRC]   # (the build line of the program's header)
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_plan_frame_equals_the_predicates_it_replaced(check_output):
    m = re.search(r"check_frame_plan: ok \((\d+) frames compared, (\d+) refused\)", check_output)
    assert m, check_output
    assert int(m.group(1)) > 10000
    # every (mode, variant) pair vrt_render accepts was compared: primary and primary + shadow with the four variants, the path trace
    pairs = {(int(a), int(b)): int(n) for a, b, n in re.findall(r"mode (\d) variant (\d): (\d+)", check_output)}
    assert set(pairs) == {(m_, v) for m_ in (0, 1) for v in range(4)} | {(2, 0)}
    assert all(n > 0 for n in pairs.values())


def test_plan_path_schedules_the_launches_the_loop_it_replaced_did(check_output):
    """plan_path + for_each_path_step against launch_path_frame's decisions and double loop as they stood before: the same launches in
    the same order with the same cursor sets, buffers and arguments, over every combination of the facts that can reach the function
    (7 spp x 6 bounce counts x 7 booleans x 3 accumulation states x 4 chain lengths x 3 pool depths x 1 or 2 frames in flight, less
    the unreachable half: 193 536 frames at the program's first run)."""
    m = re.search(r"check_path_plan: ok \((\d+) frames compared, (\d+) launches, (\d+) unreachable\)", check_output)
    assert m, check_output
    assert int(m.group(1)) >= 193536
    assert int(m.group(2)) > int(m.group(1))


def test_the_header_needs_no_hip():
    text = open(os.path.join(ROOT, "voxelraytracing_amd", "csrc", "vrt_frame_plan.h")).read()
    assert "hip" not in re.sub(r"//.*", "", text).lower()

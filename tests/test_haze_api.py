"""vrt_set_haze (include/vrt.h) without a GPU: the header declares the struct and the function and states the contract, the struct is
32 bytes as ctypes and the Rust crate have it, the library exports the function, a null context is refused, the haze kernels are a
pair of their own in every march build — which tests/kernel_families.py does not take for water or plain path kernels — and the
frame plan's check program holds a haze frame to the sun-lit frame's structure."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import pytest

from kernel_families import MARCH_BUILDS, families, path_kernel, water_kernel
from voxelraytracing_amd import _ffi, graphics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_the_struct_and_the_function():
    h = _read("include", "vrt.h")
    assert re.search(r"typedef\s+struct\s*\{\s*float\s+density;[^}]*float\s+albedo\[3\];[^}]*uint32_t\s+flags;[^}]*uint32_t\s+_reserved\[3\];[^}]*\}"
                     r"\s*vrt_haze\s*;", h)
    assert re.search(r"int\s+vrt_set_haze\s*\(\s*vrt_ctx\s*\*\s*ctx\s*,\s*const\s+vrt_haze\s*\*\s*opts\s*\)\s*;", h)
    # next to vrt_set_water_refraction, and the contract names what does not compose and what is out of scope
    assert h.index("vrt_set_water_refraction(vrt_ctx") < h.index("Haze for VRT_MODE_PATH") < h.index("vrt_set_camera_sampling(vrt_ctx")
    doc = h[h.index("Haze for VRT_MODE_PATH"):h.index("} vrt_haze;")]
    for word in ("VRT_ERR_STATE", "vrt_set_water_optics", "vrt_set_lamp_light", "vrt_set_camera_sampling", "vrt_last_error", "Build-defined, and defined exactly",
                 "rng_next_dir", "vlog", "1e-10f", "0.25f", "q > 0.5f", "height falloff", "anisotropic", "2^-20, 64", "VRT_ERR_INVALID_ARG",
                 "VRT_RENDER_ACCUMULATE", "secondary_rays"):
        assert word in doc, word
    assert [n for n in range(1, 7) if re.search(rf"\n \*   {n}  ", doc)] == [1, 2, 3, 4, 5, 6]   # numbered, as the neighbouring contracts are
    hh = _read("include", "vrt_host.h")
    assert re.search(r"int\s+vrth_haze_distance\s*\(", hh) and re.search(r"int\s+vrth_haze_exit\s*\(", hh)


def test_the_struct_is_32_bytes(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vrt.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(vrt_haze), offsetof(vrt_haze, density), '
                   'offsetof(vrt_haze, albedo), offsetof(vrt_haze, flags), offsetof(vrt_haze, _reserved)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["32", "0", "4", "16", "20"]
    assert C.sizeof(_ffi.Haze) == 32
    assert [(n, getattr(_ffi.Haze, n).offset) for n, _ in _ffi.Haze._fields_] == [("density", 0), ("albedo", 4), ("flags", 16), ("_reserved", 20)]


def test_the_library_exports_it():
    lib = _ffi.vrt()
    assert hasattr(lib, "vrt_set_haze")
    assert _ffi.VRT_SYMBOLS["vrt_set_haze"] == (C.c_int, [C.c_void_p, C.POINTER(_ffi.Haze)])
    assert hasattr(_ffi.host(), "vrth_haze_distance") and hasattr(_ffi.host(), "vrth_haze_exit")


def test_null_context_is_refused_without_a_device():
    lib = _ffi.vrt()
    o = _ffi.Haze(0.05, (C.c_float * 3)(0.9, 0.9, 0.9), 0, (C.c_uint32 * 3)(0, 0, 0))
    assert lib.vrt_set_haze(None, C.byref(o)) == _ffi.VRT_ERR_INVALID_ARG
    assert lib.vrt_set_haze(None, None) == _ffi.VRT_ERR_INVALID_ARG
    assert _ffi.host().vrth_haze_distance(None, 1, 1.0, None) == -1 and _ffi.host().vrth_haze_exit(None, None, 1.0, None) == -1


def test_python_binding():
    assert list(inspect.signature(graphics.Gpu.set_haze).parameters) == ["self", "density", "albedo"]


def test_rust_binding():
    rs = _read("bindings", "rust", "vrt-sys", "src", "lib.rs")
    assert re.search(r"pub struct vrt_haze \{\s*pub density: f32,\s*pub albedo: \[f32; 3\],\s*pub flags: u32,\s*pub _reserved: \[u32; 3\],\s*\}", rs)
    assert re.search(r"pub fn vrt_set_haze\(ctx: \*mut vrt_ctx, opts: \*const vrt_haze\) -> c_int;", rs)
    assert re.search(r"size_of::<vrt_haze>\(\) == 32", rs)


_HAZE = re.compile(r"^_ZN3vrt\d+path_haze_(primary|bounce)_kernelI(Li\dELb\dELb\dE)EEvNS_11FrameParamsENS_10HazeLaunchENS_9SunLaunchE$")


def test_the_library_holds_exactly_one_haze_pair_per_march_build_without_scratch():
    """Three marches x the root table in LDS where it applies x counting, as vrt_path.hip's with_march_build enumerates them: a
    dropped instantiation fails here, where the library is inspected, and not as a missing kernel on some route on the GPU.
    Code-object metadata: no scratch, nothing spilled."""
    regs = _ffi.kernel_registers()
    haze = {k: _HAZE.match(k) for k in regs if "haze" in k}
    assert len(haze) == 20 and all(haze.values()), sorted(k for k, m in haze.items() if not m)
    for template in ("primary", "bounce"):
        builds = sorted(m.group(2) for m in haze.values() if m.group(1) == template)
        assert builds == sorted(MARCH_BUILDS), (template, builds)
    bad = {k: regs[k] for k in haze if regs[k]["scratch_bytes"] or regs[k]["sgpr_spills"] or regs[k]["vgpr_spills"]}
    assert not bad, bad


def test_no_haze_symbol_is_taken_for_a_water_or_a_plain_path_kernel():
    regs = _ffi.kernel_registers()
    haze = [k for k in regs if "haze" in k]
    assert len(haze) == 20
    for k in haze:
        assert path_kernel(k) is None and water_kernel(k) is None and families(k) == frozenset(), k
    # ... and the families from before count what they counted
    assert sum(1 for k in regs if water_kernel(k) is not None) == 20


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    """tools/check_frame_plan.cpp built and run as tests/test_frame_plan.py does: a program of its own with AddressSanitizer and
    UBSan linked in, nothing loaded into this process."""
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.fail(f"no C++ compiler ({cxx}): the plan's check program cannot be built")
    exe = tmp_path_factory.mktemp("plan") / "check_frame_plan"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-static-libasan", "-static-libubsan", "-o", str(exe), os.path.join(ROOT, "tools", "check_frame_plan.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_a_haze_frame_is_planned_as_a_sun_lit_one(check_output):
    m = re.search(r"check_haze_plan: ok \((\d+) haze frames, (\d+) launches\)", check_output)
    assert m, check_output
    assert int(m.group(1)) >= 100000 and int(m.group(2)) > int(m.group(1))
    # the checks from before still run in front of it, with haze = false
    assert check_output.index("check_water_plan: ok") < check_output.index("check_haze_plan: ok")
    plan = _read("voxelraytracing_amd", "csrc", "vrt_frame_plan.h")
    assert re.search(r"kStepWaterPrimary, kStepWaterBounce, kStepHazePrimary, kStepHazeBounce \};", plan)

"""vrt_set_lamp_light, vrt_get_lamp_info and vrt_read_lamps (include/vrt.h) without a GPU: the header declares the structs and the
functions, the structs have the sizes a C compiler gives them, libvrt.so exports the functions, and every binding — _ffi,
graphics.Gpu, the Rust vrt-sys crate — carries them; a null context is refused before anything touches a device; the lamp-lit
kernels are kernels of their own under names the other families' counts do not see, none spills, and a lamp-lit frame's plan is
the steps the contract asks for, with and without the sun.  What needs a context is in tests/test_gpu_lamp.py."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from voxelraytracing_amd import _ffi, graphics
from kernel_families import in_family

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_the_structs_and_the_functions():
    h = _read("include", "vrt.h")
    assert re.search(r"typedef\s+struct\s*\{\s*float\s+strength;[^}]*float\s+max_geometry;[^}]*uint32_t\s+flags;[^}]*uint32_t\s+_reserved;[^}]*\}\s*vrt_lamp_light\s*;", h)
    assert re.search(r"typedef\s+struct\s*\{\s*uint16_t\s+pos\[3\];\s*uint16_t\s+voxel;\s*uint32_t\s+face;\s*uint32_t\s+_reserved;\s*\}\s*vrt_lamp\s*;", h)
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+listed;\s*uint32_t\s+cap;\s*uint64_t\s+faces;\s*uint32_t\s+builds;\s*float\s+last_build_ms;\s*\}\s*vrt_lamp_info\s*;", h)
    assert re.search(r"int\s+vrt_set_lamp_light\s*\(\s*vrt_ctx\s*\*\s*ctx\s*,\s*const\s+vrt_lamp_light\s*\*\s*opts\s*\)\s*;", h)
    assert re.search(r"int\s+vrt_get_lamp_info\s*\(\s*vrt_ctx\s*\*\s*ctx\s*,\s*vrt_lamp_info\s*\*\s*out\s*\)\s*;", h)
    assert re.search(r"int\s+vrt_read_lamps\s*\(\s*vrt_ctx\s*\*\s*ctx\s*,\s*vrt_lamp\s*\*\s*out\s*,\s*uint32_t\s+cap\s*,\s*uint32_t\s*\*\s*n\s*\)\s*;", h)


def test_the_structs_sizes_by_a_c_compile(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vrt.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(vrt_lamp_light), offsetof(vrt_lamp_light, strength), '
                   'offsetof(vrt_lamp_light, max_geometry), offsetof(vrt_lamp_light, flags), offsetof(vrt_lamp_light, _reserved));\n'
                   'printf("%zu %zu %zu %zu\\n", sizeof(vrt_lamp), offsetof(vrt_lamp, voxel), offsetof(vrt_lamp, face), offsetof(vrt_lamp, _reserved));\n'
                   'printf("%zu %zu %zu %zu %zu\\n", sizeof(vrt_lamp_info), offsetof(vrt_lamp_info, cap), offsetof(vrt_lamp_info, faces), '
                   'offsetof(vrt_lamp_info, builds), offsetof(vrt_lamp_info, last_build_ms)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).splitlines()
    assert out[0].split() == ["16", "0", "4", "8", "12"]
    assert out[1].split() == ["16", "6", "8", "12"]
    assert out[2].split() == ["24", "4", "8", "16", "20"]
    assert C.sizeof(_ffi.LampLight) == 16 and C.sizeof(_ffi.Lamp) == 16 and C.sizeof(_ffi.LampInfo) == 24 and _ffi.LAMP_DTYPE.itemsize == 16
    assert [(n, getattr(_ffi.LampLight, n).offset) for n, _ in _ffi.LampLight._fields_] == [("strength", 0), ("max_geometry", 4), ("flags", 8), ("_reserved", 12)]
    assert [(n, getattr(_ffi.Lamp, n).offset) for n, _ in _ffi.Lamp._fields_] == [("pos", 0), ("voxel", 6), ("face", 8), ("_reserved", 12)]
    assert [(n, getattr(_ffi.LampInfo, n).offset) for n, _ in _ffi.LampInfo._fields_] == [("listed", 0), ("cap", 4), ("faces", 8), ("builds", 16), ("last_build_ms", 20)]
    assert [_ffi.LAMP_DTYPE.fields[n][1] for n in ("pos", "voxel", "face", "_reserved")] == [0, 6, 8, 12]


def test_the_library_exports_them():
    lib = _ffi.vrt()
    for name in ("vrt_set_lamp_light", "vrt_get_lamp_info", "vrt_read_lamps"):
        assert hasattr(lib, name)
    assert _ffi.VRT_SYMBOLS["vrt_set_lamp_light"] == (C.c_int, [C.c_void_p, C.POINTER(_ffi.LampLight)])
    assert _ffi.VRT_SYMBOLS["vrt_get_lamp_info"] == (C.c_int, [C.c_void_p, C.POINTER(_ffi.LampInfo)])
    assert _ffi.VRT_SYMBOLS["vrt_read_lamps"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)])


def test_null_context_is_refused_without_a_device():
    lib = _ffi.vrt()
    o = _ffi.LampLight(1.0, 0.0, 0, 0)
    assert lib.vrt_set_lamp_light(None, C.byref(o)) == _ffi.VRT_ERR_INVALID_ARG
    assert lib.vrt_set_lamp_light(None, None) == _ffi.VRT_ERR_INVALID_ARG
    info, n = _ffi.LampInfo(), C.c_uint32(0)
    assert lib.vrt_get_lamp_info(None, C.byref(info)) == _ffi.VRT_ERR_INVALID_ARG
    assert lib.vrt_read_lamps(None, None, 0, C.byref(n)) == _ffi.VRT_ERR_INVALID_ARG


def test_python_binding():
    p = inspect.signature(graphics.Gpu.set_lamp_light).parameters
    assert list(p) == ["self", "strength", "max_geometry"] and p["max_geometry"].default == 0.0
    assert list(inspect.signature(graphics.Gpu.lamp_info).parameters) == ["self"]
    assert list(inspect.signature(graphics.Gpu.read_lamps).parameters) == ["self"]


def test_rust_binding():
    rs = _read("bindings", "rust", "vrt-sys", "src", "lib.rs")
    assert re.search(r"pub struct vrt_lamp_light \{\s*pub strength: f32,\s*pub max_geometry: f32,\s*pub flags: u32,\s*pub _reserved: u32,\s*\}", rs)
    assert re.search(r"pub struct vrt_lamp \{\s*pub pos: \[u16; 3\],\s*pub voxel: u16,\s*pub face: u32,\s*pub _reserved: u32,\s*\}", rs)
    assert re.search(r"pub struct vrt_lamp_info \{\s*pub listed: u32,\s*pub cap: u32,\s*pub faces: u64,\s*pub builds: u32,\s*pub last_build_ms: f32,\s*\}", rs)
    assert re.search(r"pub fn vrt_set_lamp_light\(ctx: \*mut vrt_ctx, opts: \*const vrt_lamp_light\) -> c_int;", rs)
    assert re.search(r"pub fn vrt_get_lamp_info\(ctx: \*mut vrt_ctx, out: \*mut vrt_lamp_info\) -> c_int;", rs)
    assert re.search(r"pub fn vrt_read_lamps\(ctx: \*mut vrt_ctx, out: \*mut vrt_lamp, cap: u32, n: \*mut u32\) -> c_int;", rs)
    assert re.search(r"size_of::<vrt_lamp_light>\(\) == 16", rs) and re.search(r"size_of::<vrt_lamp>\(\) == 16", rs)
    assert re.search(r"size_of::<vrt_lamp_info>\(\) == 24", rs)


def test_the_lamp_kernels_are_built_apart_from_the_others():
    """One pair of trace kernels — the primary one with and without camera sampling, ten march forms each; the bounce one, ten —
    which carries the sun term under a scalar branch and reads coat and pass-through from the launch; the lamp launch in its ten
    march forms; the three kernels of the list build.  They belong to none of the families the other kernels are counted by
    (tests/kernel_families.py), so those counts are what the existing tests say; nothing spills."""
    regs = _ffi.kernel_registers()
    lamp = {k: v for k, v in regs.items() if "lamp" in k}
    assert sum(1 for k in lamp if re.search(r"path_lamp_primary_kernelI.*Lb0EEEvNS_11FrameParamsENS_10LensLaunchENS_9SunLaunchENS_10LampLaunchE$", k)) == 10
    assert sum(1 for k in lamp if re.search(r"path_lamp_primary_kernelI.*Lb1EEEvNS_11FrameParamsENS_10LensLaunchENS_9SunLaunchENS_10LampLaunchE$", k)) == 10
    assert sum(1 for k in lamp if re.search(r"path_lamp_bounce_kernelI.*FrameParamsENS_9SunLaunchENS_10LampLaunchE$", k)) == 10
    assert sum(1 for k in lamp if re.search(r"path_lamp_rays_kernelI.*FrameParamsENS_10LampLaunchE$", k)) == 10
    assert sum(1 for k in lamp if re.search(r"lamp_(count|scan|write)_kernel", k)) == 3
    assert len(lamp) == 43
    bad = {k: v for k, v in lamp.items() if v["scratch_bytes"] or v["sgpr_spills"] or v["vgpr_spills"]}
    assert not bad, bad
    for sub in ("sunlit", "path_sun_", "lens", "translucent", "polished", "emissive"):
        assert not [k for k in lamp if in_family(k, sub) or sub in k], sub
    # the other families are what the existing tests say they are
    assert sum(1 for k in regs if in_family(k, "sunlit") or "path_sun_" in k) == 32
    assert sum(1 for k in regs if in_family(k, "translucent")) == 24 and sum(1 for k in regs if in_family(k, "polished")) == 24
    assert sum(1 for k in regs if in_family(k, "lens")) == 21 and sum(1 for k in regs if in_family(k, "emissive")) == 3


PLAN_PROGRAM = r"""
#include <cstdio>
#include "vrt_frame_plan.h"
int main(int argc, char **argv) {
    vrt::PathFacts F;
    F.spp = 2; F.bounces = 3; F.has_grid = true; F.has_cells = true; F.march_direct = true; F.emissive = true;
    F.lamp = true; F.sun = argc > 1;
    const vrt::PathPlan p = vrt::plan_path(F);
    std::printf("lamp %d sun %d cells %d samples %u emit %d\n", p.lamp, p.sun, p.cells, p.samples, p.emit);
    vrt::for_each_path_step(p, [&](const vrt::PathStep &s) { std::printf("%u:%u:%u:%d ", (unsigned)s.kind, s.sample, s.launch, vrt::traces_paths(s.kind)); });
    std::printf("\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("lamp_plan")
    (d / "plan.cpp").write_text(PLAN_PROGRAM)
    exe = d / "plan"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-I", os.path.join(ROOT, "voxelraytracing_amd", "csrc"), "-o", str(exe), str(d / "plan.cpp")])
    return str(exe)


def test_a_lamp_lit_plan_without_the_sun(plan_program):
    """2 spp, 3 bounces: one sample per chain; per segment the lamp-lit trace launch (9 primary, 10 bounce) and the launch over its
    lamp rays (11) with its launch number; the resolve pass (7) behind each sample's chain."""
    head, steps = subprocess.check_output([plan_program], text=True).splitlines()
    assert head == "lamp 1 sun 0 cells 0 samples 1 emit 1"
    assert steps.split() == ["9:0:0:1", "11:0:0:0", "10:0:1:1", "11:0:1:0", "10:0:2:1", "11:0:2:0", "7:0:3:0",
                             "9:1:3:1", "11:1:3:0", "10:1:4:1", "11:1:4:0", "10:1:5:1", "11:1:5:0", "7:1:6:0"]


def test_a_lamp_lit_plan_with_the_sun(plan_program):
    """... and with the sun on, the sun launch (5) between the two: within a segment emission, sun, lamp."""
    head, steps = subprocess.check_output([plan_program, "sun"], text=True).splitlines()
    assert head == "lamp 1 sun 1 cells 0 samples 1 emit 1"
    assert steps.split() == ["9:0:0:1", "5:0:0:0", "11:0:0:0", "10:0:1:1", "5:0:1:0", "11:0:1:0", "10:0:2:1", "5:0:2:0", "11:0:2:0", "7:0:3:0",
                             "9:1:3:1", "5:1:3:0", "11:1:3:0", "10:1:4:1", "5:1:4:0", "11:1:4:0", "10:1:5:1", "5:1:5:0", "11:1:5:0", "7:1:6:0"]


def test_the_plan_checker_holds_lamp_lit_frames(tmp_path):
    """tools/check_frame_plan.cpp, built here as a program of its own, runs check_lamp_frames over every combination of the facts:
    a lamp-lit frame has the chains and finishing passes of the sun-lit frame, the lamp launch behind each trace launch."""
    exe = tmp_path / "check_frame_plan"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "voxelraytracing_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tools", "check_frame_plan.cpp")])
    out = subprocess.check_output([str(exe)], text=True)
    m = re.search(r"check_lamp_plan: ok \((\d+) lamp-lit frames, (\d+) launches\)", out)
    assert m and int(m.group(1)) > 10000 and int(m.group(2)) > int(m.group(1))

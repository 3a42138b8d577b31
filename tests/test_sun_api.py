"""vrt_set_sun_light (include/vrt.h) without a GPU: the header declares the struct and the function, the struct is 16 bytes as
a C compiler lays it out, libvrt.so exports the function, and every binding — _ffi, graphics.Gpu, the Rust vrt-sys crate —
carries it; a null context is refused before anything touches a device; the sun-lit kernels are kernels of their own.  What
needs a context — the other refusals, the no-op and what restarts the accumulation — is in tests/test_gpu_sun.py."""
import ctypes as C
import inspect
import os
import re
import subprocess

from voxelraytracing_amd import _ffi, graphics
from kernel_families import in_family, path_kernel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_the_struct_and_the_function():
    h = _read("include", "vrt.h")
    assert re.search(r"typedef\s+struct\s*\{\s*float\s+strength;[^}]*uint32_t\s+flags;[^}]*uint32_t\s+_reserved\[2\];[^}]*\}\s*vrt_sun_light\s*;", h)
    assert re.search(r"int\s+vrt_set_sun_light\s*\(\s*vrt_ctx\s*\*\s*ctx\s*,\s*const\s+vrt_sun_light\s*\*\s*opts\s*\)\s*;", h)


def test_the_struct_is_16_bytes(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vrt.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(vrt_sun_light), offsetof(vrt_sun_light, strength), '
                   'offsetof(vrt_sun_light, flags), offsetof(vrt_sun_light, _reserved)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["16", "0", "4", "8"]
    assert C.sizeof(_ffi.SunLight) == 16
    assert [(n, getattr(_ffi.SunLight, n).offset) for n, _ in _ffi.SunLight._fields_] == [("strength", 0), ("flags", 4), ("_reserved", 8)]


def test_the_library_exports_it():
    lib = _ffi.vrt()
    assert hasattr(lib, "vrt_set_sun_light")
    assert _ffi.VRT_SYMBOLS["vrt_set_sun_light"] == (C.c_int, [C.c_void_p, C.POINTER(_ffi.SunLight)])


def test_null_context_is_refused_without_a_device():
    lib = _ffi.vrt()
    o = _ffi.SunLight(1.0, 0, (C.c_uint32 * 2)(0, 0))
    assert lib.vrt_set_sun_light(None, C.byref(o)) == _ffi.VRT_ERR_INVALID_ARG
    assert lib.vrt_set_sun_light(None, None) == _ffi.VRT_ERR_INVALID_ARG


def test_python_binding():
    assert list(inspect.signature(graphics.Gpu.set_sun_light).parameters) == ["self", "strength"]


def test_rust_binding():
    rs = _read("bindings", "rust", "vrt-sys", "src", "lib.rs")
    assert re.search(r"pub struct vrt_sun_light \{\s*pub strength: f32,\s*pub flags: u32,\s*pub _reserved: \[u32; 2\],\s*\}", rs)
    assert re.search(r"pub fn vrt_set_sun_light\(ctx: \*mut vrt_ctx, opts: \*const vrt_sun_light\) -> c_int;", rs)
    assert re.search(r"size_of::<vrt_sun_light>\(\) == 16", rs)


def test_the_sun_lit_kernels_are_built_apart_from_the_others():
    """The sun term lives in instantiations of their own (SUN = SunLaunch of the two trace templates, tests/kernel_families.py),
    which take a SunLaunch behind FrameParams: every other kernel keeps its code (profiles/sun_isa_diff.txt).  One pair of trace kernels — the ten march forms each, whether there is a
    coat or a pass-through draw read from the launch, not a family per combination — the sun launch over the march cells in
    both layouts, and the ten march forms of the sun launch that counts; nothing spills."""
    regs = _ffi.kernel_registers()
    sun = {k: v for k, v in regs.items() if in_family(k, "sunlit") or "path_sun_" in k}
    assert sum(1 for k in sun if in_family(k, "sunlit") and path_kernel(k)["template"] == "primary" and k.endswith("EvNS_11FrameParamsEDpT6_")) == 10
    assert sum(1 for k in sun if in_family(k, "sunlit") and path_kernel(k)["template"] == "bounce" and k.endswith("EvNS_11FrameParamsEDpT5_")) == 10
    assert sorted(re.search(r"path_sun_cells_kernelI(Lb\d)E", k).group(1) for k in sun if "path_sun_cells_kernel" in k) == ["Lb0", "Lb1"]
    assert sum(1 for k in sun if "path_sun_kernel" in k) == 10
    assert len(sun) == 32
    bad = {k: v for k, v in sun.items() if v["scratch_bytes"] or v["sgpr_spills"] or v["vgpr_spills"]}
    assert not bad, bad
    # the other families are what they were
    assert sum(1 for k in regs if in_family(k, "translucent")) == 24 and sum(1 for k in regs if in_family(k, "polished")) == 24

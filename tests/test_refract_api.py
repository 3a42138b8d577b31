"""vrt_set_water_refraction (include/vrt.h) without a GPU: the header declares the struct and the function and states the contract,
the struct is 16 bytes as ctypes and the Rust crate have it, the library exports the function, a null context is refused, and the
refracting kernels are a pair of their own — the ten march builds each, everything in registers — beside a water family that is what
it was."""
import ctypes as C
import inspect
import os
import re
import subprocess

from kernel_families import MARCH_BUILDS, families, in_family, path_kernel, water_kernel
from voxelraytracing_amd import _ffi, graphics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REFRACT = re.compile(r"^_ZN3vrt\d+path_refract_(primary|bounce)_kernelI(Li\dELb\dELb\dE)EEvNS_11FrameParamsES1_NS_11WaterLaunchENS_9SunLaunchENS_13RefractLaunchE$")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_the_struct_and_the_function():
    h = _read("include", "vrt.h")
    assert re.search(r"typedef\s+struct\s*\{\s*float\s+ior;[^}]*uint32_t\s+max_span;[^}]*uint32_t\s+flags;[^}]*uint32_t\s+_reserved;[^}]*\}\s*vrt_water_refraction\s*;", h)
    assert re.search(r"int\s+vrt_set_water_refraction\s*\(\s*vrt_ctx\s*\*\s*ctx\s*,\s*const\s+vrt_water_refraction\s*\*\s*opts\s*\)\s*;", h)
    # a block of its own behind vrt_water_optics, whose own text is as it was
    assert h.index("} vrt_water_optics;") < h.index("Refraction for water") < h.index("} vrt_water_refraction;") < h.index("Camera sampling for VRT_MODE_PATH")
    doc = h[h.index("Refraction for water"):h.index("} vrt_water_refraction;")]
    for word in ("eta = 1.0f / ior", "cast_setup(o, d)", "cast_step", "vrt_get_voxels", "underside event", "total internal reflection", "max_span",
                 "vexp_neg(absorb[ch] * dist)", "rng_next(rng)", "!(s2 < 1)", "secondary_rays", "VRT_ERR_INVALID_ARG", "16 zero bytes", "[1, 4]", "1024",
                 "caustics", "dispersion", "vrt_set_lamp_light", "vrt_set_camera_sampling", "x.k - n.k * bias", "x.k + n.k * bias"):
        assert word in doc, word
    hh = _read("include", "vrt_host.h")
    assert "vrth_water_refract(" in hh and "vrth_world_water_span(" in hh


def test_the_struct_is_16_bytes(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vrt.h"\n#include "vrt_host.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(vrt_water_refraction), offsetof(vrt_water_refraction, ior), '
                   'offsetof(vrt_water_refraction, max_span), offsetof(vrt_water_refraction, flags), offsetof(vrt_water_refraction, _reserved), '
                   'sizeof(vrth_water_span)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["16", "0", "4", "8", "12", "40"]
    assert C.sizeof(_ffi.WaterRefraction) == 16 and C.sizeof(_ffi.WaterSpan) == 40
    assert [(n, getattr(_ffi.WaterRefraction, n).offset) for n, _ in _ffi.WaterRefraction._fields_] == [("ior", 0), ("max_span", 4), ("flags", 8),
                                                                                                      ("_reserved", 12)]


def test_the_library_exports_it():
    lib = _ffi.vrt()
    assert hasattr(lib, "vrt_set_water_refraction")
    assert _ffi.VRT_SYMBOLS["vrt_set_water_refraction"] == (C.c_int, [C.c_void_p, C.POINTER(_ffi.WaterRefraction)])
    assert hasattr(_ffi.host(), "vrth_water_refract") and hasattr(_ffi.host(), "vrth_world_water_span")


def test_null_context_is_refused_without_a_device():
    lib = _ffi.vrt()
    o = _ffi.WaterRefraction(1.33, 0, 0, 0)
    assert lib.vrt_set_water_refraction(None, C.byref(o)) == _ffi.VRT_ERR_INVALID_ARG
    assert lib.vrt_set_water_refraction(None, None) == _ffi.VRT_ERR_INVALID_ARG


def test_python_binding():
    sig = inspect.signature(graphics.Gpu.set_water_refraction)
    assert list(sig.parameters) == ["self", "ior", "max_span"] and sig.parameters["max_span"].default == 0


def test_rust_binding():
    rs = _read("bindings", "rust", "vrt-sys", "src", "lib.rs")
    assert re.search(r"pub struct vrt_water_refraction \{\s*pub ior: f32,\s*pub max_span: u32,\s*pub flags: u32,\s*pub _reserved: u32,\s*\}", rs)
    assert re.search(r"pub fn vrt_set_water_refraction\(ctx: \*mut vrt_ctx, opts: \*const vrt_water_refraction\) -> c_int;", rs)
    assert re.search(r"size_of::<vrt_water_refraction>\(\) == 16", rs)


def test_the_library_holds_exactly_the_ten_march_builds_of_each_refracting_kernel():
    regs = _ffi.kernel_registers()
    mine = {k: _REFRACT.match(k) for k in regs if "refract" in k}
    assert len(mine) == 20 and all(mine.values()), [k for k, m in mine.items() if not m]
    for template in ("primary", "bounce"):
        builds = sorted(m.group(2) for m in mine.values() if m.group(1) == template)
        assert builds == sorted(MARCH_BUILDS), (template, builds)


def test_the_refracting_kernels_keep_everything_in_registers():
    regs = _ffi.kernel_registers()
    mine = {k: v for k, v in regs.items() if "path_refract_" in k}
    assert len(mine) == 20
    bad = {k: v for k, v in mine.items() if v["scratch_bytes"] or v["sgpr_spills"] or v["vgpr_spills"]}
    assert not bad, bad


def test_the_new_pair_is_no_water_symbol_and_the_water_family_is_what_it_was():
    regs = _ffi.kernel_registers()
    mine = [k for k in regs if "path_refract_" in k]
    assert mine and not [k for k in mine if "water" in k]
    assert all(families(k) == frozenset() and water_kernel(k) is None and path_kernel(k) is None for k in mine)
    water = [k for k in regs if "water" in k]
    assert len(water) == 23 and sum(1 for k in regs if in_family(k, "water")) == 20
    assert sum(1 for k in water if "path_water_primary_kernel" in k) == 10 and sum(1 for k in water if "path_water_bounce_kernel" in k) == 10

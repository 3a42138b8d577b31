"""vrt_write_emission (include/vrt.h) without a GPU: the header declares it, libvrt.so exports it, and every binding — _ffi,
graphics.Gpu, the Rust vrt-sys crate — carries it; a null context is refused before anything touches a device."""
import ctypes as C
import inspect
import os
import re

from voxelraytracing_amd import _ffi, graphics
from kernel_families import in_family, path_kernel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_the_function():
    h = _read("include", "vrt.h")
    assert re.search(r"int\s+vrt_write_emission\s*\(\s*vrt_ctx\s*\*\s*ctx\s*,\s*uint32_t\s+first\s*,\s*const\s+float\s*\*\s*emission\s*,"
                     r"\s*uint32_t\s+n\s*\)\s*;", h)


def test_the_library_exports_it():
    lib = _ffi.vrt()
    assert hasattr(lib, "vrt_write_emission")
    assert _ffi.VRT_SYMBOLS["vrt_write_emission"] == (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32])


def test_null_context_is_refused_without_a_device():
    lib = _ffi.vrt()
    vals = (C.c_float * 4)(1.0, 0.0, 2.0, 0.5)
    assert lib.vrt_write_emission(None, 0, vals, 4) == _ffi.VRT_ERR_INVALID_ARG
    assert lib.vrt_write_emission(None, 0, None, 0) == _ffi.VRT_ERR_INVALID_ARG


def test_python_binding():
    params = inspect.signature(graphics.Gpu.write_emission).parameters
    assert list(params) == ["self", "values", "first"] and params["first"].default == 0


def test_rust_binding():
    rs = _read("bindings", "rust", "vrt-sys", "src", "lib.rs")
    assert re.search(r"pub fn vrt_write_emission\(ctx: \*mut vrt_ctx, first: u32, emission: \*const f32, n: u32\) -> c_int;", rs)


def test_the_emissive_kernels_are_built_apart_from_the_plain_ones():
    """The emission term lives in instantiations of their own: the plain frame's kernels keep their code (tools/isa_diff.py
    compares two builds), and none of the new ones spills."""
    regs = _ffi.kernel_registers()
    emissive_cells = {k: v for k, v in regs.items() if in_family(k, "emissive")}
    assert len(emissive_cells) == 3 and all(v["vgprs"] <= 64 for v in emissive_cells.values()), emissive_cells
    # <MARCH, LDS_ROOTS, STATS, (MULTI,) EMIT = true>: the ten march forms each, + the primary's chained one
    kernels = {k: path_kernel(k) for k in regs}
    emit_alone = {k: p for k, p in kernels.items() if p and p["emit"] and not (p["polish"] or p["translucent"] or p["sun"])}
    assert sum(1 for k, p in emit_alone.items() if p["template"] == "primary" and k.endswith("EvNS_11FrameParamsEDpT6_")) == 11
    assert sum(1 for k, p in emit_alone.items() if p["template"] == "bounce" and k.endswith("EvNS_11FrameParamsEDpT5_")) == 10
    bad = {k: v for k, v in regs.items() if in_family(k, "emissive") and (v["scratch_bytes"] or v["sgpr_spills"] or v["vgpr_spills"])}
    assert not bad

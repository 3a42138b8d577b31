"""vrt_write_translucency (include/vrt.h) without a GPU: the header declares the struct and the function, libvrt.so exports it,
and every binding — _ffi, graphics.Gpu, the Rust vrt-sys crate — carries it; a null context is refused before anything touches
a device; the kernels that draw whether a path passes through are kernels of their own."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

from voxelraytracing_amd import _ffi, graphics
from kernel_families import in_family, path_kernel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_the_struct_and_the_function():
    h = _read("include", "vrt.h")
    assert re.search(r"typedef\s+struct\s*\{\s*float\s+color\[3\];[^}]*float\s+chance;[^}]*\}\s*vrt_translucency\s*;", h)
    assert re.search(r"int\s+vrt_write_translucency\s*\(\s*vrt_ctx\s*\*\s*ctx\s*,\s*uint32_t\s+first\s*,\s*const\s+vrt_translucency\s*\*\s*entries\s*,"
                     r"\s*uint32_t\s+n\s*\)\s*;", h)


def test_the_struct_is_16_bytes(tmp_path):
    """sizeof(vrt_translucency) and its offsets as a C compiler lays the header's struct out, and the same in the numpy dtype."""
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vrt.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(vrt_translucency), offsetof(vrt_translucency, color), '
                   'offsetof(vrt_translucency, chance)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["16", "0", "12"]
    d = _ffi.TRANSLUCENCY_DTYPE
    assert d.itemsize == 16 and d.names == ("color", "chance")
    assert [d.fields[n][1] for n in d.names] == [0, 12]
    assert d["color"].shape == (3,) and d["color"].base == np.dtype("<f4") and d["chance"] == np.dtype("<f4")


def test_the_library_exports_it():
    lib = _ffi.vrt()
    assert hasattr(lib, "vrt_write_translucency")
    assert _ffi.VRT_SYMBOLS["vrt_write_translucency"] == (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32])


def test_null_context_is_refused_without_a_device():
    lib = _ffi.vrt()
    entries = np.zeros(4, _ffi.TRANSLUCENCY_DTYPE)
    entries["chance"] = 0.5
    assert lib.vrt_write_translucency(None, 0, entries.ctypes.data, 4) == _ffi.VRT_ERR_INVALID_ARG
    assert lib.vrt_write_translucency(None, 0, None, 0) == _ffi.VRT_ERR_INVALID_ARG


def test_python_binding():
    params = inspect.signature(graphics.Gpu.write_translucency).parameters
    assert list(params) == ["self", "entries", "first"] and params["first"].default == 0


def test_rust_binding():
    rs = _read("bindings", "rust", "vrt-sys", "src", "lib.rs")
    assert re.search(r"pub struct vrt_translucency \{\s*pub color: \[f32; 3\],\s*pub chance: f32,\s*\}", rs)
    assert re.search(r"pub fn vrt_write_translucency\(ctx: \*mut vrt_ctx, first: u32, entries: \*const vrt_translucency, n: u32\) -> c_int;", rs)
    assert re.search(r"size_of::<vrt_translucency>\(\) == 16", rs)


def test_the_translucent_kernels_are_built_apart_from_the_others():
    """The draw lives in instantiations of their own (TRANSLUCENT of the three templates, tests/kernel_families.py): every other
    kernel keeps its code (tools/isa_diff.py compares two builds).  The family has the polished one's instantiations and no others — the coat's draw is under a word on
    the device, not a template argument; its pool kernel stays at 64 VGPRs (eight waves a SIMD), and nothing spills."""
    regs = _ffi.kernel_registers()
    translucent = {k: v for k, v in regs.items() if in_family(k, "translucent")}
    cells = {k: v for k, v in translucent.items() if path_kernel(k)["template"] == "bounce_cells"}
    assert len(cells) == 3 and all(v["vgprs"] <= 64 for v in cells.values()), cells
    assert sorted(path_kernel(k)["build"] for k in cells) == ["Lb0ELj4E", "Lb1ELj4E", "Lb1ELj5E"]
    # <MARCH, LDS_ROOTS, STATS, (MULTI,) EMIT = true>: the ten march forms each, + the primary's chained one
    assert sum(1 for k in translucent if path_kernel(k)["template"] == "primary" and path_kernel(k)["emit"] and k.endswith("EvNS_11FrameParamsEDpT6_")) == 11
    assert sum(1 for k in translucent if path_kernel(k)["template"] == "bounce" and path_kernel(k)["emit"] and k.endswith("EvNS_11FrameParamsEDpT5_")) == 10
    assert len(translucent) == 24
    bad = {k: v for k, v in translucent.items() if v["scratch_bytes"] or v["sgpr_spills"] or v["vgpr_spills"]}
    assert not bad
    # the polished family is what it was
    assert sum(1 for k in regs if in_family(k, "polished")) == 24

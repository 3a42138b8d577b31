"""vrt_set_tone_map / vrt_get_tone_info / vrt_read_tone_histogram (include/vrt.h) without a GPU: the header declares the structs,
the constants and the functions, the structs are laid out as a C compiler lays them out, both libraries export what the headers
declare, and every binding — _ffi, graphics.Gpu, the Rust vrt-sys crate — carries them; a null context is refused before anything
touches a device; the metering kernels and the mapped blits are kernels of libvrt.so and spill nothing.  What needs a context is
in tests/test_gpu_tone.py."""
import ctypes as C
import inspect
import os
import re
import subprocess

from voxelraytracing_amd import _ffi, graphics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


MAP_FIELDS = [("curve", 0), ("flags", 4), ("exposure", 8), ("white", 12), ("key", 16), ("adapt", 20), ("min_auto", 24), ("max_auto", 28),
              ("percentile", 32), ("_reserved", 36)]
INFO_FIELDS = [("exposure", 0), ("target", 4), ("luminance", 8), ("bin", 12), ("counted", 16), ("skipped", 24), ("frames", 32), ("_reserved", 36)]
CONSTANTS = {"VRT_TONE_OFF": 0, "VRT_TONE_LINEAR": 1, "VRT_TONE_REINHARD": 2, "VRT_TONE_FILMIC": 3, "VRT_TONE_AUTO": 1, "VRT_TONE_GAMMA2": 2}


def test_header_declares_the_interface():
    h = _read("include", "vrt.h")
    for name, val in CONSTANTS.items():
        assert re.search(rf"#define\s+{name}\s+{val}u\b", h), name
    assert re.search(r"int\s+vrt_set_tone_map\s*\(\s*vrt_ctx\s*\*\s*ctx\s*,\s*const\s+vrt_tone_map\s*\*\s*opts\s*\)\s*;", h)
    assert re.search(r"int\s+vrt_get_tone_info\s*\(\s*vrt_ctx\s*\*\s*ctx\s*,\s*vrt_tone_info\s*\*\s*out\s*\)\s*;", h)
    assert re.search(r"int\s+vrt_read_tone_histogram\s*\(\s*vrt_ctx\s*\*\s*ctx\s*,\s*uint32_t\s+bins\[256\]\s*\)\s*;", h)
    hh = _read("include", "vrt_host.h")
    assert re.search(r"int\s+vrth_tone_meter\s*\(", hh) and re.search(r"int\s+vrth_tone_map\s*\(", hh)


def test_the_structs_as_a_c_compiler_lays_them_out(tmp_path):
    def offs(t, fields):
        return ", ".join(f"offsetof({t}, {n})" for n, _ in fields)
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vrt.h"\nint main(void) {\n'
                   f'  size_t a[] = {{sizeof(vrt_tone_map), {offs("vrt_tone_map", MAP_FIELDS)}}};\n'
                   f'  size_t b[] = {{sizeof(vrt_tone_info), {offs("vrt_tone_info", INFO_FIELDS)}}};\n'
                   '  for (size_t i = 0; i < sizeof a / sizeof *a; i++) printf("%zu ", a[i]);\n  printf("\\n");\n'
                   '  for (size_t i = 0; i < sizeof b / sizeof *b; i++) printf("%zu ", b[i]);\n  printf("\\n");\n'
                   f'  printf("%u %u %u %u %u %u\\n", {", ".join(CONSTANTS)});\n  return 0;\n}}\n')
    exe = tmp_path / "size"
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    a, b, consts = subprocess.check_output([str(exe)], text=True).strip().split("\n")
    assert [int(x) for x in a.split()] == [48] + [o for _, o in MAP_FIELDS]
    assert [int(x) for x in b.split()] == [40] + [o for _, o in INFO_FIELDS]
    assert [int(x) for x in consts.split()] == list(CONSTANTS.values())
    assert C.sizeof(_ffi.ToneMap) == 48 and C.sizeof(_ffi.ToneInfo) == 40
    assert [(n, getattr(_ffi.ToneMap, n).offset) for n, _ in _ffi.ToneMap._fields_] == MAP_FIELDS
    assert [(n, getattr(_ffi.ToneInfo, n).offset) for n, _ in _ffi.ToneInfo._fields_] == INFO_FIELDS
    assert (_ffi.TONE_OFF, _ffi.TONE_LINEAR, _ffi.TONE_REINHARD, _ffi.TONE_FILMIC, _ffi.TONE_AUTO, _ffi.TONE_GAMMA2) == tuple(CONSTANTS.values())


def test_the_libraries_export_them():
    lib, host = _ffi.vrt(), _ffi.host()
    assert _ffi.VRT_SYMBOLS["vrt_set_tone_map"] == (C.c_int, [C.c_void_p, C.POINTER(_ffi.ToneMap)])
    assert _ffi.VRT_SYMBOLS["vrt_get_tone_info"] == (C.c_int, [C.c_void_p, C.POINTER(_ffi.ToneInfo)])
    assert _ffi.VRT_SYMBOLS["vrt_read_tone_histogram"] == (C.c_int, [C.c_void_p, C.c_void_p])
    for name in ("vrt_set_tone_map", "vrt_get_tone_info", "vrt_read_tone_histogram"):
        assert hasattr(lib, name)
    for name in ("vrth_tone_meter", "vrth_tone_map"):
        assert hasattr(host, name) and name in _ffi.VRTH_SYMBOLS


def test_null_context_is_refused_without_a_device():
    lib = _ffi.vrt()
    o = _ffi.tone_setting(_ffi.TONE_FILMIC, 1.0, auto=True)
    assert lib.vrt_set_tone_map(None, C.byref(o)) == _ffi.VRT_ERR_INVALID_ARG
    assert lib.vrt_set_tone_map(None, None) == _ffi.VRT_ERR_INVALID_ARG
    info, bins = _ffi.ToneInfo(), (C.c_uint32 * 256)()
    assert lib.vrt_get_tone_info(None, C.byref(info)) == _ffi.VRT_ERR_INVALID_ARG
    assert lib.vrt_read_tone_histogram(None, bins) == _ffi.VRT_ERR_INVALID_ARG


def test_python_binding():
    assert list(inspect.signature(graphics.Gpu.set_tone_map).parameters) == ["self", "curve", "exposure", "auto", "gamma2", "white", "key", "adapt",
                                                                             "min_auto", "max_auto", "percentile", "opts"]
    assert list(inspect.signature(graphics.Gpu.tone_info).parameters) == ["self"]
    assert list(inspect.signature(graphics.Gpu.tone_histogram).parameters) == ["self"]
    o = _ffi.tone_setting(_ffi.TONE_REINHARD, 2.0, auto=True, gamma2=True, white=4.0)
    assert (o.curve, o.flags, o.exposure, o.white, o.percentile, list(o._reserved)) == (2, 3, 2.0, 4.0, 500, [0, 0, 0])


def test_rust_binding():
    rs = _read("bindings", "rust", "vrt-sys", "src", "lib.rs")
    assert re.search(r"pub struct vrt_tone_map \{\s*pub curve: u32,\s*pub flags: u32,\s*pub exposure: f32,\s*pub white: f32,\s*pub key: f32,\s*pub adapt: f32,\s*"
                     r"pub min_auto: f32,\s*pub max_auto: f32,\s*pub percentile: u32,\s*pub _reserved: \[u32; 3\],\s*\}", rs)
    assert re.search(r"pub struct vrt_tone_info \{\s*pub exposure: f32,\s*pub target: f32,\s*pub luminance: f32,\s*pub bin: u32,\s*pub counted: u64,\s*"
                     r"pub skipped: u64,\s*pub frames: u32,\s*pub _reserved: u32,\s*\}", rs)
    assert re.search(r"pub fn vrt_set_tone_map\(ctx: \*mut vrt_ctx, opts: \*const vrt_tone_map\) -> c_int;", rs)
    assert re.search(r"pub fn vrt_get_tone_info\(ctx: \*mut vrt_ctx, out: \*mut vrt_tone_info\) -> c_int;", rs)
    assert re.search(r"pub fn vrt_read_tone_histogram\(ctx: \*mut vrt_ctx, bins: \*mut u32\) -> c_int;", rs)
    assert re.search(r"size_of::<vrt_tone_map>\(\) == 48", rs) and re.search(r"size_of::<vrt_tone_info>\(\) == 40", rs)
    for name, val in CONSTANTS.items():
        assert re.search(rf"pub const {name}: u32 = {val};", rs), name


def test_the_kernels_are_in_the_library_and_spill_nothing():
    """The two metering kernels, and the mapped blits beside the unmapped ones (which keep their own code: a kernel each)."""
    regs = _ffi.kernel_registers()
    for name in ("tone_histogram_kernel", "tone_finish_kernel", "present_tone_kernel", "present_plain_tone_kernel", "present_kernel", "present_plain_kernel"):
        found = {k: v for k, v in regs.items() if re.search(rf"\d+{name}[A-Z]", k)}
        assert len(found) == 1, (name, sorted(found))
        v = next(iter(found.values()))
        assert not (v["scratch_bytes"] or v["sgpr_spills"] or v["vgpr_spills"]), (name, v)

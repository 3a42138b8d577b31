"""The surface of the path trace's denoiser (vrt_set_denoise / vrt_read_guide / vrth_denoise) without a GPU: the header, the
ctypes bindings, the Rust binding and the 16-byte options struct say the same thing."""
import ctypes as C
import os
import re

from voxelraytracing_amd import Gpu, _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_header_declares_the_struct_and_the_calls():
    hdr = re.sub(r"/\*.*?\*/", "", _read("include", "vrt.h"), flags=re.S)
    m = re.search(r"typedef struct vrt_denoise_opts \{(.*?)\} vrt_denoise_opts;", hdr, re.S)
    assert m, "include/vrt.h has no vrt_denoise_opts"
    fields = re.findall(r"(uint32_t|float)\s+(\w+);", m.group(1))
    assert fields == [("uint32_t", "passes"), ("float", "sigma_color"), ("uint32_t", "flags"), ("uint32_t", "_reserved")]
    assert re.search(r"int vrt_set_denoise\(vrt_ctx \*ctx, const vrt_denoise_opts \*opts\);", hdr)
    assert re.search(r"int vrt_read_guide\(vrt_ctx \*ctx, uint32_t \*guide\);", hdr)
    host = re.sub(r"/\*.*?\*/", "", _read("include", "vrt_host.h"), flags=re.S)
    assert re.search(r"int vrth_denoise\(const float \*rgb, const uint32_t \*ids, const uint32_t \*guide, uint32_t w, uint32_t h, "
                     r"const vrt_denoise_opts \*opts, float \*out\);", host)


def test_the_bindings_carry_them():
    assert C.sizeof(_ffi.DenoiseOpts) == 16
    assert [(n, t) for n, t in _ffi.DenoiseOpts._fields_] == [("passes", C.c_uint32), ("sigma_color", C.c_float), ("flags", C.c_uint32),
                                                             ("_reserved", C.c_uint32)]
    assert (_ffi.DenoiseOpts.sigma_color.offset, _ffi.DenoiseOpts.flags.offset, _ffi.DenoiseOpts._reserved.offset) == (4, 8, 12)
    lib, host = _ffi.vrt(), _ffi.host()
    assert lib.vrt_set_denoise.argtypes == [C.c_void_p, C.POINTER(_ffi.DenoiseOpts)] and lib.vrt_read_guide.argtypes == [C.c_void_p, C.c_void_p]
    assert host.vrth_denoise.restype is C.c_int
    assert callable(Gpu.set_denoise) and callable(Gpu.read_guide) and callable(_ffi.denoise)
    assert 1 <= _ffi.DENOISE_PASSES <= 5 and _ffi.DENOISE_SIGMA_COLOR >= 0.0
    # no context: an argument error, not a crash (nothing touches a GPU)
    o = _ffi.DenoiseOpts(2, 0.5, 0, 0)
    assert lib.vrt_set_denoise(None, C.byref(o)) == _ffi.VRT_ERR_INVALID_ARG
    assert lib.vrt_read_guide(None, None) == _ffi.VRT_ERR_INVALID_ARG


def test_the_rust_binding_declares_the_same():
    src = _read("bindings", "rust", "vrt-sys", "src", "lib.rs")
    m = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct vrt_denoise_opts \{(.*?)\}", src, re.S)
    assert m, "bindings/rust/vrt-sys has no vrt_denoise_opts"
    assert re.findall(r"pub (\w+): (\w+),", m.group(1)) == [("passes", "u32"), ("sigma_color", "f32"), ("flags", "u32"), ("_reserved", "u32")]
    assert re.search(r"pub fn vrt_set_denoise\(ctx: \*mut vrt_ctx, opts: \*const vrt_denoise_opts\) -> c_int;", src)
    assert re.search(r"pub fn vrt_read_guide\(ctx: \*mut vrt_ctx, guide: \*mut u32\) -> c_int;", src)
    assert re.search(r"size_of::<vrt_denoise_opts>\(\) == 16", src)

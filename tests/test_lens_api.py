"""vrt_set_camera_sampling (include/vrt.h) without a GPU: the header declares the struct and the function, the struct is 16 bytes
as a C compiler lays it out, libvrt.so exports the function, and every binding — _ffi, graphics.Gpu, the Rust vrt-sys crate —
carries it; a null context is refused before anything touches a device; the kernels of a frame with the setting on are kernels
of their own and spill nothing.  What needs a context — the other refusals, off after on and what restarts the accumulation — is
in tests/test_gpu_lens.py."""
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
    assert re.search(r"typedef\s+struct\s*\{\s*float\s+pixel_spread;[^}]*float\s+aperture;[^}]*float\s+focus_distance;[^}]*uint32_t\s+flags;[^}]*\}"
                     r"\s*vrt_camera_sampling\s*;", h)
    assert re.search(r"int\s+vrt_set_camera_sampling\s*\(\s*vrt_ctx\s*\*\s*ctx\s*,\s*const\s+vrt_camera_sampling\s*\*\s*opts\s*\)\s*;", h)


def test_the_struct_is_16_bytes(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vrt.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(vrt_camera_sampling), offsetof(vrt_camera_sampling, pixel_spread), '
                   'offsetof(vrt_camera_sampling, aperture), offsetof(vrt_camera_sampling, focus_distance), '
                   'offsetof(vrt_camera_sampling, flags)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["16", "0", "4", "8", "12"]
    assert C.sizeof(_ffi.CameraSampling) == 16
    assert [(n, getattr(_ffi.CameraSampling, n).offset) for n, _ in _ffi.CameraSampling._fields_] == \
        [("pixel_spread", 0), ("aperture", 4), ("focus_distance", 8), ("flags", 12)]


def test_the_library_exports_it():
    lib = _ffi.vrt()
    assert hasattr(lib, "vrt_set_camera_sampling")
    assert _ffi.VRT_SYMBOLS["vrt_set_camera_sampling"] == (C.c_int, [C.c_void_p, C.POINTER(_ffi.CameraSampling)])
    assert hasattr(_ffi.host(), "vrth_lens_ray")   # csrc/both/lens_math.h on the host (tests/test_lens_ref.py)


def test_null_context_is_refused_without_a_device():
    lib = _ffi.vrt()
    o = _ffi.CameraSampling(1.0, 0.0, 0.0, 0)
    assert lib.vrt_set_camera_sampling(None, C.byref(o)) == _ffi.VRT_ERR_INVALID_ARG
    assert lib.vrt_set_camera_sampling(None, None) == _ffi.VRT_ERR_INVALID_ARG


def test_python_binding():
    sig = inspect.signature(graphics.Gpu.set_camera_sampling)
    assert list(sig.parameters) == ["self", "pixel_spread", "aperture", "focus_distance"]
    assert sig.parameters["pixel_spread"].default is inspect.Parameter.empty
    assert sig.parameters["aperture"].default == 0.0 and sig.parameters["focus_distance"].default == 0.0


def test_rust_binding():
    rs = _read("bindings", "rust", "vrt-sys", "src", "lib.rs")
    assert re.search(r"pub struct vrt_camera_sampling \{\s*pub pixel_spread: f32,\s*pub aperture: f32,\s*pub focus_distance: f32,\s*pub flags: u32,\s*\}", rs)
    assert re.search(r"pub fn vrt_set_camera_sampling\(ctx: \*mut vrt_ctx, opts: \*const vrt_camera_sampling\) -> c_int;", rs)
    assert re.search(r"size_of::<vrt_camera_sampling>\(\) == 16", rs)


def test_the_lens_kernels_are_built_apart_from_the_others():
    """Camera sampling lives in a primary kernel template of its own, path_lens_primary_kernel, which takes a LensLaunch behind
    FrameParams (and a SunLaunch behind that in its sun-lit form): every other kernel keeps its code (profiles/lens_isa_diff.txt).
    The ten march forms each and the one form of several samples per chain; whether there is a coat or a pass-through draw is
    read from the launch, not a family per combination.  Nothing spills: their sample loop reads its arguments anew per trip
    (vrt_path_lens.h) — read once in front of the loop they cost up to 43 spilled scalar registers."""
    regs = _ffi.kernel_registers()
    lens = {k: v for k, v in regs.items() if in_family(k, "lens")}
    plain = [k for k in lens if not path_kernel(k)["sun"] and re.search(r"FrameParamsENS_10LensLaunchEDpT", k)]
    sunlit = [k for k in lens if path_kernel(k)["sun"] and re.search(r"FrameParamsENS_10LensLaunchEDpT", k)]
    chained = [k for k in plain if path_kernel(k)["multi"] and path_kernel(k)["build"] == "Li0ELb0ELb0E"]
    assert len(plain) == 11 and len(chained) == 1 and sum(1 for k in plain if path_kernel(k)["multi"]) == 1   # (+ several samples per chain)
    assert not [k for k in sunlit if path_kernel(k)["multi"]]
    assert len(sunlit) == 10
    assert len(lens) == 21
    bad = {k: v for k, v in lens.items() if v["scratch_bytes"] or v["sgpr_spills"] or v["vgpr_spills"]}
    assert not bad, bad
    # the other families are what tests/test_sun_api.py records
    assert sum(1 for k in regs if in_family(k, "sunlit") or "path_sun_" in k) == 32
    assert sum(1 for k in regs if in_family(k, "translucent")) == 24 and sum(1 for k in regs if in_family(k, "polished")) == 24

"""The C-ABI libraries load without a GPU and export exactly what include/*.h declares."""
import ctypes as C
import os
import re

import pytest

from voxelraytracing_amd import _ffi
from kernel_families import path_kernel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header, prefix):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(" + prefix + r"\w+)\s*\(", src)))


def test_vrt_exports_every_declared_symbol():
    lib = _ffi.vrt()
    names = _declared("vrt.h", "vrt_")
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), n
    assert sorted(_ffi.VRT_SYMBOLS) == names, "bindings drifted from include/vrt.h"


def test_vrt_host_exports_every_declared_symbol():
    lib = _ffi.host()
    names = _declared("vrt_host.h", "vrth_")
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), n
    assert sorted(_ffi.VRTH_SYMBOLS) == names, "bindings drifted from include/vrt_host.h"


def test_uniform_struct_layouts_match_the_reference():
    # clientdesktop/src/graphics/mod.rs:20-28, 82-91, 113-120, 132-143
    assert C.sizeof(_ffi.Material) == 32 and _ffi.Material.is_liquid.offset == 16 and _ffi.Material.scatter.offset == 20
    assert C.sizeof(_ffi.CamData) == 160
    assert (_ffi.CamData.inv_view_mat.offset, _ffi.CamData.inv_proj_mat.offset, _ffi.CamData.proj_size.offset) == (16, 80, 144)
    assert C.sizeof(_ffi.WorldData) == 32 and _ffi.WorldData.size.offset == 12 and _ffi.WorldData.size_in_chunks.offset == 16
    assert C.sizeof(_ffi.Settings) == 48
    assert (_ffi.Settings.sun_intensity.offset, _ffi.Settings.show_step_count.offset, _ffi.Settings.sky_color.offset,
            _ffi.Settings.sun_pos.offset) == (4, 8, 16, 32)


def test_missing_library_fails_loudly(tmp_path, monkeypatch):
    monkeypatch.setattr(_ffi, "_HERE", str(tmp_path))
    with pytest.raises(ImportError, match="no fallback"):
        _ffi._load("libvrt.so", _ffi.VRT_SYMBOLS)


def test_create_validates_arguments_without_touching_the_gpu():
    lib = _ffi.vrt()
    h = C.c_void_p()
    for cfg in (_ffi.Config(1024, 2, 0, 64, -1, 0, 1, 0),    # an empty result texture
                _ffi.Config(1, 2, 64, 64, -1, 0, 1, 0),      # max_nodes < 2
                _ffi.Config(1024, 2, 64, 64, -1, 3, 2, 0)):  # shard_rank >= shard_count
        assert lib.vrt_create(C.byref(cfg), C.byref(h)) == -1
        assert lib.vrt_last_error(None)
    assert lib.vrt_create(None, C.byref(h)) == -1


def test_rust_sys_crate_declares_the_same_abi():
    """bindings/rust/vrt-sys (not compilable here: no cargo) must name every function of include/vrt.h with the same
    number of parameters, and its struct sizes (asserted in its own #[test]) must be the ctypes ones."""
    src = open(os.path.join(ROOT, "bindings", "rust", "vrt-sys", "src", "lib.rs")).read()
    rust = {m.group(1): m.group(2) for m in re.finditer(r"pub fn (vrt_\w+)\(([^)]*)\)", src)}
    hdr = open(os.path.join(ROOT, "include", "vrt.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    c_fns = {m.group(1): m.group(2) for m in re.finditer(r"\b(vrt_\w+)\s*\(([^)]*)\)\s*;", hdr)}
    assert sorted(rust) == sorted(c_fns) == sorted(_ffi.VRT_SYMBOLS)
    for name, params in c_fns.items():
        assert len([p for p in params.split(",") if p.strip()]) == len([p for p in rust[name].split(",") if p.strip()]), name
    sizes = {m.group(1): int(m.group(2)) for m in re.finditer(r"size_of::<(\w+)>\(\), (\d+)\)", src)}
    want = {"vrt_material": _ffi.Material, "vrt_cam_data": _ffi.CamData, "vrt_world_data": _ffi.WorldData, "vrt_settings": _ffi.Settings,
            "vrt_crosshair": _ffi.Crosshair, "vrt_config": _ffi.Config, "vrt_render_opts": _ffi.RenderOpts, "vrt_stats": _ffi.Stats,
            "vrt_accel_info": _ffi.AccelInfo, "vrt_issue_profile": _ffi.IssueProfile}
    assert sizes == {k: C.sizeof(v) for k, v in want.items()}
    for flag, val in (("VRT_FLAG_TILE_MAJOR", 1), ("VRT_FLAG_ROW_MAJOR", 2), ("VRT_FLAG_COMPACT", 4)):
        assert re.search(rf"#define {flag} {val}u", hdr) and re.search(rf"pub const {flag}: u32 = {val};", src)


def test_no_kernel_of_the_library_spills_registers():
    """Every gfx950 kernel of libvrt.so: no scratch, no spilled SGPRs or VGPRs (code-object metadata; _ffi.kernel_registers says
    why a spill is an error here), and the path trace's bounce kernel within the 64 VGPRs of eight waves a SIMD."""
    regs = _ffi.kernel_registers()
    assert len(regs) >= 40, f"only {len(regs)} kernels found in libvrt.so's fat binary"
    bad = {k: v for k, v in regs.items() if v["scratch_bytes"] or v["sgpr_spills"] or v["vgpr_spills"]}
    assert not bad, f"kernels that spill: {bad}"
    bounce = {k: v for k, v in regs.items() if "path_bounce_cells_kernel" in k and not path_kernel(k)["emit"]}   # (the plain frame's)
    assert len(bounce) == 3 and all(v["vgprs"] <= 64 for v in bounce.values()), bounce   # (direct x 256- / 320-ray pools, blocks x 256)

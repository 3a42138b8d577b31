"""The column queries' records and constants (include/vrt.h: vrt_get_voxels, vrt_column_tops, vrt_read_top_map) as the bindings
hold them, and the argument checks that need no GPU."""
import ctypes as C
import os
import re

import numpy as np

from voxelraytracing_amd import _ffi

import column_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_record_sizes_and_layouts():
    assert [C.sizeof(t) for t in (_ffi.VoxelAt, _ffi.ColumnQuery, _ffi.ColumnTop, _ffi.TopEntry)] == [4, 16, 16, 8]
    assert [d.itemsize for d in (_ffi.VOXEL_AT_DTYPE, _ffi.COLUMN_QUERY_DTYPE, _ffi.COLUMN_TOP_DTYPE, _ffi.TOP_ENTRY_DTYPE)] == [4, 16, 16, 8]
    for ct, dt in ((_ffi.VoxelAt, _ffi.VOXEL_AT_DTYPE), (_ffi.ColumnQuery, _ffi.COLUMN_QUERY_DTYPE), (_ffi.ColumnTop, _ffi.COLUMN_TOP_DTYPE),
                   (_ffi.TopEntry, _ffi.TOP_ENTRY_DTYPE)):
        assert [(n, getattr(ct, n).offset) for n, _ in ct._fields_] == [(n, dt.fields[n][1]) for n in dt.names]


def test_the_constants_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "vrt.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "vrt-sys", "src", "lib.rs")).read()
    for name, val in (("VOXEL_OK", 0), ("VOXEL_OUT_OF_BOUNDS", 1), ("VOXEL_NO_CHUNK", 3), ("COLUMN_FROM_Y", 1), ("COLUMN_SOLID", 2),
                      ("COLUMN_NONE", 0), ("COLUMN_FOUND", 1), ("COLUMN_OUTSIDE", 2)):
        assert getattr(_ffi, name) == val
        assert re.search(rf"#define VRT_{name} {val}u", hdr), name
        assert re.search(rf"pub const VRT_{name}: u\d+ = {val};", rust), name
    for rec, size in (("vrt_voxel_at", 4), ("vrt_column_query", 16), ("vrt_column_top", 16), ("vrt_top_entry", 8)):
        assert re.search(rf"size_of::<{rec}>\(\) == {size}\)", rust), rec


def test_the_statuses_are_the_numbers_get_voxel_returns():
    """VRT_VOXEL_* are SetVoxelErr's numbers: what vrth_world_get_voxel returns for a voxel, for a position outside the world
    and for one in a missing chunk."""
    w = cc.case("leaf").world
    lib = _ffi.host()
    v = C.c_uint16()

    def get(p):
        return lib.vrth_world_get_voxel(w._h, (C.c_int32 * 3)(*p), C.byref(v))

    x, y, z = cc.LEAF_TOPS[16]
    assert get((x - 32, y - 32, z - 32)) == _ffi.VOXEL_OK and v.value == cc.STONE
    assert get((-33, 0, 0)) == _ffi.VOXEL_OUT_OF_BOUNDS and get((0, 0, 1000)) == _ffi.VOXEL_OUT_OF_BOUNDS
    assert get((10, 10, 10)) == _ffi.VOXEL_NO_CHUNK
    want = cc.ref_get_voxels(cc.case("leaf").dw, [(x - 32, y - 32, z - 32), (-33, 0, 0), (0, 0, 1000), (10, 10, 10)])
    assert want["status"].tolist() == [0, 1, 1, 3] and want["voxel"].tolist() == [cc.STONE, 0, 0, 0]


def test_null_contexts_are_refused_without_touching_the_gpu():
    lib = _ffi.vrt()
    buf = np.zeros(64, np.uint32)
    p = buf.ctypes.data
    for n in (0, 1, 4):
        assert lib.vrt_get_voxels(None, p, n, p) == -1
        assert lib.vrt_get_voxels_device(None, p, n, p) == -1
        assert lib.vrt_column_tops(None, p, n, p) == -1
        assert lib.vrt_column_tops_device(None, p, n, p) == -1
    assert lib.vrt_get_voxels(None, None, 1, None) == -1
    assert lib.vrt_column_tops(None, None, 1, None) == -1
    for flags in (0, 2, 1, 7):
        assert lib.vrt_read_top_map(None, flags, p) == -1
        assert lib.vrt_top_map_device(None, flags, p) == -1
    assert lib.vrt_read_top_map(None, 0, None) == -1
    assert lib.vrt_top_map_device(None, 0, None) == -1
    assert not buf.any()

"""ctypes bindings of the two in-tree native libraries.

* ``libvrt.so``       — include/vrt.h: the HIP backend (kernels + C ABI), the drop-in for the reference's
                        ``GpuResources``/``Buffers``/``PixelShader`` seam (clientdesktop/src/graphics).
* ``libvrt_host.so``  — include/vrt_host.h: the C++ host mirror of the reference's world / camera types.

Both are REQUIRED: there is no Python or CPU fallback.  A missing library raises ``ImportError`` with the
build command, so a GPU box can never silently run something else.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


class Material(C.Structure):
    """clientdesktop/src/graphics/mod.rs:20-28"""
    _fields_ = [("color", C.c_float * 3), ("is_empty", C.c_uint32), ("is_liquid", C.c_uint32),
                ("scatter", C.c_float), ("_padding", C.c_uint32 * 2)]


class CamData(C.Structure):
    """clientdesktop/src/graphics/mod.rs:82-91"""
    _fields_ = [("pos", C.c_float * 3), ("_padding0", C.c_uint32), ("inv_view_mat", C.c_float * 16),
                ("inv_proj_mat", C.c_float * 16), ("proj_size", C.c_float * 2), ("_padding1", C.c_uint32 * 2)]


class WorldData(C.Structure):
    """clientdesktop/src/graphics/mod.rs:113-120"""
    _fields_ = [("min", C.c_int32 * 3), ("size", C.c_uint32), ("size_in_chunks", C.c_uint32),
                ("_padding", C.c_uint32 * 3)]


class Settings(C.Structure):
    """clientdesktop/src/graphics/mod.rs:132-143"""
    _fields_ = [("max_ray_bounces", C.c_uint32), ("sun_intensity", C.c_float), ("show_step_count", C.c_uint32),
                ("_padding0", C.c_uint32), ("sky_color", C.c_float * 3), ("_padding1", C.c_uint32),
                ("sun_pos", C.c_float * 3), ("_padding2", C.c_uint32)]


MAX_DEVICES = 16


class Config(C.Structure):
    _fields_ = [("max_nodes", C.c_uint32), ("world_size_chunks", C.c_uint32), ("width", C.c_uint32),
                ("height", C.c_uint32), ("device", C.c_int32), ("shard_rank", C.c_uint32),
                ("shard_count", C.c_uint32), ("flags", C.c_uint32), ("shard_root_weight", C.c_uint32),
                ("n_devices", C.c_uint32), ("device_ids", C.c_int32 * MAX_DEVICES)]


class RenderOpts(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("variant", C.c_uint32), ("stats", C.c_uint32), ("spp", C.c_uint32),
                ("seed", C.c_uint32), ("flags", C.c_uint32), ("_reserved", C.c_uint32 * 2)]


class Stats(C.Structure):
    _fields_ = [("primary_rays", C.c_uint64), ("secondary_rays", C.c_uint64), ("hits", C.c_uint64),
                ("steps", C.c_uint64), ("node_visits", C.c_uint64), ("primary_steps", C.c_uint64),
                ("primary_node_visits", C.c_uint64), ("ms_total", C.c_float), ("ms_primary", C.c_float),
                ("ms_secondary", C.c_float), ("frames", C.c_uint32), ("sum_ms_primary", C.c_double),
                ("sum_ms_secondary", C.c_double), ("sum_ms_total", C.c_double),
                ("clock_shader_ticks", C.c_uint64), ("clock_ref_ticks", C.c_uint64)]


class Crosshair(C.Structure):
    """clientdesktop/src/graphics/mod.rs:63-80"""
    _fields_ = [("color", C.c_float * 4), ("style", C.c_uint32), ("size", C.c_float), ("_padding", C.c_uint32 * 2)]


class AccelInfo(C.Structure):
    _fields_ = [("available", C.c_uint32), ("world_size_chunks", C.c_uint32), ("cells", C.c_uint64),
                ("bricks", C.c_uint64), ("bytes", C.c_uint64), ("builds", C.c_uint32), ("last_build_ms", C.c_float),
                ("chunk_builds", C.c_uint32), ("ordered_frames", C.c_uint32)]


class IssueProfile(C.Structure):
    _fields_ = [("frames", C.c_uint32), ("devices", C.c_uint32), ("issuing_threads", C.c_uint32), ("_reserved", C.c_uint32),
                ("render_us", C.c_double), ("root_issue_us", C.c_double), ("shard_issue_us_mean", C.c_double), ("shard_issue_us_max", C.c_double),
                ("join_wait_us", C.c_double), ("tail_us", C.c_double), ("message_waits_us", C.c_double)]


class DenoiseOpts(C.Structure):
    """include/vrt.h vrt_denoise_opts: the path trace's a-trous filter (vrt_set_denoise)"""
    _fields_ = [("passes", C.c_uint32), ("sigma_color", C.c_float), ("flags", C.c_uint32), ("_reserved", C.c_uint32)]


class ToneMap(C.Structure):
    """include/vrt.h vrt_tone_map: exposure and tone curve of presented path frames (vrt_set_tone_map)"""
    _fields_ = [("curve", C.c_uint32), ("flags", C.c_uint32), ("exposure", C.c_float), ("white", C.c_float), ("key", C.c_float),
                ("adapt", C.c_float), ("min_auto", C.c_float), ("max_auto", C.c_float), ("percentile", C.c_uint32),
                ("_reserved", C.c_uint32 * 3)]


class ToneInfo(C.Structure):
    """include/vrt.h vrt_tone_info (vrt_get_tone_info)"""
    _fields_ = [("exposure", C.c_float), ("target", C.c_float), ("luminance", C.c_float), ("bin", C.c_uint32),
                ("counted", C.c_uint64), ("skipped", C.c_uint64), ("frames", C.c_uint32), ("_reserved", C.c_uint32)]


TONE_OFF, TONE_LINEAR, TONE_REINHARD, TONE_FILMIC = 0, 1, 2, 3   # vrt_tone_map.curve (VRT_TONE_*)
TONE_AUTO, TONE_GAMMA2 = 1, 2                                    # vrt_tone_map.flags
TONE_KEY, TONE_PERCENTILE = 0.18, 500                            # the suggested metering


class SunLight(C.Structure):
    """include/vrt.h vrt_sun_light: the path trace's direct sunlight (vrt_set_sun_light)"""
    _fields_ = [("strength", C.c_float), ("flags", C.c_uint32), ("_reserved", C.c_uint32 * 2)]


class WaterOptics(C.Structure):
    """include/vrt.h vrt_water_optics: the path trace's water (vrt_set_water_optics)"""
    _fields_ = [("absorb", C.c_float * 3), ("reflectance", C.c_float), ("flags", C.c_uint32), ("_reserved", C.c_uint32 * 3)]


WATER_ON = 1   # vrt_water_optics.flags (VRT_WATER_ON)


class Haze(C.Structure):
    """include/vrt.h vrt_haze: air that scatters light in the path trace (vrt_set_haze)"""
    _fields_ = [("density", C.c_float), ("albedo", C.c_float * 3), ("flags", C.c_uint32), ("_reserved", C.c_uint32 * 3)]


class WaterRefraction(C.Structure):
    """include/vrt.h vrt_water_refraction: Snell's law at the water's surface, the surface from below (vrt_set_water_refraction)"""
    _fields_ = [("ior", C.c_float), ("max_span", C.c_uint32), ("flags", C.c_uint32), ("_reserved", C.c_uint32)]


class WaterSpan(C.Structure):
    """include/vrt_host.h vrth_water_span: what vrth_world_water_span's walk found"""
    _fields_ = [("dist", C.c_float), ("prev", C.c_int32 * 3), ("m", C.c_int32 * 3), ("v", C.c_uint32), ("event", C.c_uint32), ("steps", C.c_uint32)]


REFRACT_ENTERED, REFRACT_TOTAL, REFRACT_MIRRORED, REFRACT_LEFT = 0, 1, 2, 3   # vrth_water_refract's branches (VRTH_REFRACT_*)


class CameraSampling(C.Structure):
    """include/vrt.h vrt_camera_sampling: the path trace's pixel jitter and thin lens (vrt_set_camera_sampling)"""
    _fields_ = [("pixel_spread", C.c_float), ("aperture", C.c_float), ("focus_distance", C.c_float), ("flags", C.c_uint32)]


class LampLight(C.Structure):
    """include/vrt.h vrt_lamp_light: the path trace's lamp light (vrt_set_lamp_light)"""
    _fields_ = [("strength", C.c_float), ("max_geometry", C.c_float), ("flags", C.c_uint32), ("_reserved", C.c_uint32)]


class Lamp(C.Structure):
    """include/vrt.h vrt_lamp: an entry of the lamp list (vrt_read_lamps)"""
    _fields_ = [("pos", C.c_uint16 * 3), ("voxel", C.c_uint16), ("face", C.c_uint32), ("_reserved", C.c_uint32)]


class LampInfo(C.Structure):
    """include/vrt.h vrt_lamp_info (vrt_get_lamp_info)"""
    _fields_ = [("listed", C.c_uint32), ("cap", C.c_uint32), ("faces", C.c_uint64), ("builds", C.c_uint32), ("last_build_ms", C.c_float)]


LAMP_DTYPE = np.dtype([("pos", "<u2", (3,)), ("voxel", "<u2"), ("face", "<u4"), ("_reserved", "<u4")])


class RayQuery(C.Structure):
    """include/vrt.h vrt_ray_query: common::math::cast_ray's arguments (common/src/math.rs:153-158)"""
    _fields_ = [("start", C.c_float * 3), ("max_dist", C.c_float), ("dir", C.c_float * 3), ("_reserved", C.c_uint32)]


class RayHit(C.Structure):
    """include/vrt.h vrt_ray_hit: Option<HitResult> (math.rs:148-152) plus the DDA's dist and a status"""
    _fields_ = [("pos", C.c_int32 * 3), ("face", C.c_int32 * 3), ("dist", C.c_float), ("status", C.c_uint32)]


class BoxQuery(C.Structure):
    """include/vrt.h vrt_box_query: clip_aabb_movement's arguments (client/src/player.rs:202-207)"""
    _fields_ = [("from_", C.c_float * 3), ("flags", C.c_uint32), ("to", C.c_float * 3), ("_r0", C.c_uint32),
                ("mv", C.c_float * 3), ("_r1", C.c_uint32)]


class BoxMove(C.Structure):
    """include/vrt.h vrt_box_move: mv_clipped plus a status, what was clipped and how many boxes each pass gathered"""
    _fields_ = [("mv", C.c_float * 3), ("status", C.c_uint32), ("flags", C.c_uint32), ("boxes", C.c_uint32 * 2),
                ("_reserved", C.c_uint32)]


class VoxelAt(C.Structure):
    """include/vrt.h vrt_voxel_at: ClientWorld::get_voxel's Result (world.rs:352-357), the voxel or the SetVoxelErr's number"""
    _fields_ = [("voxel", C.c_uint16), ("status", C.c_uint16)]


class ColumnQuery(C.Structure):
    """include/vrt.h vrt_column_query: highest_vox_at's column (world.rs:359-366), where to start and what counts"""
    _fields_ = [("x", C.c_int32), ("z", C.c_int32), ("from_y", C.c_int32), ("flags", C.c_uint32)]


class ColumnTop(C.Structure):
    """include/vrt.h vrt_column_top: the highest voxel of a column that counts"""
    _fields_ = [("y", C.c_int32), ("voxel", C.c_uint32), ("status", C.c_uint32), ("_reserved", C.c_uint32)]


class TopEntry(C.Structure):
    """include/vrt.h vrt_top_entry: one column of vrt_read_top_map"""
    _fields_ = [("y", C.c_int32), ("voxel", C.c_uint32)]


VOXEL_OK, VOXEL_OUT_OF_BOUNDS, VOXEL_NO_CHUNK = 0, 1, 3    # vrt_voxel_at.status (SetVoxelErr's numbers)
COLUMN_FROM_Y, COLUMN_SOLID = 1, 2                          # vrt_column_query.flags
COLUMN_NONE, COLUMN_FOUND, COLUMN_OUTSIDE = 0, 1, 2         # vrt_column_top.status
# the same records as numpy structured dtypes (4, 16, 16 and 8 bytes)
VOXEL_AT_DTYPE = np.dtype([("voxel", "<u2"), ("status", "<u2")])
COLUMN_QUERY_DTYPE = np.dtype([("x", "<i4"), ("z", "<i4"), ("from_y", "<i4"), ("flags", "<u4")])
COLUMN_TOP_DTYPE = np.dtype([("y", "<i4"), ("voxel", "<u4"), ("status", "<u4"), ("_reserved", "<u4")])
TOP_ENTRY_DTYPE = np.dtype([("y", "<i4"), ("voxel", "<u4")])
assert C.sizeof(VoxelAt) == 4 and C.sizeof(ColumnQuery) == 16 and C.sizeof(ColumnTop) == 16 and C.sizeof(TopEntry) == 8
assert (VOXEL_AT_DTYPE.itemsize, COLUMN_QUERY_DTYPE.itemsize, COLUMN_TOP_DTYPE.itemsize, TOP_ENTRY_DTYPE.itemsize) == (4, 16, 16, 8)


class Shape(C.Structure):
    """include/vrt.h vrt_shape: one call of the server's BuiltFeature (server/src/world/gen.rs:312-354)"""
    _fields_ = [("kind", C.c_uint32), ("voxel", C.c_uint32), ("a", C.c_int32 * 3), ("b", C.c_int32 * 3), ("r", C.c_float),
                ("height", C.c_uint32)]


SHAPE_POINT, SHAPE_LINE, SHAPE_SPHERE, SHAPE_DISC = 0, 1, 2, 3   # vrt_shape.kind (VRT_SHAPE_*)
SHAPE_DTYPE = np.dtype([("kind", "<u4"), ("voxel", "<u4"), ("a", "<i4", 3), ("b", "<i4", 3), ("r", "<f4"), ("height", "<u4")])
assert C.sizeof(Shape) == 40 and SHAPE_DTYPE.itemsize == 40

RAY_MISS, RAY_HIT, RAY_REJECTED = 0, 1, 2
BOX_AUTOJUMP, BOX_MAX_VOXELS = 1, 4096                      # vrt_box_query.flags, the cap on the first gather's range
BOX_MOVED, BOX_REJECTED = 0, 2                              # vrt_box_move.status
BOX_CLIPPED_X, BOX_CLIPPED_Y, BOX_CLIPPED_Z, BOX_STEPPED_UP = 1, 2, 4, 8   # vrt_box_move.flags
# the same records as numpy structured dtypes (32 bytes each)
RAY_QUERY_DTYPE = np.dtype([("start", "<f4", 3), ("max_dist", "<f4"), ("dir", "<f4", 3), ("_reserved", "<u4")])
RAY_HIT_DTYPE = np.dtype([("pos", "<i4", 3), ("face", "<i4", 3), ("dist", "<f4"), ("status", "<u4")])
# ... and the box records (48 and 32 bytes)
BOX_QUERY_DTYPE = np.dtype([("from", "<f4", 3), ("flags", "<u4"), ("to", "<f4", 3), ("_r0", "<u4"), ("mv", "<f4", 3), ("_r1", "<u4")])
BOX_MOVE_DTYPE = np.dtype([("mv", "<f4", 3), ("status", "<u4"), ("flags", "<u4"), ("boxes", "<u4", 2), ("_reserved", "<u4")])
# include/vrt.h vrt_polish: one entry of vrt_write_polish's table (32 bytes)
POLISH_DTYPE = np.dtype([("color", "<f4", 3), ("chance", "<f4"), ("scatter", "<f4"), ("_reserved", "<u4", 3)])
# include/vrt.h vrt_translucency: one entry of vrt_write_translucency's table (16 bytes)
TRANSLUCENCY_DTYPE = np.dtype([("color", "<f4", 3), ("chance", "<f4")])


assert C.sizeof(Material) == 32 and C.sizeof(CamData) == 160
assert C.sizeof(RayQuery) == 32 and C.sizeof(RayHit) == 32
assert RAY_QUERY_DTYPE.itemsize == 32 and RAY_HIT_DTYPE.itemsize == 32
assert C.sizeof(BoxQuery) == 48 and C.sizeof(BoxMove) == 32
assert BOX_QUERY_DTYPE.itemsize == 48 and BOX_MOVE_DTYPE.itemsize == 32
assert C.sizeof(WorldData) == 32 and C.sizeof(Settings) == 48
assert C.sizeof(DenoiseOpts) == 16
assert C.sizeof(ToneMap) == 48 and C.sizeof(ToneInfo) == 40
assert C.sizeof(SunLight) == 16
assert C.sizeof(LampLight) == 16 and C.sizeof(Lamp) == 16 and LAMP_DTYPE.itemsize == 16 and C.sizeof(LampInfo) == 24
assert C.sizeof(CameraSampling) == 16
assert POLISH_DTYPE.itemsize == 32
assert TRANSLUCENCY_DTYPE.itemsize == 16

MODE_PRIMARY, MODE_PRIMARY_SHADOW, MODE_PATH = 0, 1, 2
RENDER_OWN_STREAMS, RENDER_TIMED, RENDER_ACCUMULATE = 1, 2, 4   # vrt_render_opts.flags (VRT_RENDER_*)
# include/vrt.h vrt_status
VRT_OK, VRT_ERR_INVALID_ARG, VRT_ERR_OUT_OF_RANGE, VRT_ERR_DEVICE, VRT_ERR_OOM, VRT_ERR_STATE = 0, -1, -2, -3, -4, -5

ID_VOXEL_MASK = 0x7FFF
ID_HIT, ID_NX, ID_NY, ID_NZ = 1 << 16, 1 << 17, 1 << 18, 1 << 19
ID_WATER, ID_SHADOW_RAY, ID_SHADOWED = 1 << 20, 1 << 21, 1 << 22

# every entry point include/vrt.h declares: (restype, argtypes)
_P = C.c_void_p
VRT_SYMBOLS = {
    "vrt_create": (C.c_int, [C.POINTER(Config), C.POINTER(_P)]),
    "vrt_destroy": (None, [_P]),
    "vrt_last_error": (C.c_char_p, [_P]),
    "vrt_write_nodes": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32]),
    "vrt_write_chunk_roots": (C.c_int, [_P, C.c_uint32, _P, C.c_uint32]),
    "vrt_write_chunk_roots_tagged": (C.c_int, [_P, C.c_uint32, _P, C.c_uint32, C.c_uint64]),
    "vrt_resize_world": (C.c_int, [_P, C.c_uint32]),
    "vrt_write_materials": (C.c_int, [_P, C.c_uint32, _P, C.c_uint32]),
    "vrt_write_emission": (C.c_int, [_P, C.c_uint32, _P, C.c_uint32]),
    "vrt_write_polish": (C.c_int, [_P, C.c_uint32, _P, C.c_uint32]),
    "vrt_write_translucency": (C.c_int, [_P, C.c_uint32, _P, C.c_uint32]),
    "vrt_set_camera": (C.c_int, [_P, C.POINTER(CamData)]),
    "vrt_set_settings": (C.c_int, [_P, C.POINTER(Settings)]),
    "vrt_set_world": (C.c_int, [_P, C.POINTER(WorldData)]),
    "vrt_resize_output": (C.c_int, [_P, C.c_uint32, C.c_uint32]),
    "vrt_render": (C.c_int, [_P, C.POINTER(RenderOpts)]),
    "vrt_set_frames_in_flight": (C.c_int, [_P, C.c_uint32]),
    "vrt_reset_accumulation": (C.c_int, [_P]),
    "vrt_get_accumulation": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "vrt_set_denoise": (C.c_int, [_P, C.POINTER(DenoiseOpts)]),
    "vrt_read_guide": (C.c_int, [_P, _P]),
    "vrt_selftest_denoise": (C.c_int, [C.c_int32, _P, _P, _P, C.c_uint32, C.c_uint32, C.POINTER(DenoiseOpts), _P, _P]),
    "vrt_set_tone_map": (C.c_int, [_P, C.POINTER(ToneMap)]),
    "vrt_get_tone_info": (C.c_int, [_P, C.POINTER(ToneInfo)]),
    "vrt_read_tone_histogram": (C.c_int, [_P, _P]),
    "vrt_set_sun_light": (C.c_int, [_P, C.POINTER(SunLight)]),
    "vrt_set_water_optics": (C.c_int, [_P, C.POINTER(WaterOptics)]),
    "vrt_set_water_refraction": (C.c_int, [_P, C.POINTER(WaterRefraction)]),
    "vrt_set_haze": (C.c_int, [_P, C.POINTER(Haze)]),
    "vrt_set_camera_sampling": (C.c_int, [_P, C.POINTER(CameraSampling)]),
    "vrt_set_lamp_light": (C.c_int, [_P, C.POINTER(LampLight)]),
    "vrt_get_lamp_info": (C.c_int, [_P, C.POINTER(LampInfo)]),
    "vrt_read_lamps": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(C.c_uint32)]),
    "vrt_synchronize": (C.c_int, [_P]),
    "vrt_read_output": (C.c_int, [_P, _P, _P, _P]),
    "vrt_present": (C.c_int, [_P, C.POINTER(Crosshair), C.c_uint32, C.c_uint32, _P]),
    "vrt_selftest_exact_math": (C.c_int, [C.c_int32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
    "vrt_selftest_math_values": (C.c_int, [C.c_int32, C.c_uint32, C.c_uint32, _P, _P]),
    "vrt_present_device": (C.c_int, [_P, C.POINTER(Crosshair), C.c_uint32, C.c_uint32, C.POINTER(_P), C.POINTER(C.c_uint64)]),
    "vrt_set_presentation": (C.c_int, [_P, C.POINTER(Crosshair), C.c_uint32, C.c_uint32, C.c_uint32]),
    "vrt_get_stats": (C.c_int, [_P, C.POINTER(Stats)]),
    "vrt_get_issue_profile": (C.c_int, [_P, C.POINTER(IssueProfile)]),
    "vrt_get_accel_info": (C.c_int, [_P, C.POINTER(AccelInfo)]),
    "vrt_read_accel": (C.c_int, [_P, _P, _P]),
    "vrt_read_march_cells": (C.c_int, [_P, _P, _P]),
    "vrt_get_sun_marks": (C.c_int, [_P, _P, _P, _P, _P]),
    "vrt_read_lit_voxels": (C.c_int, [_P, _P, _P, _P, _P]),
    "vrt_read_dark_voxels": (C.c_int, [_P, _P, _P, _P]),
    "vrt_get_dark_marks": (C.c_int, [_P, _P, _P, _P, _P]),
    "vrt_read_tile_cost": (C.c_int, [_P, _P]),
    "vrt_read_tile_order": (C.c_int, [_P, _P, C.POINTER(C.c_uint32)]),
    "vrt_selftest_tile_order": (C.c_int, [C.c_int32, _P, C.c_uint32, C.c_uint32, C.c_int32, _P]),
    "vrt_read_steps": (C.c_int, [_P, _P]),
    "vrt_set_stream": (C.c_int, [_P, _P]),
    "vrt_bind_output": (C.c_int, [_P, _P]),
    "vrt_device_output": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_uint64)]),
    "vrt_shard_info": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "vrt_assemble": (C.c_int, [_P, _P, C.c_uint64, _P]),
    "vrt_assemble_compact": (C.c_int, [_P, _P, C.c_uint64, _P]),
    "vrt_cast_rays": (C.c_int, [_P, _P, C.c_uint32, _P]),
    "vrt_cast_rays_device": (C.c_int, [_P, _P, C.c_uint32, _P]),
    "vrt_clip_moves": (C.c_int, [_P, _P, C.c_uint32, _P]),
    "vrt_clip_moves_device": (C.c_int, [_P, _P, C.c_uint32, _P]),
    "vrt_get_voxels": (C.c_int, [_P, _P, C.c_uint32, _P]),
    "vrt_get_voxels_device": (C.c_int, [_P, _P, C.c_uint32, _P]),
    "vrt_column_tops": (C.c_int, [_P, _P, C.c_uint32, _P]),
    "vrt_column_tops_device": (C.c_int, [_P, _P, C.c_uint32, _P]),
    "vrt_read_top_map": (C.c_int, [_P, C.c_uint32, _P]),
    "vrt_top_map_device": (C.c_int, [_P, C.c_uint32, _P]),
    "vrt_generate_chunks": (C.c_int, [_P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint64, _P]),
    "vrt_build_chunks": (C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint64, _P]),
    "vrt_edit_chunks": (C.c_int, [_P, _P, C.c_uint32, _P, _P, _P, C.c_uint32, _P, C.c_uint64, _P, _P]),
}


def _load(name: str, symbols: dict) -> C.CDLL:
    path = os.path.join(_HERE, name)
    absent = ()
    if name == "libvrt.so" and os.environ.get("VRT_LIB"):   # development: A/B another build of the backend (tools/ab/)
        path = os.environ["VRT_LIB"]
        # ... which may be an older one: VRT_LIB_WITHOUT names (comma-separated) the entry points it is known not to have yet.
        # Only those may be missing, and only from such a build: the tree's own library answers to the whole header.
        absent = tuple(s for s in os.environ.get("VRT_LIB_WITHOUT", "").split(",") if s)
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing — the native library is the product, there is no fallback. Build it with "
            f"`python -c 'import __graft_entry__ as g; g.build()'` or `make -C voxelraytracing_amd/csrc`.")
    lib = C.CDLL(path)
    for sym, (res, args) in symbols.items():
        if sym in absent and not hasattr(lib, sym):
            continue
        fn = getattr(lib, sym)  # AttributeError if the ABI drifted from the header
        fn.restype = res
        fn.argtypes = args
    return lib


def code_object_sha256(path: str | None = None) -> str:
    """sha256 of the device code (the ELF section .hip_fatbin) of libvrt.so: names the kernels a measurement belongs to
    (bench.py prints PMC-derived figures only next to the build they were collected on)."""
    import hashlib
    import struct
    path = path or os.environ.get("VRT_LIB") or os.path.join(_HERE, "libvrt.so")
    data = open(path, "rb").read()
    if data[:4] != b"\x7fELF" or data[4] != 2:
        return hashlib.sha256(data).hexdigest()
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", data, 0x3A)
    sec = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    names = sec[shstrndx]
    for s in sec:
        name = data[names[4] + s[0]:data.index(b"\0", names[4] + s[0])]
        if name == b".hip_fatbin":
            return hashlib.sha256(data[s[4]:s[4] + s[5]]).hexdigest()
    return hashlib.sha256(data).hexdigest()


def kernel_registers(path: str | None = None) -> dict:
    """{kernel symbol: {"vgprs", "sgprs", "vgpr_spills", "sgpr_spills", "scratch_bytes"}} of the gfx950 kernels in libvrt.so,
    read from the code objects' metadata (llvm-readelf; no GPU).  tests/test_abi.py holds every kernel to no spills and no
    scratch: a bounce kernel that spilled (SGPRs into VGPR lanes, three VGPRs into scratch) faulted on the card in round 3
    while the same source without the spills was bit-exact, so a spill is a build error here, not a slowdown."""
    import re
    import struct
    import subprocess
    import tempfile
    path = path or os.environ.get("VRT_LIB") or os.path.join(_HERE, "libvrt.so")
    data = open(path, "rb").read()
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", data, 0x3A)
    sec = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    names = sec[shstrndx]
    fat = b""
    for s in sec:
        if data[names[4] + s[0]:data.index(b"\0", names[4] + s[0])] == b".hip_fatbin":
            fat = data[s[4]:s[4] + s[5]]
    magic = b"__CLANG_OFFLOAD_BUNDLE__"   # one bundle per translation unit: {count, {offset, size, triple}...}
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    found = {}
    at = fat.find(magic)
    while at >= 0:
        count, = struct.unpack_from("<Q", fat, at + 24)
        q = at + 32
        for _ in range(count):
            off, size, tl = struct.unpack_from("<QQQ", fat, q)
            triple = fat[q + 24:q + 24 + tl].decode()
            q += 24 + tl
            if "gfx950" not in triple or not size:
                continue
            with tempfile.NamedTemporaryFile(suffix=".co") as f:
                f.write(fat[at + off:at + off + size])
                f.flush()
                notes = subprocess.run([readelf, "--notes", f.name], capture_output=True, text=True, check=True).stdout
            for m in re.finditer(r"\.private_segment_fixed_size:\s+(\d+)\s+\.sgpr_count:\s+(\d+)\s+\.sgpr_spill_count:\s+(\d+)\s+"
                                 r"\.symbol:\s+(\S+?)\.kd\s.*?\.vgpr_count:\s+(\d+)\s+\.vgpr_spill_count:\s+(\d+)", notes, re.S):
                found[m.group(4)] = {"scratch_bytes": int(m.group(1)), "sgprs": int(m.group(2)), "sgpr_spills": int(m.group(3)),
                                     "vgprs": int(m.group(5)), "vgpr_spills": int(m.group(6))}
        at = fat.find(magic, at + 24)
    return found


_vrt = None


def vrt() -> C.CDLL:
    """The HIP backend. Loading needs libamdhip64 but no GPU; every compute call needs a GPU."""
    global _vrt
    if _vrt is None:
        # One HIP runtime per process: the torch wheel bundles its own libamdhip64.so.7 / libhsa-runtime64 and
        # fails to initialise ("No HIP GPUs are available") if the system copy was mapped first.  Loading torch's
        # first lets libvrt.so bind to it by SONAME, so torch streams / tensors and vrt_* calls share one runtime
        # (needed by vrt_set_stream and vrt_bind_output).  A C or Rust host simply links /opt/rocm's.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _vrt = _load("libvrt.so", VRT_SYMBOLS)
    return _vrt


_U32P = C.POINTER(C.c_uint32)
_I32P = C.POINTER(C.c_int32)
VRTH_SYMBOLS = {
    "vrth_world_new": (_P, [_I32P, C.c_uint32, C.c_uint32]),
    "vrth_world_free": (None, [_P]),
    "vrth_world_create_chunk": (C.c_int, [_P, _I32P, _P, C.c_uint32, _U32P]),
    "vrth_world_set_voxel": (C.c_int, [_P, _I32P, C.c_uint16, _U32P, _U32P]),
    "vrth_world_get_voxel": (C.c_int, [_P, _I32P, C.POINTER(C.c_uint16)]),
    "vrth_world_center_chunks": (C.c_uint32, [_P, _I32P]),
    "vrth_world_resize": (None, [_P, C.c_uint32]),
    "vrth_world_nodes": (_P, [_P]),
    "vrth_world_max_nodes": (C.c_uint32, [_P]),
    "vrth_world_chunk_roots": (C.c_uint32, [_P, _P, C.c_uint32]),
    "vrth_world_chunk_roots_ptr": (C.c_void_p, [_P]),
    "vrth_world_chunk_roots_generation": (C.c_uint64, [_P]),
    "vrth_world_info": (None, [_P, _I32P, _U32P, _U32P, _U32P]),
    "vrth_world_alloc_status": (None, [_P, _U32P, _U32P]),
    "vrth_world_chunk_state": (C.c_int, [_P, _I32P, _U32P, _U32P, _U32P, _P, C.c_uint32]),
    "vrth_world_highest_vox_at": (C.c_int, [_P, C.c_int32, C.c_int32, _I32P]),
    "vrth_world_data_from": (None, [_P, C.POINTER(WorldData)]),
    "vrth_world_cast_ray": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.POINTER(RayHit)]),
    "vrth_world_cast_rays": (None, [_P, _P, C.c_uint32, _P, C.c_int]),
    "vrth_world_get_collisions": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), _P, _P, C.c_uint32, _U32P]),
    "vrth_world_clip_move": (C.c_int, [_P, _P, C.POINTER(BoxQuery), C.POINTER(BoxMove)]),
    "vrth_world_clip_moves": (None, [_P, _P, _P, C.c_uint32, _P, C.c_int]),
    "vrth_world_get_voxels": (None, [_P, _P, C.c_uint32, _P, C.c_int]),
    "vrth_world_column_top": (C.c_int, [_P, _P, C.POINTER(ColumnQuery), C.POINTER(ColumnTop)]),
    "vrth_world_column_tops": (None, [_P, _P, _P, C.c_uint32, _P, C.c_int]),
    "vrth_world_top_map": (C.c_int, [_P, _P, C.c_uint32, _P, C.c_int]),
    "vrth_world_create_chunks": (C.c_int, [_P, _P, C.c_uint32, _P, _P, _P, C.c_uint32, _U32P]),
    "vrth_cam_data_create": (None, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.POINTER(C.c_float), C.POINTER(CamData)]),
    "vrth_axis_rot_to_ray": (None, [C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "vrth_std_materials": (None, [_P]),
    "vrth_std_voxel_name": (C.c_char_p, [C.c_uint32]),
    "vrth_svo_build_by_set_node": (C.c_uint32, [_P, _P, C.c_uint32]),
    "vrth_svo_build_bottom_up": (C.c_uint32, [_P, _P, C.c_uint32]),
    "vrth_svo_to_dense": (None, [_P, _P]),
    "vrth_gen_height": (C.c_int32, [C.c_uint32, C.c_int32, C.c_int32]),
    "vrth_gen_dense": (C.c_int, [C.c_uint32, _I32P, _P]),
    "vrth_gen_dense_superflat": (None, [_I32P, _P]),
    "vrth_world_generate": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_int]),
    "vrth_world_generate_missing": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_int, _P, C.c_uint32, _U32P]),
    "vrth_apply_shapes": (C.c_int, [_P, _I32P, _P, C.c_uint32]),
    "vrth_edit_chunks": (C.c_int, [_P, C.c_uint32, _P, _P, _P, C.c_uint32, _P, C.c_uint64, _P, _P, C.c_int]),
    "vrth_region_load_into_world": (C.c_int, [_P, _P, C.c_uint64, _I32P, _U32P]),
    "vrth_region_save_from_world": (C.c_uint64, [_P, _I32P, _P, C.c_uint64]),
    "vrth_chunk_msg_ingest": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(C.c_uint64), _I32P, _U32P, _U32P]),
    "vrth_chunk_msg_encode": (C.c_uint64, [_P, _I32P, _P, C.c_uint64]),
    "vrth_region_of_chunk": (None, [_I32P, _I32P, _U32P]),
    "vrth_region_file_name": (C.c_uint32, [_I32P, C.c_char_p, C.c_uint32]),
    "vrth_denoise": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, C.POINTER(DenoiseOpts), _P]),
    "vrth_lens_ray": (C.c_int, [_P, _I32P, C.POINTER(CameraSampling), C.c_uint32, C.c_uint32, _P, _P]),
    "vrth_tone_meter": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(ToneMap), C.c_int, C.c_float, C.POINTER(ToneInfo), _P]),
    "vrth_tone_map": (C.c_int, [_P, C.c_uint64, C.POINTER(ToneMap), C.c_float, _P]),
    "vrth_water_transmittance": (C.c_int, [_P, _P, C.c_uint64, _P]),
    "vrth_water_refract": (C.c_int, [C.c_float, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_int, C.POINTER(C.c_float)]),
    "vrth_world_water_span": (C.c_int, [_P, _P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32, C.POINTER(WaterSpan)]),
    "vrth_haze_distance": (C.c_int, [_P, C.c_uint64, C.c_float, _P]),
    "vrth_haze_exit": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.POINTER(C.c_float)]),
}

# Gpu.set_denoise's suggested setting (docs/KERNELS.md: the sweep they come from)
DENOISE_PASSES, DENOISE_SIGMA_COLOR = 5, 0.0

_host = None


def host() -> C.CDLL:
    """The C++ host mirror (ClientWorld, CamData::create, world generator). CPU only."""
    global _host
    if _host is None:
        _host = _load("libvrt_host.so", VRTH_SYMBOLS)
    return _host


def denoise(rgb, ids, guide, passes: int = DENOISE_PASSES, sigma_color: float = DENOISE_SIGMA_COLOR) -> np.ndarray:
    """vrth_denoise: the filter a denoised path frame goes through on the GPU (vrt_set_denoise), on the host, in the same text —
    rgb [h, w, 3] f32, ids and guide [h, w] u32 (Gpu.read_output, Gpu.read_guide) -> the filtered [h, w, 3] f32."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    h, w = rgb.shape[:2]
    ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(h, w)
    guide = np.ascontiguousarray(guide, dtype=np.uint32).reshape(h, w)
    out = np.empty_like(rgb)
    o = DenoiseOpts(passes, sigma_color, 0, 0)
    if host().vrth_denoise(rgb.ctypes.data, ids.ctypes.data, guide.ctypes.data, w, h, C.byref(o), out.ctypes.data):
        raise ValueError(f"denoise: passes {passes} (0..5), sigma_color {sigma_color} (finite, >= 0)")
    return out


def selftest_denoise(rgb, ids, guide, passes: int, sigma_color: float, device: int = 0):
    """vrt_selftest_denoise: the pass kernels of vrt_set_denoise on a frame of the caller's choosing, through the launcher a frame
    uses (include/vrt.h).  Arguments as denoise() above -> (the filtered rgb [h, w, 3] f32, the id words [h, w] u32 the last pass
    wrote).  A refused call raises VrtError."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    h, w = rgb.shape[:2]
    ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(h, w)
    guide = np.ascontiguousarray(guide, dtype=np.uint32).reshape(h, w)
    out, ids_out = np.empty_like(rgb), np.empty_like(ids)
    o = DenoiseOpts(passes, sigma_color, 0, 0)
    rc = vrt().vrt_selftest_denoise(device, rgb.ctypes.data, ids.ctypes.data, guide.ctypes.data, w, h, C.byref(o), out.ctypes.data, ids_out.ctypes.data)
    if rc:
        from .graphics import VrtError
        raise VrtError(rc, f"vrt_selftest_denoise refused {w} x {h}, passes {passes}, sigma_color {sigma_color}")
    return out, ids_out


def tone_setting(curve: int = TONE_FILMIC, exposure: float = 1.0, auto: bool = False, gamma2: bool = False, white: float = 0.0,
                 key: float = TONE_KEY, adapt: float = 1.0, min_auto: float = 0.0, max_auto: float = 0.0,
                 percentile: int = TONE_PERCENTILE) -> ToneMap:
    """A vrt_tone_map from keywords (Gpu.set_tone_map takes the same ones)."""
    return ToneMap(curve, (TONE_AUTO if auto else 0) | (TONE_GAMMA2 if gamma2 else 0), exposure, white, key, adapt, min_auto, max_auto,
                   percentile, (C.c_uint32 * 3)(0, 0, 0))


def tone_meter(rgb, opts: ToneMap, prev_exposure=None):
    """vrth_tone_meter: what a metered frame's kernels compute (vrt_set_tone_map with VRT_TONE_AUTO), on the host, in the same
    text — rgb [h, w, 3] f32 -> (ToneInfo, bins [256] u32); prev_exposure: the adapted exposure of the metered frame before
    (None: the adaptation starts here)."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    h, w = rgb.shape[:2]
    info, bins = ToneInfo(), np.zeros(256, dtype=np.uint32)
    if host().vrth_tone_meter(rgb.ctypes.data, w, h, C.byref(opts), 0 if prev_exposure is None else 1,
                              0.0 if prev_exposure is None else float(prev_exposure), C.byref(info), bins.ctypes.data):
        raise ValueError("tone_meter: a setting vrt_set_tone_map refuses")
    return info, bins


def tone_map(rgb, opts: ToneMap, exposure: float) -> np.ndarray:
    """vrth_tone_map: encode(curve(c * E)) of every value of rgb (f32, any shape), in the text the mapped blit compiles."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    out = np.empty_like(rgb)
    if host().vrth_tone_map(rgb.ctypes.data, rgb.size, C.byref(opts), float(exposure), out.ctypes.data):
        raise ValueError("tone_map: a setting vrt_set_tone_map refuses")
    return out


def water_transmittance(absorb, dist) -> np.ndarray:
    """vrth_water_transmittance: vexp_neg(absorb * dist) elementwise (f32, broadcast against each other), in the text the water
    kernels compile (csrc/both/water_math.h) — the factor vrt_set_water_optics puts on a wet segment's throughput."""
    a, d = np.broadcast_arrays(np.asarray(absorb, dtype=np.float32), np.asarray(dist, dtype=np.float32))
    a, d = np.ascontiguousarray(a), np.ascontiguousarray(d)
    out = np.empty(a.shape, dtype=np.float32)
    if host().vrth_water_transmittance(a.ctypes.data, d.ctypes.data, a.size, out.ctypes.data):
        raise ValueError("vrth_water_transmittance refused the arguments")
    return out


def haze_distance(u, inv: float) -> np.ndarray:
    """vrth_haze_distance: (-vlog(max(u, 1e-10))) * inv elementwise (f32), in the text the haze kernels compile
    (csrc/both/haze_math.h) — how far vrt_set_haze's draw u reaches; inv = 1.0f / density."""
    u = np.ascontiguousarray(np.asarray(u, dtype=np.float32))
    out = np.empty(u.shape, dtype=np.float32)
    if host().vrth_haze_distance(u.ctypes.data, u.size, float(inv), out.ctypes.data):
        raise ValueError("vrth_haze_distance refused the arguments")
    return out


def haze_exit(o, d, world_max: float) -> np.float32:
    """vrth_haze_exit: where the ray from o (world-local) along d leaves the box (0, world_max)^3 — the length in the haze of a
    segment that hits nothing; 0 for an origin on or beyond a face, or a NaN."""
    f3 = C.c_float * 3
    out = C.c_float()
    if host().vrth_haze_exit(f3(*(float(np.float32(x)) for x in o)), f3(*(float(np.float32(x)) for x in d)), float(np.float32(world_max)), C.byref(out)):
        raise ValueError("vrth_haze_exit refused the arguments")
    return np.float32(out.value)


def water_refract(ior: float, reflectance: float, d, normal, u: float = 0.0, leaving: bool = False):
    """vrth_water_refract: (d' [3] f32, the branch: REFRACT_*) of vrt_set_water_refraction's bend into the water (leaving False: A of
    the contract) or of the underside event (leaving True: C; normal points back into the water, u is the event's draw)."""
    f3 = C.c_float * 3
    out = f3()
    branch = host().vrth_water_refract(ior, reflectance, f3(*(float(x) for x in d)), f3(*(float(x) for x in normal)), u, 1 if leaving else 0, out)
    if branch < 0:
        raise ValueError("vrth_water_refract refused the arguments")
    return np.array(out[:], dtype=np.float32), branch


def world_water_span(world_handle, materials, o, d, max_span: int = 0) -> WaterSpan:
    """vrth_world_water_span: the span walk (B of vrt_set_water_refraction's contract) over a host world from o (world-local)
    along d.  materials: the 256-entry table (a ctypes array of Material)."""
    f3 = C.c_float * 3
    out = WaterSpan()
    if host().vrth_world_water_span(world_handle, C.addressof(materials), f3(*(float(x) for x in o)), f3(*(float(x) for x in d)), max_span, C.byref(out)):
        raise ValueError("vrth_world_water_span refused the arguments")
    return out

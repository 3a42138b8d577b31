"""GPU boundary — Python handles on libvrt.so, named after the reference's seam types.

    Gpu / GpuResources / Buffers / NodeBuffer / PixelShader  <- clientdesktop/src/graphics/{mod.rs,shader.rs}
    CamData.create, Settings, Material, WorldData            <- clientdesktop/src/graphics/mod.rs:20-143

The frame loop of main.rs:426-453 maps call for call.  There is no CPU path: every
method ends in a vrt_* call of the HIP backend and raises ``VrtError`` if that fails.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _ffi
from ._ffi import (CamData, Material, Settings, WorldData, Stats, RenderOpts,  # noqa: F401  (re-exported)
                   MODE_PRIMARY, MODE_PRIMARY_SHADOW, MODE_PATH, RENDER_OWN_STREAMS, RENDER_TIMED, RENDER_ACCUMULATE)


class VrtError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"vrt error {code}: {msg}")
        self.code = code


def _f(vals, n):
    return (C.c_float * n)(*[float(v) for v in vals])


_scratch3a, _scratch3b, _scratch2 = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 2)()


def cam_data_create(rot_deg, eye, fov_deg: float, proj_size) -> CamData:
    """CamData::create(cam, eye, fov, proj_size) — mod.rs:92-111 (rot and fov in degrees)."""
    out = CamData()
    _scratch3a[0], _scratch3a[1], _scratch3a[2] = rot_deg      # (per-frame call of the frame loop: no allocations here)
    _scratch3b[0], _scratch3b[1], _scratch3b[2] = eye
    _scratch2[0], _scratch2[1] = proj_size
    _ffi.host().vrth_cam_data_create(_scratch3a, _scratch3b, fov_deg, _scratch2, C.byref(out))
    return out


def axis_rot_to_ray(rot_rad):
    """common/src/math.rs:131-146"""
    out = (C.c_float * 3)()
    _ffi.host().vrth_axis_rot_to_ray(_f(rot_rad, 3), out)
    return tuple(out)


def make_settings(max_ray_bounces=3, sun_intensity=4.0, show_step_count=0, sky_color=(0.81, 0.93, 1.0),
                  sun_pos=(0.0, 0.0, 0.0)) -> Settings:
    """Defaults are AppState::new's (clientdesktop/src/main.rs:152-156; sun_pos left at the origin there)."""
    s = Settings()
    s.max_ray_bounces, s.sun_intensity, s.show_step_count = max_ray_bounces, sun_intensity, show_step_count
    s.sky_color[:] = sky_color
    s.sun_pos[:] = sun_pos
    return s


def std_materials():
    """Material::construct_arr over the standard data pack (mod.rs:38-60): (Material*256) array."""
    arr = (Material * 256)()
    _ffi.host().vrth_std_materials(arr)
    return arr


def selftest_tile_order(cost, tiles_x: int, tiles_y: int, radius: int, device: int = 0) -> np.ndarray:
    """order[tiles_x * tiles_y] the tile-order kernels make of cost (radius < 0: the exact order, 1..6: the dilated block order) —
    see vrt_selftest_tile_order in include/vrt.h.  Entries nothing wrote are 0xFFFFFFFF; a refused call raises and writes nothing."""
    cost = np.ascontiguousarray(cost, dtype=np.uint32).reshape(-1)
    if cost.size != tiles_x * tiles_y:
        raise ValueError(f"{cost.size} costs for {tiles_x} x {tiles_y} tiles")
    order = np.full(cost.size, 0xFFFFFFFF, dtype=np.uint32)
    lib = _ffi.vrt()
    rc = lib.vrt_selftest_tile_order(device, cost.ctypes.data_as(C.c_void_p), tiles_x, tiles_y, radius, order.ctypes.data_as(C.c_void_p))
    if rc:
        raise VrtError(rc, "vrt_selftest_tile_order refused the call")
    return order


# vrt_selftest_math_values' ops (include/vrt.h VRT_MATH_*): name -> (op, input words, output words per operand set)
MATH_OPS = {name: (op, n_in, n_out) for op, (name, n_in, n_out) in enumerate([
    ("div", 2, 1), ("sqrt", 1, 1), ("unit_steps", 3, 4), ("normalize", 3, 4), ("lens_div", 2, 2), ("lens_sqrt", 1, 2),
    ("rng_next", 1, 2), ("rng_next_u2", 1, 2), ("log_banded", 1, 1), ("log_general", 1, 1), ("cos2pi", 1, 1), ("rng_dir", 1, 5),
    ("trunc2i", 1, 1), ("flr2i", 1, 1), ("abs_mul", 2, 1), ("min3_f32", 3, 1), ("min3_bits", 3, 1), ("bfi", 3, 1),
    ("low_bits", 2, 4), ("or_and", 3, 1), ("mad_i24", 3, 1), ("exp_neg", 2, 1)])}


def selftest_math_values(op: str, *words, device: int = 0) -> np.ndarray:
    """out[output words, n] (uint32 bit patterns) of the kernels' exact-arithmetic function `op` (a key of MATH_OPS) over n operand
    sets, one array of n 32-bit words (uint32, int32 or float32: taken by their bits) per input word — see vrt_selftest_math_values
    in include/vrt.h.  Set i runs on lane i % 64 of wave i / 64: the caller composes whole waves.  A refused call raises."""
    code, n_in, n_out = MATH_OPS[op]
    if len(words) != n_in:
        raise ValueError(f"{op} takes {n_in} input words, not {len(words)}")
    planes = []
    for w in words:
        w = np.ascontiguousarray(w).reshape(-1)
        if w.dtype.itemsize != 4:
            raise ValueError(f"{op}: 32-bit words, not {w.dtype}")
        planes.append(w.view(np.uint32))
    src = np.ascontiguousarray(np.stack(planes))
    n = src.shape[1]
    out = np.zeros((n_out, n), dtype=np.uint32)
    rc = _ffi.vrt().vrt_selftest_math_values(device, code, n, src.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    if rc:
        raise VrtError(rc, "vrt_selftest_math_values refused the call")
    return out


class Gpu:
    """Owns one backend context; stands where the reference passes `&Gpu` (mod.rs:227-304).

    Arguments are GpuResources::new's (mod.rs:155-161) plus the tile shard of this process."""

    def __init__(self, max_nodes: int, world_size: int, result_size, device: int = -1,
                 shard_rank: int = 0, shard_count: int = 1, tile_major: bool = False, root_weight: int = 1,
                 row_major: bool = False, compact: bool = False, devices=None, texel_messages: bool = False,
                 staged_messages: bool = False, poison_messages: bool = False):
        """devices: a list of HIP device ordinals makes this ONE context over several devices (vrt_config.device_ids)."""
        self._lib = _ffi.vrt()
        cfg = _ffi.Config(max_nodes, world_size, result_size[0], result_size[1], device, shard_rank, shard_count,
                          (1 if tile_major else 0) | (2 if row_major else 0) | (4 if compact else 0) | (8 if texel_messages else 0) |
                          (16 if staged_messages else 0) | (32 if poison_messages else 0),
                          root_weight)
        if devices:
            cfg.n_devices = len(devices)
            for i, d in enumerate(devices):
                cfg.device_ids[i] = d
        h = C.c_void_p()
        rc = self._lib.vrt_create(C.byref(cfg), C.byref(h))
        if rc:
            raise VrtError(rc, self._lib.vrt_last_error(None).decode())
        self._h = h
        self.result_size = (result_size[0], result_size[1])
        self.shard_rank, self.shard_count = shard_rank, shard_count
        self._roots_size = int(world_size)   # the chunk_roots buffer holds _roots_size^3 entries: no world is larger (validate_frame)
        self._world_size = 0                 # vrt_world_data.size_in_chunks as last written

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vrt_destroy(self._h)
            self._h = None

    __del__ = close

    def _ck(self, rc: int):
        if rc:
            raise VrtError(rc, self._lib.vrt_last_error(self._h).decode())

    # --- Buffers (shader.rs:43-143) ---
    def write_nodes(self, pool, start: int, end: int):
        """NodeBuffer::write(gpu, src_nodes, start..end) — shader.rs:22-40. pool: u16 array or address of node 0."""
        ptr = pool if isinstance(pool, int) else pool.ctypes.data
        self._ck(self._lib.vrt_write_nodes(self._h, C.c_void_p(ptr), start, end))

    def write_chunk_roots(self, roots: np.ndarray, offset: int = 0, tag: int = 0):
        """ArrayBuffer::write (shader.rs:133-142).  tag: vrt_write_chunk_roots_tagged — e.g. ClientWorld.roots_generation()."""
        roots = np.ascontiguousarray(roots, dtype=np.uint32)
        self._ck(self._lib.vrt_write_chunk_roots_tagged(self._h, offset, roots.ctypes.data, roots.size, tag))

    def resize_chunk_buffer(self, world_size: int):
        self._ck(self._lib.vrt_resize_world(self._h, world_size))
        self._roots_size = int(world_size)

    def write_materials(self, mats, first: int = 0, n: Optional[int] = None):
        n = len(mats) if n is None else n
        self._ck(self._lib.vrt_write_materials(self._h, first, C.cast(mats, C.c_void_p), n))

    def write_emission(self, values, first: int = 0):
        """vrt_write_emission: entries [first, first + len(values)) of the per-material emission table (MODE_PATH only; all 0
        until written).  values: a sequence of floats or a float32 array; a negative, NaN or infinite entry, or first +
        len(values) > 256, raises VrtError and writes nothing."""
        v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
        self._ck(self._lib.vrt_write_emission(self._h, first, v.ctypes.data if v.size else None, v.size))

    def write_polish(self, entries, first: int = 0):
        """vrt_write_polish: entries [first, first + len(entries)) of the per-material polish table, the path trace's second,
        specular lobe (MODE_PATH only; all 0 until written).  entries: an array of _ffi.POLISH_DTYPE (color, chance, scatter);
        a negative, NaN or infinite float, or first + len(entries) > 256, raises VrtError and writes nothing."""
        e = np.ascontiguousarray(entries, dtype=_ffi.POLISH_DTYPE).reshape(-1)
        self._ck(self._lib.vrt_write_polish(self._h, first, e.ctypes.data if e.size else None, e.size))

    def write_translucency(self, entries, first: int = 0):
        """vrt_write_translucency: entries [first, first + len(entries)) of the per-material translucency table, the path
        trace's pass-through lobe (MODE_PATH only; all 0 until written).  entries: an array of _ffi.TRANSLUCENCY_DTYPE (color,
        chance); a negative, NaN or infinite float, or first + len(entries) > 256, raises VrtError and writes nothing."""
        e = np.ascontiguousarray(entries, dtype=_ffi.TRANSLUCENCY_DTYPE).reshape(-1)
        self._ck(self._lib.vrt_write_translucency(self._h, first, e.ctypes.data if e.size else None, e.size))

    def write_cam_data(self, cam: CamData):
        self._ck(self._lib.vrt_set_camera(self._h, C.byref(cam)))

    def write_settings(self, s: Settings):
        self._ck(self._lib.vrt_set_settings(self._h, C.byref(s)))

    def write_world_data(self, w: WorldData):
        self._ck(self._lib.vrt_set_world(self._h, C.byref(w)))
        self._world_size = int(w.size_in_chunks)   # (top_map sizes its array by it)

    def resize_result_texture(self, new_size):
        self._ck(self._lib.vrt_resize_output(self._h, new_size[0], new_size[1]))
        self.result_size = (new_size[0], new_size[1])

    # --- PixelShader (shader.rs:295-380) ---
    def encode_pass(self, mode: int = MODE_PRIMARY, variant: int = 0, stats: bool = False, spp: int = 1, seed: int = 0,
                    own_streams: bool = False, timed: bool = False, accumulate: bool = False):
        """PixelShader::encode_pass + queue.submit (shader.rs:371-379, main.rs:453,565). Asynchronous.
        own_streams: VRT_RENDER_OWN_STREAMS; accumulate: VRT_RENDER_ACCUMULATE, MODE_PATH only — the output is the mean of
        every sample since the accumulation last started again (include/vrt.h)."""
        flags = (RENDER_OWN_STREAMS if own_streams else 0) | (RENDER_TIMED if timed else 0) | (RENDER_ACCUMULATE if accumulate else 0)
        o = RenderOpts(mode, variant, int(stats), spp, seed, flags)   # stats: False/True, or 2 = clock probe
        self._ck(self._lib.vrt_render(self._h, C.byref(o)))

    render = encode_pass

    def set_frames_in_flight(self, n: int):
        """1..4 frames in flight (default 2); see vrt_set_frames_in_flight in include/vrt.h."""
        self._ck(self._lib.vrt_set_frames_in_flight(self._h, n))

    def reset_accumulation(self):
        """The next accumulating frame starts again at sample 0 (vrt_reset_accumulation)."""
        self._ck(self._lib.vrt_reset_accumulation(self._h))

    def accumulation(self):
        """(samples, seed) of the last accumulating frame's mean (vrt_get_accumulation; no synchronisation)."""
        n, seed = C.c_uint32(0), C.c_uint32(0)
        self._ck(self._lib.vrt_get_accumulation(self._h, C.byref(n), C.byref(seed)))
        return n.value, seed.value

    def set_denoise(self, passes: int, sigma_color: float = 0.0):
        """vrt_set_denoise: every later MODE_PATH frame goes through `passes` (1..5; 0 = off) passes of the edge-stopped a-trous
        filter, tap spacing 1, 2, 4, 8, 16 pixels, sigma_color the colour stop of the first pass (halved every pass; 0 = none).
        _ffi.DENOISE_PASSES / DENOISE_SIGMA_COLOR are the suggested setting.  Sharded and multi-device contexts refuse it."""
        o = _ffi.DenoiseOpts(passes, sigma_color, 0, 0)
        self._ck(self._lib.vrt_set_denoise(self._h, C.byref(o)))

    def read_guide(self) -> np.ndarray:
        """vrt_read_guide: the guide words [h, w] of the last denoised frame (the plane coordinate of each filterable pixel's face)."""
        w, h = self.result_size
        a = np.empty((h, w), dtype=np.uint32)
        self._ck(self._lib.vrt_read_guide(self._h, a.ctypes.data_as(C.c_void_p)))
        return a

    def set_tone_map(self, curve: int = _ffi.TONE_FILMIC, exposure: float = 1.0, auto: bool = False, gamma2: bool = False, white: float = 0.0,
                     key: float = _ffi.TONE_KEY, adapt: float = 1.0, min_auto: float = 0.0, max_auto: float = 0.0,
                     percentile: int = _ffi.TONE_PERCENTILE, opts=None):
        """vrt_set_tone_map: every later MODE_PATH frame is presented (present / present_device only) through an exposure and a
        tone curve — _ffi.TONE_LINEAR / TONE_REINHARD (white: the value mapped to 1) / TONE_FILMIC, gamma2: a square-root encode
        behind it; curve _ffi.TONE_OFF = off, the default.  auto: the exposure is metered from every frame on the GPU (the
        percentile-th thousandth of the luminance histogram is brought to key, times `exposure`, within min_auto / max_auto)
        and adapts by `adapt` of the way per frame.  opts: a ready _ffi.ToneMap instead of the keywords.  Sharded and multi-device
        contexts refuse a curve."""
        o = opts if opts is not None else _ffi.tone_setting(curve, exposure, auto, gamma2, white, key, adapt, min_auto, max_auto, percentile)
        self._ck(self._lib.vrt_set_tone_map(self._h, C.byref(o)))

    def tone_info(self) -> _ffi.ToneInfo:
        """vrt_get_tone_info: the exposure of the last mapped frame and what it metered (synchronises)."""
        info = _ffi.ToneInfo()
        self._ck(self._lib.vrt_get_tone_info(self._h, C.byref(info)))
        return info

    def tone_histogram(self) -> np.ndarray:
        """vrt_read_tone_histogram: the 256 luminance bins of the last metered frame (synchronises)."""
        bins = np.empty(256, dtype=np.uint32)
        self._ck(self._lib.vrt_read_tone_histogram(self._h, bins.ctypes.data_as(C.c_void_p)))
        return bins

    def set_sun_light(self, strength: float):
        """vrt_set_sun_light: every hit of a later MODE_PATH frame sends a ray to the sun and, where nothing is in the way, adds
        settings.sun_intensity * strength * dot(normal, sun direction) times its colour (0 = off, the default).  The primary
        modes ignore it; changing it restarts the accumulation."""
        o = _ffi.SunLight(strength, 0, (C.c_uint32 * 2)(0, 0))
        self._ck(self._lib.vrt_set_sun_light(self._h, C.byref(o)))

    def set_water_optics(self, absorb=None, reflectance: float = 0.0):
        """vrt_set_water_optics: later MODE_PATH frames see water — a segment that starts outside a liquid stops at a liquid voxel
        and is reflected with Schlick's probability (reflectance: at normal incidence, in [0, 1]) or goes on into it; a segment
        that starts inside one loses exp(-absorb * length in the liquid) per channel (absorb: three floats per voxel length, or
        one for all three).  absorb None = off, the default.  The primary modes ignore it; changing it restarts the accumulation.
        Not yet together with set_lamp_light or set_camera_sampling: such a frame is refused."""
        if absorb is None:
            self._ck(self._lib.vrt_set_water_optics(self._h, None))
            return
        a = np.broadcast_to(np.asarray(absorb, dtype=np.float32), (3,))
        o = _ffi.WaterOptics((C.c_float * 3)(*(float(x) for x in a)), reflectance, _ffi.WATER_ON, (C.c_uint32 * 3)(0, 0, 0))
        self._ck(self._lib.vrt_set_water_optics(self._h, C.byref(o)))

    def set_water_refraction(self, ior: float, max_span: int = 0):
        """vrt_set_water_refraction: in later MODE_PATH frames with set_water_optics on, a path that enters the water is bent by
        Snell's law (ior: the water's index of refraction relative to air, in [1, 4]; 1.33 is water's), and a segment inside the
        water that reaches its surface from below is mirrored back (always, past the critical angle) or bent out into the air.
        max_span: the unit voxels such a segment's walk to the surface may cross (0 = 64, at most 1024).  ior 0 = off, the
        default.  With water optics off the setting is kept and changes nothing; changing it restarts the accumulation."""
        o = _ffi.WaterRefraction(ior, max_span, 0, 0)
        self._ck(self._lib.vrt_set_water_refraction(self._h, C.byref(o)))

    def set_haze(self, density: float, albedo=1.0):
        """vrt_set_haze: later MODE_PATH frames have air that scatters light — every segment of a path may end in a scatter event
        (density: extinction per voxel length, in [2^-20, 64]) that keeps albedo of the throughput (three floats in [0, 1], or one
        for all three), sends a sun ray from there when set_sun_light is on, and goes on in a uniformly drawn direction.
        density 0 = off, the default.  The primary modes ignore it; changing it restarts the accumulation.  With it on, a path
        frame is refused (VRT_ERR_STATE) while set_water_optics, set_lamp_light or set_camera_sampling is on."""
        a = np.broadcast_to(np.asarray(albedo, dtype=np.float32), (3,))
        o = _ffi.Haze(density, (C.c_float * 3)(*(float(x) for x in a)), 0, (C.c_uint32 * 3)(0, 0, 0))
        self._ck(self._lib.vrt_set_haze(self._h, C.byref(o)))

    def set_camera_sampling(self, pixel_spread: float, aperture: float = 0.0, focus_distance: float = 0.0):
        """vrt_set_camera_sampling: every sample of a later MODE_PATH frame gets a primary ray of its own — through a point of
        the pixel_spread-wide box around the pixel's centre (1: the pixel itself; 0: no jitter) and, with aperture != 0, from
        a point of a lens of that radius (in voxels) towards the point of the pixel's ray focus_distance away.  Both 0 = off,
        the default.  The primary modes ignore it; changing it restarts the accumulation."""
        o = _ffi.CameraSampling(pixel_spread, aperture, focus_distance, 0)
        self._ck(self._lib.vrt_set_camera_sampling(self._h, C.byref(o)))

    def set_lamp_light(self, strength: float, max_geometry: float = 0.0):
        """vrt_set_lamp_light: every hit of a later MODE_PATH frame sends a ray to a point of a face of the world's lamp list —
        the emissive voxels' faces that look at air or a liquid, derived on the GPU — and, where it arrives, adds that lamp's
        light (0 = off, the default; 1 = what a diffuse bounce would have found by chance).  max_geometry clamps the geometry
        factor (0 = no clamp).  The primary modes ignore it; changing it restarts the accumulation."""
        o = _ffi.LampLight(strength, max_geometry, 0, 0)
        self._ck(self._lib.vrt_set_lamp_light(self._h, C.byref(o)))

    def lamp_info(self) -> dict:
        """vrt_get_lamp_info: of the list the last lamp-lit frame used — listed, cap, faces, builds, last_build_ms."""
        o = _ffi.LampInfo()
        self._ck(self._lib.vrt_get_lamp_info(self._h, C.byref(o)))
        return {"listed": o.listed, "cap": o.cap, "faces": o.faces, "builds": o.builds, "last_build_ms": o.last_build_ms}

    def read_lamps(self) -> np.ndarray:
        """vrt_read_lamps: the lamp list the last lamp-lit frame used, as records of _ffi.LAMP_DTYPE in list order."""
        n = C.c_uint32(0)
        self._ck(self._lib.vrt_read_lamps(self._h, None, 0, C.byref(n)))
        a = np.zeros(n.value, dtype=_ffi.LAMP_DTYPE)
        if n.value:
            self._ck(self._lib.vrt_read_lamps(self._h, a.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return a

    def synchronize(self):
        self._ck(self._lib.vrt_synchronize(self._h))

    # --- read-back (no reference counterpart) ---
    def read_output(self, rgb=True, ids=True, rgba8=False):
        w, h = self.result_size
        a_rgb = np.empty((h, w, 3), dtype=np.float32) if rgb else None
        a_ids = np.empty((h, w), dtype=np.uint32) if ids else None
        a_q = np.empty((h, w, 4), dtype=np.uint8) if rgba8 else None
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        self._ck(self._lib.vrt_read_output(self._h, p(a_rgb), p(a_ids), p(a_q)))
        return a_rgb, a_ids, a_q

    def present(self, screen_size=None, color=(1.0, 1.0, 1.0, 0.33), style: int = 2, size: float = 5.0) -> np.ndarray:
        """ScreenShader::encode_pass into host memory: rgba8 [screen_h, screen_w, 4] of the last frame, sampled through the
        reference's (bilinear) sampler at any window size, under the crosshair (defaults = Crosshair::default(), mod.rs:71-80)."""
        sw, sh = screen_size or self.result_size
        ch = _ffi.Crosshair((C.c_float * 4)(*color), style, size)
        out = np.empty((sh, sw, 4), dtype=np.uint8)
        self._ck(self._lib.vrt_present(self._h, C.byref(ch), sw, sh, out.ctypes.data_as(C.c_void_p)))
        return out

    def present_device(self, screen_size=None, color=(1.0, 1.0, 1.0, 0.33), style: int = 2, size: float = 5.0):
        """vrt_present_device: (device pointer, bytes) of the presented rgba8 image, left on the GPU."""
        sw, sh = screen_size or self.result_size
        ch = _ffi.Crosshair((C.c_float * 4)(*color), style, size)
        ptr, nb = C.c_void_p(), C.c_uint64()
        self._ck(self._lib.vrt_present_device(self._h, C.byref(ch), sw, sh, C.byref(ptr), C.byref(nb)))
        return ptr.value, nb.value

    def set_presentation(self, screen_size=None, color=(1.0, 1.0, 1.0, 0.33), style: int = 2, size: float = 5.0, skip_texels: bool = False, off: bool = False):
        """vrt_set_presentation: the frames that follow are presented to a window of screen_size under this crosshair — when the window
        samples the texture texel for texel their march kernel stores the window's image itself and present / present_device with the
        same crosshair and size launch nothing (main.rs:452-454 in one launch).  skip_texels: such frames store the image only."""
        sw, sh = screen_size or self.result_size
        ch = _ffi.Crosshair((C.c_float * 4)(*color), style, size)
        self._ck(self._lib.vrt_set_presentation(self._h, None if off else C.byref(ch), sw, sh, 1 if skip_texels else 0))

    def read_steps(self) -> np.ndarray:
        w, h = self.result_size
        a = np.empty((h, w), dtype=np.uint32)
        self._ck(self._lib.vrt_read_steps(self._h, a.ctypes.data_as(C.c_void_p)))
        return a

    def stats(self) -> Stats:
        s = Stats()
        self._ck(self._lib.vrt_get_stats(self._h, C.byref(s)))
        return s

    def issue_profile(self) -> dict:
        """vrt_get_issue_profile: what issuing a frame cost the host (us, averaged over the render calls since the last call)."""
        p = _ffi.IssueProfile()
        self._ck(self._lib.vrt_get_issue_profile(self._h, C.byref(p)))
        return {k: getattr(p, k) for k, _ in p._fields_ if not k.startswith("_")}

    def accel_info(self) -> "_ffi.AccelInfo":
        """The derived lookup tables of the default march (cell grid + brick pool); rebuilt lazily by render()."""
        a = _ffi.AccelInfo()
        self._ck(self._lib.vrt_get_accel_info(self._h, C.byref(a)))
        return a

    def read_accel(self):
        """(grid[G,G,G] indexed [z,y,x], bricks[n,64]) as built on the device — see vrt_read_accel in include/vrt.h."""
        a = self.accel_info()
        g = a.world_size_chunks * 8
        grid = np.empty((g, g, g), dtype=np.uint32)
        bricks = np.empty((int(a.bricks), 64), dtype=np.uint16)
        self._ck(self._lib.vrt_read_accel(self._h, grid.ctypes.data_as(C.c_void_p), bricks.ctypes.data_as(C.c_void_p)))
        return grid, bricks

    def read_march_cells(self):
        """(cells[G,G,G,4] indexed [z,y,x], direct) — see vrt_read_march_cells in include/vrt.h."""
        g = self.accel_info().world_size_chunks * 8
        cells = np.empty((g, g, g, 4), dtype=np.uint32)
        direct = C.c_uint32()
        self._ck(self._lib.vrt_read_march_cells(self._h, cells.ctypes.data_as(C.c_void_p), C.byref(direct)))
        return cells, bool(direct.value)

    def read_tile_cost(self, tiles: int) -> np.ndarray:
        """The trips per tile the last frame that noted them took — see vrt_read_tile_cost in include/vrt.h."""
        cost = np.empty(tiles, dtype=np.uint32)
        self._ck(self._lib.vrt_read_tile_cost(self._h, cost.ctypes.data_as(C.c_void_p)))
        return cost

    def read_tile_order(self, tiles: int):
        """(order[tiles], dilated): the order the next frame of this view launches in — see vrt_read_tile_order in include/vrt.h."""
        order = np.empty(tiles, dtype=np.uint32)
        dilated = C.c_uint32()
        self._ck(self._lib.vrt_read_tile_order(self._h, order.ctypes.data_as(C.c_void_p), C.byref(dilated)))
        return order, bool(dilated.value)

    def lit_voxels(self, voxels: bool = False):
        """{passes, layers, lit_trips[, lit[n,n,n] indexed [z,y,x], n = 32 S]} — see vrt_read_lit_voxels in include/vrt.h."""
        p, k, t = C.c_uint32(), C.c_uint32(), C.c_uint32()
        lit = None
        if voxels:
            n = self.accel_info().world_size_chunks * 32
            lit = np.empty((n, n, n), dtype=np.uint8)
        self._ck(self._lib.vrt_read_lit_voxels(self._h, C.byref(p), C.byref(k), C.byref(t), lit.ctypes.data_as(C.c_void_p) if voxels else None))
        out = dict(passes=p.value, layers=k.value, lit_trips=t.value)
        if voxels:
            out["lit"] = lit
        return out

    def dark_voxels(self, voxels: bool = False):
        """{passes, layers[, dark[n,n,n] indexed [z,y,x], n = 32 S]} — see vrt_read_dark_voxels in include/vrt.h."""
        p, k = C.c_uint32(), C.c_uint32()
        dark = None
        if voxels:
            n = self.accel_info().world_size_chunks * 32
            dark = np.empty((n, n, n), dtype=np.uint8)
        self._ck(self._lib.vrt_read_dark_voxels(self._h, C.byref(p), C.byref(k), dark.ctypes.data_as(C.c_void_p) if voxels else None))
        out = dict(passes=p.value, layers=k.value)
        if voxels:
            out["dark"] = dark
        return out

    def dark_marks(self, cells: bool = False):
        """{passes, count, used[, dark[G,G,G] indexed [z,y,x]]} — see vrt_get_dark_marks in include/vrt.h."""
        p, n, u = C.c_uint32(), C.c_uint32(), C.c_uint32()
        dark = None
        if cells:
            g = self.accel_info().world_size_chunks * 8
            dark = np.empty((g, g, g), dtype=np.uint8)
        self._ck(self._lib.vrt_get_dark_marks(self._h, C.byref(p), C.byref(n), C.byref(u), dark.ctypes.data_as(C.c_void_p) if cells else None))
        out = dict(passes=p.value, count=n.value, used=bool(u.value))
        if cells:
            out["dark"] = dark
        return out

    def sun_marks(self, cells: bool = False):
        """{passes, min_leaf, lit_trips[, lit[G,G,G] indexed [z,y,x]]} — see vrt_get_sun_marks in include/vrt.h."""
        p, m, t = C.c_uint32(), C.c_uint32(), C.c_uint32()
        lit = None
        if cells:
            g = self.accel_info().world_size_chunks * 8
            lit = np.empty((g, g, g), dtype=np.uint8)
        self._ck(self._lib.vrt_get_sun_marks(self._h, C.byref(p), C.byref(m), C.byref(t), lit.ctypes.data_as(C.c_void_p) if cells else None))
        out = dict(passes=p.value, min_leaf=m.value, lit_trips=t.value)
        if cells:
            out["lit"] = lit
        return out

    # --- device plumbing for torch / RCCL ---
    def set_stream(self, hip_stream: int):
        self._ck(self._lib.vrt_set_stream(self._h, C.c_void_p(hip_stream)))

    def bind_output(self, texels_ptr: int):
        """Render into caller-owned device memory (a torch tensor); 0 restores the context's own buffer."""
        self._ck(self._lib.vrt_bind_output(self._h, C.c_void_p(texels_ptr or None)))

    def device_output(self):
        """(device pointer, bytes) of the 16-byte-texel buffer frames are written to."""
        t, nb = C.c_void_p(), C.c_uint64()
        self._ck(self._lib.vrt_device_output(self._h, C.byref(t), C.byref(nb)))
        return t.value, nb.value

    def shard_info(self):
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._ck(self._lib.vrt_shard_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def assemble(self, gathered_ptr: int, dst_ptr: int, rank_stride_bytes: int = 0, compact: bool = False):
        fn = self._lib.vrt_assemble_compact if compact else self._lib.vrt_assemble
        self._ck(fn(self._h, C.c_void_p(gathered_ptr), rank_stride_bytes, C.c_void_p(dst_ptr)))

    # --- world queries (include/vrt.h vrt_cast_rays) ---
    def cast_rays(self, starts, dirs, max_dist) -> np.ndarray:
        """common::math::cast_ray (math.rs:153-226) for every ray at once on the GPU, against the world as of every write so far:
        (n,3) starts and dirs, a scalar or (n,) max_dist.  Returns _ffi.RAY_HIT_DTYPE records (pos, face, dist, status)."""
        from .world import ray_queries
        q = ray_queries(starts, dirs, max_dist)
        out = np.zeros(q.size, _ffi.RAY_HIT_DTYPE)
        self._ck(self._lib.vrt_cast_rays(self._h, q.ctypes.data, q.size, out.ctypes.data))
        return out

    def cast_rays_device(self, queries_ptr: int, n: int, out_ptr: int):
        """vrt_cast_rays_device: n vrt_ray_query records at a device address in, n vrt_ray_hit records out, enqueued on the
        context's stream (vrt_set_stream) without waiting."""
        self._ck(self._lib.vrt_cast_rays_device(self._h, C.c_void_p(queries_ptr or None), n, C.c_void_p(out_ptr or None)))

    def clip_moves(self, queries: np.ndarray) -> np.ndarray:
        """clip_aabb_movement (player.rs:202-244) for every box at once on the GPU, against the world and the material table as of
        every write so far: _ffi.BOX_QUERY_DTYPE records (world.box_queries) in, _ffi.BOX_MOVE_DTYPE records out."""
        q = np.ascontiguousarray(queries, _ffi.BOX_QUERY_DTYPE)
        out = np.zeros(q.size, _ffi.BOX_MOVE_DTYPE)
        self._ck(self._lib.vrt_clip_moves(self._h, q.ctypes.data, q.size, out.ctypes.data))
        return out

    def clip_moves_device(self, queries_ptr: int, n: int, out_ptr: int):
        """vrt_clip_moves_device: n vrt_box_query records at a device address in, n vrt_box_move records out, enqueued on the
        context's stream (vrt_set_stream) without waiting."""
        self._ck(self._lib.vrt_clip_moves_device(self._h, C.c_void_p(queries_ptr or None), n, C.c_void_p(out_ptr or None)))

    def get_voxels(self, positions) -> np.ndarray:
        """ClientWorld::get_voxel (world.rs:352-357) for every (n,3) integer position at once on the GPU, against the world as of
        every write so far: _ffi.VOXEL_AT_DTYPE records (voxel, status = VOXEL_OK / VOXEL_OUT_OF_BOUNDS / VOXEL_NO_CHUNK)."""
        pos = np.ascontiguousarray(np.asarray(positions, np.int32).reshape(-1, 3))
        out = np.zeros(pos.shape[0], _ffi.VOXEL_AT_DTYPE)
        self._ck(self._lib.vrt_get_voxels(self._h, pos.ctypes.data, pos.shape[0], out.ctypes.data))
        return out

    def get_voxels_device(self, pos_ptr: int, n: int, out_ptr: int):
        """vrt_get_voxels_device: n x 3 int32 at a device address in, n vrt_voxel_at records out, enqueued on the context's stream
        (vrt_set_stream) without waiting."""
        self._ck(self._lib.vrt_get_voxels_device(self._h, C.c_void_p(pos_ptr or None), n, C.c_void_p(out_ptr or None)))

    def column_tops(self, queries: np.ndarray) -> np.ndarray:
        """ClientWorld::highest_vox_at (world.rs:359-366) with include/vrt.h's flags for every column at once on the GPU, against
        the world and the material table as of every write so far: _ffi.COLUMN_QUERY_DTYPE records (world.column_queries) in,
        _ffi.COLUMN_TOP_DTYPE records out."""
        q = np.ascontiguousarray(queries, _ffi.COLUMN_QUERY_DTYPE)
        out = np.zeros(q.size, _ffi.COLUMN_TOP_DTYPE)
        self._ck(self._lib.vrt_column_tops(self._h, q.ctypes.data, q.size, out.ctypes.data))
        return out

    def column_tops_device(self, queries_ptr: int, n: int, out_ptr: int):
        """vrt_column_tops_device: n vrt_column_query records at a device address in, n vrt_column_top records out, enqueued on
        the context's stream (vrt_set_stream) without waiting."""
        self._ck(self._lib.vrt_column_tops_device(self._h, C.c_void_p(queries_ptr or None), n, C.c_void_p(out_ptr or None)))

    def top_map(self, solid: bool = False) -> np.ndarray:
        """vrt_read_top_map: the whole world from above, _ffi.TOP_ENTRY_DTYPE records [z - min.z][x - min.x]; a column where
        nothing counts holds y = min.y - 1, voxel 0.  solid: VRT_COLUMN_SOLID."""
        W = 32 * self._world_size   # (0: no world set yet, and the library says so)
        # room for the largest world the context can hold, whatever it was last told: the library writes (32 S)^2 entries
        cap = 32 * max(self._roots_size, self._world_size, 1)
        buf = np.zeros(cap * cap, _ffi.TOP_ENTRY_DTYPE)
        self._ck(self._lib.vrt_read_top_map(self._h, _ffi.COLUMN_SOLID if solid else 0, buf.ctypes.data))
        return buf[:W * W].reshape(W, W).copy()

    def top_map_device(self, map_ptr: int, flags: int = 0):
        """vrt_top_map_device: (32 S)^2 vrt_top_entry records to a device address (8-byte aligned), enqueued on the context's
        stream (vrt_set_stream) without waiting."""
        self._ck(self._lib.vrt_top_map_device(self._h, flags, C.c_void_p(map_ptr or None)))

    # --- the chunk source (include/vrt.h vrt_generate_chunks / vrt_build_chunks / vrt_edit_chunks) ---
    def generate_chunks(self, seed: int, positions, strict: bool = True):
        """The build's world generator on the GPU (csrc/host/worldgen.hpp): (n,3) chunk positions -> (nodes, offsets), chunk i's
        nodes being nodes[offsets[i]:offsets[i+1]], word for word svo_build_bottom_up(gen_dense(seed, pos)).  A chunk whose tree
        the builder refuses has an empty range; strict=True raises VrtError for it (VRT_ERR_OUT_OF_RANGE), strict=False
        returns the other chunks' nodes."""
        pos = np.ascontiguousarray(np.asarray(positions, np.int32).reshape(-1, 3))
        return self._chunks(lambda nodes, cap, offs: self._lib.vrt_generate_chunks(
            self._h, seed & 0xFFFFFFFF, pos.ctypes.data, pos.shape[0], nodes, cap, offs), pos.shape[0], strict)

    def build_chunks(self, dense, strict: bool = True):
        """build_svo_bottom_up on the GPU for (n, 32768) u16 blocks, dense[x + 32*(y + 32*z)]: (nodes, offsets) as generate_chunks."""
        d = np.ascontiguousarray(np.asarray(dense, np.uint16).reshape(-1, 32768))
        return self._chunks(lambda nodes, cap, offs: self._lib.vrt_build_chunks(self._h, d.ctypes.data, d.shape[0], nodes, cap, offs),
                            d.shape[0], strict)

    def edit_chunks(self, positions, nodes, offsets, shapes, strict: bool = True):
        """The server's feature placement (World::place_features, server/src/world/mod.rs:28-55) or a brush, on the GPU: chunks
        at (n,3) positions with trees nodes[offsets[i]:offsets[i+1]] (chunk-relative child addresses: a GiveChunkData payload,
        a pool range) and vrt_shape records (world.shape_records) applied in order -> (nodes, offsets, changed); chunk i's new
        tree is word for word svo_build_bottom_up of its edited voxels and changed[i] says whether any voxel differs (the
        chunks to re-broadcast).  The CPU twin is world.edit_chunks.  strict as generate_chunks's."""
        from .world import shape_records
        pos = np.ascontiguousarray(np.asarray(positions, np.int32).reshape(-1, 3))
        nin = np.ascontiguousarray(nodes, np.uint16)
        oin = np.ascontiguousarray(offsets, np.uint64)
        sh = shape_records(shapes)
        n = pos.shape[0]
        if oin.size != n + 1:
            raise ValueError(f"{n} chunks need {n + 1} offsets, not {oin.size}")
        changed = np.zeros(n, np.uint8)
        nodes_out, offs = self._chunks(lambda out, cap, offs: self._lib.vrt_edit_chunks(
            self._h, pos.ctypes.data, n, nin.ctypes.data, oin.ctypes.data, sh.ctypes.data if sh.size else None, sh.size, out, cap, offs,
            changed.ctypes.data), n, strict)
        return nodes_out, offs, changed

    def _chunks(self, call, n: int, strict: bool):
        offs = np.zeros(n + 1, np.uint64)
        nodes = np.empty(max(1, 2048 * n), np.uint16)   # a guess (a generated chunk averages ~1 000 nodes); OOM tells the need
        rc = call(nodes.ctypes.data, nodes.size, offs.ctypes.data)
        if rc == _ffi.VRT_ERR_OOM and int(offs[n]) > nodes.size:
            nodes = np.empty(int(offs[n]), np.uint16)
            rc = call(nodes.ctypes.data, nodes.size, offs.ctypes.data)
        if rc and not (rc == _ffi.VRT_ERR_OUT_OF_RANGE and not strict):
            self._ck(rc)
        return nodes[:int(offs[n])].copy(), offs

    # --- convenience: what join_game does (main.rs:211-223) ---
    def upload_world(self, world, materials=None):
        """Upload the whole pool, chunk_roots, WorldData and materials of a ClientWorld."""
        self.write_nodes(world.nodes_ptr(), 0, world.max_nodes() & ~1)
        self.write_chunk_roots(world.chunk_roots())
        self.write_world_data(world.world_data())
        self.write_materials(materials if materials is not None else std_materials())

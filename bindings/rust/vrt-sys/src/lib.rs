//! Raw bindings to `include/vrt.h` — the C ABI of the MI355X SVO ray-march backend.
//!
//! The four uniform structs are byte-identical to the reference's `#[repr(C)]` structs
//! (`clientdesktop/src/graphics/mod.rs:20-28, 63-70, 82-91, 113-120, 132-143`), so the client can either use these
//! or pass pointers to its own `Material` / `Crosshair` / `CamData` / `WorldData` / `Settings` values unchanged.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)]
pub struct vrt_ctx {
    _private: [u8; 0],
}

pub const VRT_OK: c_int = 0;
pub const VRT_ERR_INVALID_ARG: c_int = -1;
pub const VRT_ERR_OUT_OF_RANGE: c_int = -2;
pub const VRT_ERR_DEVICE: c_int = -3;
pub const VRT_ERR_OOM: c_int = -4;
pub const VRT_ERR_STATE: c_int = -5;

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct vrt_material {
    pub color: [f32; 3],
    pub is_empty: u32,
    pub is_liquid: u32,
    pub scatter: f32,
    pub _padding: [u32; 2],
}

/// One entry of vrt_write_polish's table: the coat of path_tracer.wgsl's Material (polish_color, polish_bounce_chance,
/// polish_scatter).  All zero = no coat.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vrt_polish {
    pub color: [f32; 3],
    pub chance: f32,
    pub scatter: f32,
    pub _reserved: [u32; 3],
}

/// One entry of vrt_write_translucency's table: the pass-through lobe of path_tracer.wgsl's Material (translucency).
/// All zero = opaque.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vrt_translucency {
    pub color: [f32; 3],
    pub chance: f32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct vrt_cam_data {
    pub pos: [f32; 3],
    pub _padding0: u32,
    pub inv_view_mat: [f32; 16],
    pub inv_proj_mat: [f32; 16],
    pub proj_size: [f32; 2],
    pub _padding1: [u32; 2],
}

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct vrt_world_data {
    pub min: [i32; 3],
    pub size: u32,
    pub size_in_chunks: u32,
    pub _padding: [u32; 3],
}

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct vrt_settings {
    pub max_ray_bounces: u32,
    pub sun_intensity: f32,
    pub show_step_count: u32,
    pub _padding0: u32,
    pub sky_color: [f32; 3],
    pub _padding1: u32,
    pub sun_pos: [f32; 3],
    pub _padding2: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct vrt_crosshair {
    pub color: [f32; 4],
    pub style: u32,
    pub size: f32,
    pub _padding: [u32; 2],
}

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct vrt_config {
    pub max_nodes: u32,
    pub world_size_chunks: u32,
    pub width: u32,
    pub height: u32,
    pub device: i32,
    pub shard_rank: u32,
    pub shard_count: u32,
    pub flags: u32,
    pub shard_root_weight: u32,
    pub n_devices: u32,
    pub device_ids: [i32; VRT_MAX_DEVICES],
}

pub const VRT_MAX_DEVICES: usize = 16;
pub const VRT_FLAG_TILE_MAJOR: u32 = 1;
pub const VRT_FLAG_ROW_MAJOR: u32 = 2;
pub const VRT_FLAG_COMPACT: u32 = 4;
pub const VRT_PRESENT_SKIP_TEXELS: u32 = 1;
pub const VRT_FLAG_TEXEL_MESSAGES: u32 = 8;
pub const VRT_FLAG_STAGED_MESSAGES: u32 = 16;
pub const VRT_FLAG_POISON_MESSAGES: u32 = 32;

pub const VRT_MODE_PRIMARY: u32 = 0;
pub const VRT_MODE_PRIMARY_SHADOW: u32 = 1;
pub const VRT_MODE_PATH: u32 = 2;

pub const VRT_RENDER_OWN_STREAMS: u32 = 1;
pub const VRT_RENDER_TIMED: u32 = 2;
pub const VRT_RENDER_ACCUMULATE: u32 = 4;

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct vrt_render_opts {
    pub mode: u32,
    pub variant: u32,
    pub stats: u32,
    pub spp: u32,
    pub seed: u32,
    pub flags: u32,
    pub _reserved: [u32; 2],
}

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct vrt_stats {
    pub primary_rays: u64,
    pub secondary_rays: u64,
    pub hits: u64,
    pub steps: u64,
    pub node_visits: u64,
    pub primary_steps: u64,
    pub primary_node_visits: u64,
    pub ms_total: f32,
    pub ms_primary: f32,
    pub ms_secondary: f32,
    pub frames: u32,
    pub sum_ms_primary: f64,
    pub sum_ms_secondary: f64,
    pub sum_ms_total: f64,
    pub clock_shader_ticks: u64,
    pub clock_ref_ticks: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct vrt_accel_info {
    pub available: u32,
    pub world_size_chunks: u32,
    pub cells: u64,
    pub bricks: u64,
    pub bytes: u64,
    pub builds: u32,
    pub last_build_ms: f32,
    pub chunk_builds: u32,
    pub ordered_frames: u32,
}

/// One `common::math::cast_ray(start, dir, max_dist, ..)` query (vrt_cast_rays).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vrt_ray_query {
    pub start: [f32; 3],
    pub max_dist: f32,
    pub dir: [f32; 3],
    pub _reserved: u32,
}

pub const VRT_RAY_MISS: u32 = 0;
pub const VRT_RAY_HIT: u32 = 1;
pub const VRT_RAY_REJECTED: u32 = 2;

/// Its answer: `Option<HitResult>` as `status` (VRT_RAY_*) plus `pos` / `face`, and the DDA's `dist` at the hit.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vrt_ray_hit {
    pub pos: [i32; 3],
    pub face: [i32; 3],
    pub dist: f32,
    pub status: u32,
}

const _: () = assert!(core::mem::size_of::<vrt_ray_query>() == 32);
const _: () = assert!(core::mem::size_of::<vrt_ray_hit>() == 32);

/// One `clip_aabb_movement(Aabb::new(from, to), mv, |bb| world.get_collisions_w(bb, ..), autojump)` query (vrt_clip_moves).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vrt_box_query {
    pub from: [f32; 3],
    pub flags: u32,
    pub to: [f32; 3],
    pub _r0: u32,
    pub mv: [f32; 3],
    pub _r1: u32,
}

pub const VRT_BOX_AUTOJUMP: u32 = 1;
pub const VRT_BOX_MAX_VOXELS: u32 = 4096;
pub const VRT_BOX_MOVED: u32 = 0;
pub const VRT_BOX_REJECTED: u32 = 2;
pub const VRT_BOX_CLIPPED_X: u32 = 1;
pub const VRT_BOX_CLIPPED_Y: u32 = 2;
pub const VRT_BOX_CLIPPED_Z: u32 = 4;
pub const VRT_BOX_STEPPED_UP: u32 = 8;

/// Its answer: `mv` is the reference's `mv_clipped` when `status` is VRT_BOX_MOVED; `flags` says which axes the first pass
/// clipped and whether the step-up was taken, `boxes[p]` how many solid voxels pass `p` gathered.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vrt_box_move {
    pub mv: [f32; 3],
    pub status: u32,
    pub flags: u32,
    pub boxes: [u32; 2],
    pub _reserved: u32,
}

const _: () = assert!(core::mem::size_of::<vrt_box_query>() == 48);
const _: () = assert!(core::mem::size_of::<vrt_box_move>() == 32);

pub const VRT_VOXEL_OK: u16 = 0;
pub const VRT_VOXEL_OUT_OF_BOUNDS: u16 = 1;
pub const VRT_VOXEL_NO_CHUNK: u16 = 3;

/// `ClientWorld::get_voxel(pos)` (vrt_get_voxels): the voxel when `status` is VRT_VOXEL_OK, else 0 and the SetVoxelErr's number.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vrt_voxel_at {
    pub voxel: u16,
    pub status: u16,
}

pub const VRT_COLUMN_FROM_Y: u32 = 1;
pub const VRT_COLUMN_SOLID: u32 = 2;
pub const VRT_COLUMN_NONE: u32 = 0;
pub const VRT_COLUMN_FOUND: u32 = 1;
pub const VRT_COLUMN_OUTSIDE: u32 = 2;

/// One `ClientWorld::highest_vox_at` query (vrt_column_tops): the column, and with VRT_COLUMN_FROM_Y where the scan starts.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vrt_column_query {
    pub x: i32,
    pub z: i32,
    pub from_y: i32,
    pub flags: u32,
}

/// Its answer: the highest voxel that counts when `status` is VRT_COLUMN_FOUND.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vrt_column_top {
    pub y: i32,
    pub voxel: u32,
    pub status: u32,
    pub _reserved: u32,
}

/// One column of vrt_read_top_map: `y` is `world.min[1] - 1` and `voxel` 0 where nothing counts.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vrt_top_entry {
    pub y: i32,
    pub voxel: u32,
}

const _: () = assert!(core::mem::size_of::<vrt_voxel_at>() == 4);
const _: () = assert!(core::mem::size_of::<vrt_column_query>() == 16);
const _: () = assert!(core::mem::size_of::<vrt_column_top>() == 16);
const _: () = assert!(core::mem::size_of::<vrt_top_entry>() == 8);

/// vrt_set_denoise: the path trace's edge-stopped a-trous filter (passes 0 = off, 1..5; sigma_color 0 = no colour stop).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vrt_denoise_opts {
    pub passes: u32,
    pub sigma_color: f32,
    pub flags: u32,
    pub _reserved: u32,
}

/// vrt_set_tone_map: exposure and tone curve of presented path frames (curve VRT_TONE_OFF = off; include/vrt.h has the contract).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vrt_tone_map {
    pub curve: u32,
    pub flags: u32,
    pub exposure: f32,
    pub white: f32,
    pub key: f32,
    pub adapt: f32,
    pub min_auto: f32,
    pub max_auto: f32,
    pub percentile: u32,
    pub _reserved: [u32; 3],
}

/// vrt_get_tone_info: the last mapped frame's exposure and, with VRT_TONE_AUTO, what it metered.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vrt_tone_info {
    pub exposure: f32,
    pub target: f32,
    pub luminance: f32,
    pub bin: u32,
    pub counted: u64,
    pub skipped: u64,
    pub frames: u32,
    pub _reserved: u32,
}

pub const VRT_TONE_OFF: u32 = 0;
pub const VRT_TONE_LINEAR: u32 = 1;
pub const VRT_TONE_REINHARD: u32 = 2;
pub const VRT_TONE_FILMIC: u32 = 3;
pub const VRT_TONE_AUTO: u32 = 1;
pub const VRT_TONE_GAMMA2: u32 = 2;

/// vrt_set_sun_light: direct sunlight for the path trace (strength 0 = off; the sun term's factor on settings.sun_intensity).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vrt_sun_light {
    pub strength: f32,
    pub flags: u32,
    pub _reserved: [u32; 2],
}

/// vrt_set_water_optics: water for the path trace — absorption per voxel length and channel inside a liquid, the surface's
/// reflectance at normal incidence (flags 0 = off, VRT_WATER_ON = on).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vrt_water_optics {
    pub absorb: [f32; 3],
    pub reflectance: f32,
    pub flags: u32,
    pub _reserved: [u32; 3],
}

/// vrt_set_haze: air that scatters light in the path trace — extinction per voxel length (density 0 = off; otherwise in
/// [2^-20, 64]) and what a scatter event keeps of the throughput per channel (albedo, in [0, 1]).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vrt_haze {
    pub density: f32,
    pub albedo: [f32; 3],
    pub flags: u32,
    pub _reserved: [u32; 3],
}

/// vrt_set_water_refraction: Snell's law at the water's surface and the surface seen from below, in frames with water optics on
/// (ior 0 = off; otherwise in [1, 4]; max_span: the unit voxels a wet segment's span walk may cross, 0 = 64, at most 1024).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vrt_water_refraction {
    pub ior: f32,
    pub max_span: u32,
    pub flags: u32,
    pub _reserved: u32,
}
pub const VRT_WATER_ON: u32 = 1;

/// vrt_set_camera_sampling: pixel jitter and a thin lens for the path trace (pixel_spread and aperture both 0 = off).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vrt_camera_sampling {
    pub pixel_spread: f32,
    pub aperture: f32,
    pub focus_distance: f32,
    pub flags: u32,
}

/// vrt_set_lamp_light: next-event estimation towards the world's emissive voxels for the path trace (strength 0 = off;
/// max_geometry 0 = the geometry factor is not clamped).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vrt_lamp_light {
    pub strength: f32,
    pub max_geometry: f32,
    pub flags: u32,
    pub _reserved: u32,
}

/// An entry of the lamp list (vrt_read_lamps): a face of an emissive voxel, world-local voxel coordinates; face = 2 * axis + side.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vrt_lamp {
    pub pos: [u16; 3],
    pub voxel: u16,
    pub face: u32,
    pub _reserved: u32,
}

/// The lamp list the last lamp-lit frame used (vrt_get_lamp_info).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vrt_lamp_info {
    pub listed: u32,
    pub cap: u32,
    pub faces: u64,
    pub builds: u32,
    pub last_build_ms: f32,
}

/// What issuing a frame costs the host (vrt_get_issue_profile), microseconds per vrt_render call.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vrt_issue_profile {
    pub frames: u32,
    pub devices: u32,
    pub issuing_threads: u32,
    pub _reserved: u32,
    pub render_us: f64,
    pub root_issue_us: f64,
    pub shard_issue_us_mean: f64,
    pub shard_issue_us_max: f64,
    pub join_wait_us: f64,
    pub tail_us: f64,
    pub message_waits_us: f64,
}

/// One call of the server's BuiltFeature (server/src/world/gen.rs:312-354) for vrt_edit_chunks.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vrt_shape {
    pub kind: u32,
    pub voxel: u32,
    pub a: [i32; 3],
    pub b: [i32; 3],
    pub r: f32,
    pub height: u32,
}
pub const VRT_SHAPE_POINT: u32 = 0;
pub const VRT_SHAPE_LINE: u32 = 1;
pub const VRT_SHAPE_SPHERE: u32 = 2;
pub const VRT_SHAPE_DISC: u32 = 3;

pub const VRT_ID_VOXEL_MASK: u32 = 0x7FFF;
pub const VRT_ID_HIT: u32 = 1 << 16;
pub const VRT_ID_NX: u32 = 1 << 17;
pub const VRT_ID_NY: u32 = 1 << 18;
pub const VRT_ID_NZ: u32 = 1 << 19;
pub const VRT_ID_WATER: u32 = 1 << 20;
pub const VRT_ID_SHADOW_RAY: u32 = 1 << 21;
pub const VRT_ID_SHADOWED: u32 = 1 << 22;

extern "C" {
    pub fn vrt_create(cfg: *const vrt_config, out: *mut *mut vrt_ctx) -> c_int;
    pub fn vrt_destroy(ctx: *mut vrt_ctx);
    pub fn vrt_last_error(ctx: *const vrt_ctx) -> *const c_char;
    pub fn vrt_write_nodes(ctx: *mut vrt_ctx, pool: *const u16, start: u32, end: u32) -> c_int;
    pub fn vrt_write_chunk_roots(ctx: *mut vrt_ctx, offset: u32, roots: *const u32, n: u32) -> c_int;
    pub fn vrt_write_chunk_roots_tagged(ctx: *mut vrt_ctx, offset: u32, roots: *const u32, n: u32, tag: u64) -> c_int;
    pub fn vrt_resize_world(ctx: *mut vrt_ctx, world_size_chunks: u32) -> c_int;
    pub fn vrt_write_materials(ctx: *mut vrt_ctx, first: u32, mats: *const vrt_material, n: u32) -> c_int;
    pub fn vrt_write_emission(ctx: *mut vrt_ctx, first: u32, emission: *const f32, n: u32) -> c_int;
    pub fn vrt_write_polish(ctx: *mut vrt_ctx, first: u32, polish: *const vrt_polish, n: u32) -> c_int;
    pub fn vrt_write_translucency(ctx: *mut vrt_ctx, first: u32, entries: *const vrt_translucency, n: u32) -> c_int;
    pub fn vrt_set_camera(ctx: *mut vrt_ctx, cam: *const vrt_cam_data) -> c_int;
    pub fn vrt_set_settings(ctx: *mut vrt_ctx, settings: *const vrt_settings) -> c_int;
    pub fn vrt_set_world(ctx: *mut vrt_ctx, world: *const vrt_world_data) -> c_int;
    pub fn vrt_resize_output(ctx: *mut vrt_ctx, width: u32, height: u32) -> c_int;
    pub fn vrt_render(ctx: *mut vrt_ctx, opts: *const vrt_render_opts) -> c_int;
    pub fn vrt_set_frames_in_flight(ctx: *mut vrt_ctx, n: u32) -> c_int;
    pub fn vrt_reset_accumulation(ctx: *mut vrt_ctx) -> c_int;
    pub fn vrt_get_accumulation(ctx: *mut vrt_ctx, samples: *mut u32, seed: *mut u32) -> c_int;
    pub fn vrt_set_denoise(ctx: *mut vrt_ctx, opts: *const vrt_denoise_opts) -> c_int;
    pub fn vrt_read_guide(ctx: *mut vrt_ctx, guide: *mut u32) -> c_int;
    pub fn vrt_selftest_denoise(device: i32, rgb: *const f32, ids: *const u32, guide: *const u32, w: u32, h: u32, opts: *const vrt_denoise_opts, rgb_out: *mut f32, ids_out: *mut u32) -> c_int;
    pub fn vrt_set_tone_map(ctx: *mut vrt_ctx, opts: *const vrt_tone_map) -> c_int;
    pub fn vrt_get_tone_info(ctx: *mut vrt_ctx, out: *mut vrt_tone_info) -> c_int;
    pub fn vrt_read_tone_histogram(ctx: *mut vrt_ctx, bins: *mut u32) -> c_int;
    pub fn vrt_set_sun_light(ctx: *mut vrt_ctx, opts: *const vrt_sun_light) -> c_int;
    pub fn vrt_set_water_optics(ctx: *mut vrt_ctx, opts: *const vrt_water_optics) -> c_int;
    pub fn vrt_set_water_refraction(ctx: *mut vrt_ctx, opts: *const vrt_water_refraction) -> c_int;
    pub fn vrt_set_haze(ctx: *mut vrt_ctx, opts: *const vrt_haze) -> c_int;
    pub fn vrt_set_camera_sampling(ctx: *mut vrt_ctx, opts: *const vrt_camera_sampling) -> c_int;
    pub fn vrt_set_lamp_light(ctx: *mut vrt_ctx, opts: *const vrt_lamp_light) -> c_int;
    pub fn vrt_get_lamp_info(ctx: *mut vrt_ctx, out: *mut vrt_lamp_info) -> c_int;
    pub fn vrt_read_lamps(ctx: *mut vrt_ctx, out: *mut vrt_lamp, cap: u32, n: *mut u32) -> c_int;
    pub fn vrt_synchronize(ctx: *mut vrt_ctx) -> c_int;
    pub fn vrt_read_output(ctx: *mut vrt_ctx, rgb: *mut f32, ids: *mut u32, rgba8: *mut u8) -> c_int;
    pub fn vrt_present(ctx: *mut vrt_ctx, crosshair: *const vrt_crosshair, screen_w: u32, screen_h: u32, rgba8: *mut u8) -> c_int;
    pub fn vrt_selftest_exact_math(device: i32, n: u32, seed: u32, mismatches: *mut u64) -> c_int;
    /// `op`: 0 .. 21, the VRT_MATH_* of include/vrt.h, which also gives the words per operand set of `input` and `out`.
    pub fn vrt_selftest_math_values(device: i32, op: u32, n: u32, input: *const u32, out: *mut u32) -> c_int;
    pub fn vrt_present_device(ctx: *mut vrt_ctx, crosshair: *const vrt_crosshair, screen_w: u32, screen_h: u32, rgba8_device: *mut *mut c_void, bytes: *mut u64) -> c_int;
    pub fn vrt_set_presentation(ctx: *mut vrt_ctx, crosshair: *const vrt_crosshair, screen_w: u32, screen_h: u32, flags: u32) -> c_int;
    pub fn vrt_get_stats(ctx: *mut vrt_ctx, out: *mut vrt_stats) -> c_int;
    pub fn vrt_get_issue_profile(ctx: *mut vrt_ctx, out: *mut vrt_issue_profile) -> c_int;
    pub fn vrt_get_accel_info(ctx: *mut vrt_ctx, out: *mut vrt_accel_info) -> c_int;
    pub fn vrt_read_accel(ctx: *mut vrt_ctx, grid: *mut u32, bricks: *mut u16) -> c_int;
    pub fn vrt_read_march_cells(ctx: *mut vrt_ctx, cells: *mut u32, direct: *mut u32) -> c_int;
    pub fn vrt_read_tile_cost(ctx: *mut vrt_ctx, cost: *mut u32) -> c_int;
    pub fn vrt_read_tile_order(ctx: *mut vrt_ctx, order: *mut u32, dilated: *mut u32) -> c_int;
    pub fn vrt_selftest_tile_order(device: i32, cost: *const u32, tiles_x: u32, tiles_y: u32, radius: i32, order: *mut u32) -> c_int;
    pub fn vrt_get_sun_marks(ctx: *mut vrt_ctx, passes: *mut u32, min_leaf: *mut u32, lit_trips: *mut u32, lit: *mut u8) -> c_int;
    pub fn vrt_read_lit_voxels(ctx: *mut vrt_ctx, passes: *mut u32, layers: *mut u32, lit_trips: *mut u32, lit: *mut u8) -> c_int;
    pub fn vrt_read_dark_voxels(ctx: *mut vrt_ctx, passes: *mut u32, layers: *mut u32, dark: *mut u8) -> c_int;
    pub fn vrt_get_dark_marks(ctx: *mut vrt_ctx, passes: *mut u32, count: *mut u32, used: *mut u32, dark: *mut u8) -> c_int;
    pub fn vrt_read_steps(ctx: *mut vrt_ctx, steps: *mut u32) -> c_int;
    pub fn vrt_set_stream(ctx: *mut vrt_ctx, hip_stream: *mut c_void) -> c_int;
    pub fn vrt_bind_output(ctx: *mut vrt_ctx, texels: *mut c_void) -> c_int;
    pub fn vrt_device_output(ctx: *mut vrt_ctx, texels: *mut *mut c_void, bytes: *mut u64) -> c_int;
    pub fn vrt_shard_info(ctx: *mut vrt_ctx, tiles_local: *mut u32, tiles_padded: *mut u32, tiles_total: *mut u32) -> c_int;
    pub fn vrt_assemble(ctx: *mut vrt_ctx, gathered: *const c_void, rank_stride_bytes: u64, dst: *mut c_void) -> c_int;
    pub fn vrt_assemble_compact(ctx: *mut vrt_ctx, gathered: *const c_void, rank_stride_bytes: u64, dst: *mut c_void) -> c_int;
    pub fn vrt_cast_rays(ctx: *mut vrt_ctx, queries: *const vrt_ray_query, n: u32, out: *mut vrt_ray_hit) -> c_int;
    pub fn vrt_cast_rays_device(ctx: *mut vrt_ctx, queries_device: *const c_void, n: u32, out_device: *mut c_void) -> c_int;
    pub fn vrt_clip_moves(ctx: *mut vrt_ctx, queries: *const vrt_box_query, n: u32, out: *mut vrt_box_move) -> c_int;
    pub fn vrt_clip_moves_device(ctx: *mut vrt_ctx, queries_device: *const c_void, n: u32, out_device: *mut c_void) -> c_int;
    pub fn vrt_get_voxels(ctx: *mut vrt_ctx, pos: *const i32, n: u32, out: *mut vrt_voxel_at) -> c_int;
    pub fn vrt_get_voxels_device(ctx: *mut vrt_ctx, pos_device: *const c_void, n: u32, out_device: *mut c_void) -> c_int;
    pub fn vrt_column_tops(ctx: *mut vrt_ctx, queries: *const vrt_column_query, n: u32, out: *mut vrt_column_top) -> c_int;
    pub fn vrt_column_tops_device(ctx: *mut vrt_ctx, queries_device: *const c_void, n: u32, out_device: *mut c_void) -> c_int;
    pub fn vrt_read_top_map(ctx: *mut vrt_ctx, flags: u32, map: *mut vrt_top_entry) -> c_int;
    pub fn vrt_top_map_device(ctx: *mut vrt_ctx, flags: u32, map_device: *mut c_void) -> c_int;
    pub fn vrt_generate_chunks(ctx: *mut vrt_ctx, seed: u32, chunk_pos: *const i32, n: u32, nodes: *mut u16, cap_nodes: u64,
                               offsets: *mut u64) -> c_int;
    pub fn vrt_build_chunks(ctx: *mut vrt_ctx, dense: *const u16, n: u32, nodes: *mut u16, cap_nodes: u64, offsets: *mut u64) -> c_int;
    pub fn vrt_edit_chunks(ctx: *mut vrt_ctx, chunk_pos: *const i32, n: u32, nodes_in: *const u16, offsets_in: *const u64,
                           shapes: *const vrt_shape, m: u32, nodes_out: *mut u16, cap_nodes: u64, offsets_out: *mut u64,
                           changed: *mut u8) -> c_int;
}

#[cfg(test)]
mod layout {
    use super::*;
    use std::mem::size_of;
    #[test]
    fn struct_sizes_match_the_header() {
        assert_eq!(size_of::<vrt_material>(), 32);
        assert_eq!(size_of::<vrt_cam_data>(), 160);
        assert_eq!(size_of::<vrt_world_data>(), 32);
        assert_eq!(size_of::<vrt_settings>(), 48);
        assert_eq!(size_of::<vrt_crosshair>(), 32);
        assert_eq!(size_of::<vrt_config>(), 104);
        assert_eq!(size_of::<vrt_render_opts>(), 32);
        assert_eq!(size_of::<vrt_stats>(), 112);
        assert_eq!(size_of::<vrt_accel_info>(), 48);
        assert_eq!(size_of::<vrt_issue_profile>(), 72);
        assert!(size_of::<vrt_denoise_opts>() == 16);
        assert!(size_of::<vrt_tone_map>() == 48);
        assert!(size_of::<vrt_tone_info>() == 40);
        assert!(size_of::<vrt_sun_light>() == 16);
        assert!(size_of::<vrt_water_optics>() == 32);
        assert!(size_of::<vrt_water_refraction>() == 16);
        assert!(size_of::<vrt_haze>() == 32);
        assert!(size_of::<vrt_camera_sampling>() == 16);
        assert!(size_of::<vrt_lamp_light>() == 16);
        assert!(size_of::<vrt_lamp>() == 16);
        assert!(size_of::<vrt_lamp_info>() == 24);
        assert!(size_of::<vrt_shape>() == 40);
        assert!(size_of::<vrt_polish>() == 32);
        assert!(size_of::<vrt_translucency>() == 16);
    }
}

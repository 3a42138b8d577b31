/*
 * vrt.h — C ABI of the MI355X (gfx950) SVO ray-march backend (libvrt.so).
 *
 * This is the drop-in boundary for the reference's GPU seam: everything the winit frame loop does to
 * `GpuResources` / `Buffers` / `PixelShader` (MasonFeurer/VoxelRayTracing,
 * clientdesktop/src/graphics/{mod.rs,shader.rs}, callers in clientdesktop/src/main.rs) maps to one
 * call below.  Plain pointers and sizes only; the four uniform structs are byte-identical to the
 * reference's #[repr(C)] structs, so a Rust host passes its own values unchanged (INTEGRATION.md shows
 * the `extern "C"` block a maintainer would add).
 *
 * Semantics shared by every write: the host owns the source memory, the call copies at call time
 * (wgpu `queue.write_buffer`, shader.rs:105,113,141) and the data is visible to the next vrt_render.
 * One thread per context (the reference drives this seam from the winit thread only,
 * main.rs:681-722); calls are ordered on one HIP stream.
 *
 * Every function returns VRT_OK (0) or a negative vrt_status; vrt_last_error() gives the text.
 * Nothing aborts: the reference's unwrap()/panic sites (mod.rs:223-274, client/src/world.rs:251)
 * become status codes.
 */
#ifndef VRT_H
#define VRT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vrt_ctx vrt_ctx;

typedef enum {
    VRT_OK = 0,
    VRT_ERR_INVALID_ARG = -1,
    VRT_ERR_OUT_OF_RANGE = -2,
    VRT_ERR_DEVICE = -3,
    VRT_ERR_OOM = -4,
    VRT_ERR_STATE = -5
} vrt_status;

/* Material — clientdesktop/src/graphics/mod.rs:20-28 (32 B). */
typedef struct {
    float color[3];
    uint32_t is_empty;
    uint32_t is_liquid;
    float scatter;
    uint32_t _padding[2];
} vrt_material;

/* CamData — mod.rs:82-91 (160 B). Column-major 4x4 (glam Mat4). */
typedef struct {
    float pos[3];
    uint32_t _padding0;
    float inv_view_mat[16];
    float inv_proj_mat[16];
    float proj_size[2];
    uint32_t _padding1[2];
} vrt_cam_data;

/* WorldData — mod.rs:113-120 (32 B). */
typedef struct {
    int32_t min[3];
    uint32_t size;
    uint32_t size_in_chunks;
    uint32_t _padding[3];
} vrt_world_data;

/* Settings — mod.rs:132-143 (48 B). */
typedef struct {
    uint32_t max_ray_bounces;
    float sun_intensity;
    uint32_t show_step_count;
    uint32_t _padding0;
    float sky_color[3];
    uint32_t _padding1;
    float sun_pos[3];
    uint32_t _padding2;
} vrt_settings;

/* Crosshair — mod.rs:63-70 (32 B). style: 0 off, 1 dot, 2 cross (screen_shader.wgsl:9-13). */
typedef struct {
    float color[4];
    uint32_t style;
    float size;
    uint32_t _padding[2];
} vrt_crosshair;

/* Replaces the arguments of GpuResources::new(gpu, fmt, result_size, max_nodes, world_size)
 * (mod.rs:155-195).  shard_rank/shard_count: this context traces only its share of the 8x8 screen tiles
 * (tile-interleaved multi-GPU sharding; 0/1 = whole frame).  Tiles are dealt out in periods of
 * P = shard_root_weight + shard_count - 1: the first shard_root_weight tiles of every period belong to rank 0, the
 * next ones to ranks 1, 2, ... one each.  shard_root_weight 0 or 1 = equal shares (tile t belongs to rank t % N).
 * A weight > 1 lets the gather root, whose own tiles never cross a link, take more of the frame than the ranks
 * whose tiles all arrive over one xGMI link each. */
#define VRT_MAX_DEVICES 16
typedef struct {
    uint32_t max_nodes;          /* NodeBuffer capacity in nodes (shader.rs:9-16; forced even); 2 .. 2^31 - 2^17 */
    uint32_t world_size_chunks;  /* S: chunk_roots holds S^3 entries (shader.rs:59,67) */
    uint32_t width, height;      /* result texture size, any non-zero size (main.rs:257-262: 1080 rows at the window's
                                  * aspect).  As in the reference, width/8 x height/8 tiles of 8x8 pixels are traced
                                  * (main.rs:452, integer division); the pixels beyond them stay zero, alpha included */
    int32_t device;              /* HIP device ordinal; -1 = current */
    uint32_t shard_rank, shard_count;
    uint32_t flags;              /* VRT_FLAG_* */
    uint32_t shard_root_weight;  /* tiles per period dealt to rank 0; 0 = 1 (a multi-device context: 0 = a default for n_devices) */
    /* One context, one thread, N devices (the reference drives one GpuResources from the winit thread, main.rs:398-455):
     * n_devices > 1 makes this a multi-device context over device_ids[0 .. n_devices) — the same ordinal may appear more
     * than once (a one-GPU rehearsal).  Every write is replicated to all of them (the scene is read-only during a frame),
     * vrt_render traces the frame's 8x8 tiles interleaved over the devices — device_ids[0] its share straight into the
     * row-major frame, the others as 8-byte records stored over xGMI directly into device_ids[0]'s memory
     * (hipDeviceEnablePeerAccess; no collective library, no second process) — and device_ids[0] shades those records into the
     * frame.  The frame, read-backs, vrt_present and vrt_device_output are device_ids[0]'s.  shard_rank / shard_count must be
     * 0 / 0-1; of the flags VRT_FLAG_TEXEL_MESSAGES, VRT_FLAG_STAGED_MESSAGES and VRT_FLAG_POISON_MESSAGES apply.  n_devices
     * 0 or 1: `device` alone, as before. */
    uint32_t n_devices;
    int32_t device_ids[VRT_MAX_DEVICES];
} vrt_config;

/* Write the output in the tile-major shard layout even with shard_count = 1 (a one-rank gather pipeline). */
#define VRT_FLAG_TILE_MAJOR 1u
/* A sharded context that writes its tiles at their final positions of a row-major full-frame buffer instead of a
 * compact tile-major one: the gather root rendering straight into the frame (vrt_assemble then skips its tiles). */
#define VRT_FLAG_ROW_MAJOR 2u
/* A tile-major shard context whose buffer travels over a link: store 8 bytes per pixel slot instead of the 16-byte
 * texel — {id word | bit 23 (norm.y < 0), water_dist as f32} — which is all the gather root needs, beside the frame's
 * uniforms it holds anyway, to shade the pixel itself bit for bit (vrt_assemble_compact).  Plain primary(+shadow)
 * frames with the default march only; vrt_read_output is not available on such a context. */
#define VRT_FLAG_COMPACT 4u

/* A multi-device context (vrt_config.n_devices > 1) whose other devices send whole 16-byte texels instead of 8-byte
 * records: twice the bytes over every link, but every kind of frame — also the path trace and the non-default marches,
 * whose pixels the root cannot re-shade from an id word. */
#define VRT_FLAG_TEXEL_MESSAGES 8u
/* A multi-device context whose other devices render their messages into a buffer of their own and copy it to device_ids[0]
 * afterwards (hipMemcpyPeerAsync on the sender's stream) instead of storing into device_ids[0]'s memory directly.  Taken
 * by itself for every device whose peer access to device_ids[0] is refused (hipDeviceEnablePeerAccess); the flag forces
 * it for all of them (tests, and hosts on which peer stores are slower than a copy engine). */
#define VRT_FLAG_STAGED_MESSAGES 16u
/* Testing: device_ids[0] overwrites a message slot with 0xFF bytes as soon as it has assembled the slot's frame, so a frame
 * assembled from a slot that its senders have not written again yet — a missing wait, a stale read — is visibly wrong. */
#define VRT_FLAG_POISON_MESSAGES 32u

typedef enum {
    VRT_MODE_PRIMARY = 0,        /* the reference's live shader (ray_tracer.wgsl) */
    VRT_MODE_PRIMARY_SHADOW = 1, /* + 1 shadow ray per solid hit, from a compacted hit buffer */
    VRT_MODE_PATH = 2            /* multi-bounce path trace after path_tracer.wgsl (build-defined) */
} vrt_mode;

typedef struct {
    uint32_t mode;     /* vrt_mode */
    uint32_t variant;  /* kernel variant: 0 = default (grid march over the derived cell grid / brick pool; primary +
                        * shadow fused into one launch), 1 = literal octree walk (the shader's text), 2 = ancestor-cache
                        * octree walk, 3 = grid march with the shadow rays as a second launch; DESIGN.md §Kernels */
    uint32_t stats;    /* 1: also count steps / node visits this frame (slower; not for timing); 2: clock probe — the default
                        * primary + shadow kernel with s_memtime / s_memrealtime stamps around one wave in sixteen
                        * (vrt_stats.clock_*; the frame itself is the normal one) */
    uint32_t spp;      /* VRT_MODE_PATH only */
    uint32_t seed;     /* VRT_MODE_PATH only */
    uint32_t flags;    /* VRT_RENDER_* */
    uint32_t _reserved[2];
} vrt_render_opts;

/* Run this frame on the context's own in-flight streams although the caller has set a stream (vrt_set_stream) and / or
 * bound an output (vrt_bind_output).  The caller promises that nothing it enqueues on its stream reads this frame's
 * output before vrt_synchronize (or a device-wide synchronise), and that frames in flight are bound to different
 * buffers.  For a gather root that renders its own tiles in place: they never feed the collective. */
#define VRT_RENDER_OWN_STREAMS 1u
/* This frame's launches carry timing events (vrt_stats.frames / sum_ms_*) whatever the context's sampling of plain frames
 * is (every 8th: a launch with events costs the host three times one without). */
#define VRT_RENDER_TIMED 2u
/* VRT_MODE_PATH only (any other mode: VRT_ERR_INVALID_ARG, nothing enqueued): progressive accumulation.  With n samples
 * accumulated so far the frame traces samples n .. n + spp - 1, adds them in sample order to the context's running sum
 * (never divided) and stores sum / (n + spp) in its output texels, with the id word a plain path frame writes: K frames of
 * s spp are, bit for bit, one frame of K * s spp with the same seed.  The sum starts again at n = 0 (without a device
 * step: the first frame stores it) after vrt_reset_accumulation, or when anything the image depends on has changed since
 * the previous accumulating frame: the camera, settings or world (byte-wise), any vrt_write_materials, a non-empty
 * vrt_write_emission, vrt_write_polish or vrt_write_translucency that is not refused, a non-empty vrt_write_nodes, a chunk_roots write that changes content, vrt_resize_world / vrt_resize_output, or another opts.seed.
 * Non-accumulating frames in between change nothing.  n + spp > 2^24: VRT_ERR_OUT_OF_RANGE, nothing enqueued. */
#define VRT_RENDER_ACCUMULATE 4u

/* New relative to the reference (it presents to a swapchain and never reads back). */
typedef struct {
    uint64_t primary_rays;
    uint64_t secondary_rays;      /* shadow / bounce rays actually launched */
    uint64_t hits;
    uint64_t steps;               /* valid when the frame was rendered with opts.stats = 1 */
    uint64_t node_visits;
    uint64_t primary_steps;
    uint64_t primary_node_visits;
    float ms_total;               /* hipEvent time of the last frame's kernels, same stream */
    float ms_primary;             /* the march kernel over primary rays */
    float ms_secondary;           /* shadow / bounce kernels */
    uint32_t frames;              /* frames *timed* since the previous vrt_get_stats — every stats frame, and every 8th plain */
    double sum_ms_primary;        /* frame (the first included; a launch that carries timing events costs the host three times */
    double sum_ms_secondary;      /* one that does not) — and their summed kernel times (events stamped by the dispatches) */
    double sum_ms_total;
    uint64_t clock_shader_ticks;  /* clock-probe frames (opts.stats = 2) since the previous vrt_get_stats: summed s_memtime */
    uint64_t clock_ref_ticks;     /* ... and s_memrealtime (100 MHz) differences: shader clock = 100 MHz x their ratio */
} vrt_stats;

/* Per-pixel id word written next to the f32 radiance (build-defined; bit-exact parity target):
 * bits 0..14 voxel id; 16 hit; 17..19 norm.x/y/z != 0; 20 water overlay; 21 shadow ray launched;
 * 22 shadow ray occluded. */
#define VRT_ID_VOXEL_MASK 0x7FFFu
#define VRT_ID_HIT (1u << 16)
#define VRT_ID_NX (1u << 17)
#define VRT_ID_NY (1u << 18)
#define VRT_ID_NZ (1u << 19)
#define VRT_ID_WATER (1u << 20)
#define VRT_ID_SHADOW_RAY (1u << 21)
#define VRT_ID_SHADOWED (1u << 22)

/* GpuResources::new + Buffers::new + PixelShader::new (mod.rs:155-195, shader.rs:55-72,301-344). */
int vrt_create(const vrt_config *cfg, vrt_ctx **out);
void vrt_destroy(vrt_ctx *ctx);

/* Text of the last error on this context (ctx may be NULL: last creation error). */
const char *vrt_last_error(const vrt_ctx *ctx);

/* NodeBuffer::write(gpu, src_nodes (the whole pool), start..end) — shader.rs:22-40.
 * `pool` points at node 0 of the host pool; [start,end) is widened to even bounds exactly as the
 * reference does, so pool must be readable on [start&~1, end+(end&1)). */
int vrt_write_nodes(vrt_ctx *ctx, const uint16_t *pool, uint32_t start, uint32_t end);

/* ArrayBuffer<NodeAddr>::write(gpu, offset, items) — shader.rs:133-142; silently truncates to the
 * buffer's capacity like the reference. */
int vrt_write_chunk_roots(vrt_ctx *ctx, uint32_t offset, const uint32_t *roots, uint32_t n);

/* The same with the caller's word for "which table this is": the reference rewrites the table every frame (main.rs:446),
 * nearly always unchanged, and at 32^3 chunks the backend's compare of 128 KB is half a frame's host time.  tag != 0 that
 * equals the tag of the previous call (same offset and n) returns at once — the caller vouches that the contents are
 * the same — any other value is an ordinary write that remembers the tag (a host world's generation counter, bumped by
 * create_chunk / center_chunks / resize; include/vrt_host.h: vrth_world_chunk_roots_generation).  tag 0 = no tag. */
int vrt_write_chunk_roots_tagged(vrt_ctx *ctx, uint32_t offset, const uint32_t *roots, uint32_t n, uint64_t tag);

/* Buffers::resize_chunk_buffer(world_size) + recreate_bind_group — shader.rs:74-80, main.rs:441-445.
 * Contents are undefined afterwards (a fresh buffer in the reference). */
int vrt_resize_world(vrt_ctx *ctx, uint32_t world_size_chunks);

/* SimpleBuffer<[Material;256]>::write_slice(first, mats) — shader.rs:108-115, main.rs:219-223. */
int vrt_write_materials(vrt_ctx *ctx, uint32_t first, const vrt_material *mats, uint32_t n);

/* New relative to the live reference: the emission of path_tracer.wgsl's Material (:27, :183-184), kept in a table of its
 * own beside the material table (vrt_material stays the reference's 32 bytes; its _padding is not read).  256 floats per
 * context, indexed like the material table (voxel ids >= 255 use entry 255), all 0 until written; entries [first,
 * first + n) are copied at call time.  VRT_MODE_PATH only: the primary (+ shadow) modes are the live ray_tracer.wgsl,
 * which has no emission, and ignore the table.
 * On every hit of a path (the hit of its last allowed segment included) whose voxel's entry e is not 0, the sample's light
 * gains (mc * e) * thr per channel in f32 — mc the colour the throughput is then multiplied by (face shading, and the
 * step-count grey under show_step_count), thr the throughput before the hit — ahead of thr *= mc, as :183-186 order it.
 * A hit with e == 0 adds nothing.  A sample's light is its terms summed in segment order (the sky's, on a miss, last); the
 * frame's is the sum of its samples' lights in sample order, / spp, and VRT_RENDER_ACCUMULATE keeps its identity.  Id words,
 * step counts, the RNG stream and every path direction are those of the same frame without emission.
 * first + n > 256: VRT_ERR_OUT_OF_RANGE; emission NULL with n > 0, or an entry that is negative, NaN or infinite:
 * VRT_ERR_INVALID_ARG — nothing written either way.  n == 0 is a no-op; any other write restarts the accumulation.  A table
 * that is all zero (never written, or written back to zeros) renders exactly as a context without one. */
int vrt_write_emission(vrt_ctx *ctx, uint32_t first, const float *emission, uint32_t n);

/* New relative to the live reference: the rest of path_tracer.wgsl's Material — polish_bounce_chance, polish_color and
 * polish_scatter (:28-31), whose three uses in ray_color are commented out there (:175, :180, :185): a second, specular lobe.
 * A coin flip per hit chooses between the material's own lobe and a coat with a colour and a roughness of its own.
 * (translucency, :29 and :167-173, the struct's last field, is vrt_translucency below: a table of its own again.) */
typedef struct {
    float    color[3];      /* what the throughput is multiplied by on a polished bounce; NOT face-shaded */
    float    chance;        /* a hit bounces off the coat when u < chance; 0 = never (the default) */
    float    scatter;       /* the coat's scatter, used in place of vrt_material.scatter on a polished bounce */
    uint32_t _reserved[3];  /* not read */
} vrt_polish;               /* 32 B */
/* The table: 256 entries per context, indexed like the material and emission tables (voxel ids >= 255 use entry 255), all
 * bytes 0 until written; entries [first, first + n) are copied at call time.  VRT_MODE_PATH only: the primary (+ shadow)
 * modes ignore the table, and their frames are byte for byte what they are without it.
 * A frame is polished when at least one entry's chance != 0.0f.  A table whose chances are all +0 or -0 renders byte for
 * byte as a context that never called this function — same kernels, nothing launched or allocated — whatever the other
 * fields hold.
 * On every hit of a polished frame after which the path goes on, whatever that voxel's own entry says, the body of
 * ray_color's loop is, in this order:
 *   1. mc is the hit colour as without the table (face shading, or the step-count grey under show_step_count);
 *   2. the emission term is unchanged and uses mc: (mc * e) * thr, ahead of everything below;
 *   3. u = rng_next(rng): one draw, taken before the six draws of rng_next_dir (:175 stands before :178);
 *   4. polished = u < entry.chance (rng_next can return exactly 1.0: chance = 1 is "nearly always", any chance > 1 "always");
 *   5. scatter = polished ? entry.scatter : material.scatter;
 *   6. tint = polished ? entry.color : mc — selects (the reference's mix(a, b, f32(bool)) is one for finite operands);
 *      entry.color is used as written, also under show_step_count;
 *   7. the specular and the scattered direction, the mix by scatter and both normalisations are as without the table;
 *   8. thr *= tint; the next origin is as without the table.
 * A hit on the path's last allowed segment draws nothing that anything can observe; its emission is still added.
 * What follows from that: id words and the primary segment are those of the unpolished frame.  Writing the first non-zero
 * chance shifts the RNG stream of every path by one draw per hit, so the frame changes even where no ray meets a coated
 * voxel.  At max_ray_bounces <= 1 a polish table changes nothing.  The sums keep the emission contract: a sample's light is
 * its terms in segment order with the sky last; the frame's light is its samples' lights in sample order, divided by spp.
 * VRT_RENDER_ACCUMULATE keeps its identity: K frames of s spp equal one frame of K * s spp, bit for bit.
 * first + n > 256: VRT_ERR_OUT_OF_RANGE; polish NULL with n > 0, a null context, or any of an entry's five floats negative,
 * NaN or infinite: VRT_ERR_INVALID_ARG — a refused call writes nothing.  n == 0 is a no-op; any other write restarts the
 * accumulation, as vrt_write_emission does.  A context over several devices replicates the write to every device; a shard's
 * context keeps its own table. */
int vrt_write_polish(vrt_ctx *ctx, uint32_t first, const vrt_polish *polish, uint32_t n);

/* New relative to the live reference: the last field of path_tracer.wgsl's Material, translucency (:29), whose use in
 * ray_color is commented out there (:167-173): a third lobe, through which a path passes straight on.  The reference's text
 * cannot be taken literally — it restarts the ray 0.001 along its direction, inside the voxel it has just hit, which the
 * next ray_world hits again on its first lookup until the bounces run out — so the pass is defined here.  Two things are
 * the reference's: the draw stands ahead of the coat's draw, and a pass costs one of the path's segments. */
typedef struct {
    float color[3];   /* what the throughput is multiplied by when a path passes through; used as written, NOT face-shaded */
    float chance;     /* a hit passes through when u < chance; 0 = never (the default) */
} vrt_translucency;   /* 16 B: one load */
/* The table: 256 entries per context, indexed like the material, emission and polish tables (voxel ids >= 255 use entry
 * 255), all bytes 0 until written; entries [first, first + n) are copied at call time.  VRT_MODE_PATH only: the primary
 * (+ shadow) modes ignore the table, and their frames are byte for byte what they are without it.
 * A frame is translucent when at least one entry's chance != 0.0f.  A table whose chances are all +0 or -0 renders byte for
 * byte as a context that never called this function — same kernels, nothing launched or allocated — whatever the colours
 * hold.
 * On every hit of a translucent frame after which the path may go on, the body of ray_color's loop is, in this order:
 *   1. mc is the hit colour as without the table (face shading, or the step-count grey under show_step_count);
 *   2. the emission term is unchanged, (mc * e) * thr, ahead of everything below: a pane that gives off light does so
 *      whether or not the path passes;
 *   3. ut = rng_next(rng): one draw on every hit, whatever that voxel's entry says, taken before the coat's draw u (a
 *      polished frame only) and before the direction's six;
 *   4. passes = ut < entry.chance (as for the coat: chance = 1 is "nearly always", any chance > 1 "always");
 *   5. if passes: no further draw is taken (no u, no direction); thr *= entry.color per channel; dir is unchanged; the
 *      origin moves across the one UNIT voxel that holds the hit position pos, whatever the size of the leaf the tree keeps
 *      that voxel in (a re-canonicalised tree renders the same), all in strict binary32 with nothing contracted — per axis
 *        c = floorf(pos); far = dir > 0 ? c + 1 : c; t_a = dir != 0 ? (far - pos) / dir : +inf;
 *      then t = t_x; if (t_y < t) t = t_y; if (t_z < t) t = t_z (compares and selects, not fminf), and
 *        origin = pos + dir * (t + 0.001f) per component, a multiply and then an add,
 *      the form in which the march itself advances across an air node.  The next segment is an ordinary one from that
 *      origin, with the march's usual start nudge; one that starts inside a solid voxel hits on its first lookup with a
 *      zero normal, as any such segment does — a hit like any other, which draws ut again and can pass again.  A ray that
 *      leaves the world misses and takes the sky;
 *   6. if not: the body is exactly the polished or the unpolished body (vrt_write_polish above), the bounce origin
 *      pos + norm * bias.
 * A hit on the path's last allowed segment draws nothing that anything can observe; its emission is still added.
 * What follows from that: id words and the primary segment are those of the frame without the table.  Writing the first
 * non-zero chance shifts the RNG stream of every path by one draw per hit, so the frame changes even where no ray meets a
 * translucent voxel.  At max_ray_bounces <= 1 the table changes nothing.  Liquids do not consult it: the march passes them
 * itself.  The sums keep the emission contract: a sample's light is its terms in segment order with the sky last; the
 * frame's light is its samples' lights in sample order, divided by spp.  VRT_RENDER_ACCUMULATE keeps its identity: K frames
 * of s spp equal one frame of K * s spp, bit for bit.  The denoiser's key and guide come from the primary segment and are
 * what they were.
 * first + n > 256: VRT_ERR_OUT_OF_RANGE; entries NULL with n > 0, a null context, or any of an entry's four floats
 * negative, NaN or infinite: VRT_ERR_INVALID_ARG — a refused call writes nothing.  n == 0 is a no-op; any other write
 * restarts the accumulation, as vrt_write_emission does.  A context over several devices replicates the write to every
 * device; a shard's context keeps its own table. */
int vrt_write_translucency(vrt_ctx *ctx, uint32_t first, const vrt_translucency *entries, uint32_t n);

/* SimpleBuffer<T>::write — shader.rs:101-106; callers main.rs:428,439,447-449. */
int vrt_set_camera(vrt_ctx *ctx, const vrt_cam_data *cam);
int vrt_set_settings(vrt_ctx *ctx, const vrt_settings *settings);
int vrt_set_world(vrt_ctx *ctx, const vrt_world_data *world);

/* GpuResources::resize_result_texture — mod.rs:201-211. */
int vrt_resize_output(vrt_ctx *ctx, uint32_t width, uint32_t height);

/* PixelShader::encode_pass(encoder, tex_size/8) + queue.submit — shader.rs:371-379, main.rs:452-453,565.
 * Asynchronous: enqueues the frame's kernels on the context's stream. opts NULL = primary, default. */
int vrt_render(vrt_ctx *ctx, const vrt_render_opts *opts);

/* How many frames the context keeps in flight (1..4, default 2 — a swapchain gives the reference's wgpu path the same):
 * consecutive vrt_render calls of plain frames (default march, no stats, the context's own stream and output buffers;
 * also path-trace frames) alternate between that many internal streams, each with its own output (and path) buffers, so
 * one frame's tail overlaps the next one's ramp-up.  Every other call waits for all of them first; vrt_read_output / vrt_present /
 * vrt_device_output refer to the most recent frame.  1 = strictly one frame at a time; while the view is at rest (camera,
 * settings, world and materials unchanged since the previous frame) the launch's tail is then shortened from within:
 * primary + shadow frames launch their 8x8 tiles longest first, in the order of the march-loop trips the view's second frame
 * noted.  While the camera moves (and nothing else changes) a frame of up to 40 000 tiles notes its trips once in a while, one
 * small launch behind it sorts blocks of 4 x 4 tiles by their trips dilated over 5 blocks, and that order is kept for the frames
 * that follow until the camera leaves what the dilation covers (1080p at 70 degrees: ~ 9 degrees, 6.5 voxels); a view that leaps
 * stops asking.  Any other change of the view returns to screen order.  The frame is the same whatever the order;
 * VRT_TILE_ORDER=0 keeps screen order always, VRT_TILE_ORDER_MOVING=0 while the camera moves (profiles/r05_tile_order_moving.txt). */
int vrt_set_frames_in_flight(vrt_ctx *ctx, uint32_t n);

/* VRT_RENDER_ACCUMULATE: the next accumulating frame starts again at n = 0. */
int vrt_reset_accumulation(vrt_ctx *ctx);
/* VRT_RENDER_ACCUMULATE: the samples in the last accumulating frame's mean (0 before the first) and its seed.  Host-side
 * state: never synchronises.  Either pointer may be NULL. */
int vrt_get_accumulation(vrt_ctx *ctx, uint32_t *samples, uint32_t *seed);

/* While the view moves every VRT_MODE_PATH frame is a fresh 1-spp image.  vrt_set_denoise filters every later path frame on
 * the GPU with an edge-stopped a-trous filter (Dammertz et al. 2010), on the frame's own stream behind its last path launch
 * (the resolve of an accumulating or multi-sample frame included): the filtered colours are what the frame's texels hold, for
 * vrt_read_output, vrt_present*, vrt_device_output and a bound output alike; id words are never touched.  The primary modes
 * are the live shader's bytes and are never filtered.  Build-defined, and defined exactly:
 *   traced area  the 8 (W / 8) x 8 (H / 8) pixels a frame stores to; pixels beyond it keep their zeros
 *   filterable   a pixel whose id word has VRT_ID_HIT and at least one of VRT_ID_NX / NY / NZ; every other pixel is copied
 *   key(p)       id(p) & (VRT_ID_VOXEL_MASK | VRT_ID_HIT | VRT_ID_NX | VRT_ID_NY | VRT_ID_NZ | VRT_ID_WATER)
 *   guide(p)     (uint32_t)(int32_t)floorf(pos[a] + 0.5f) of a filterable pixel: pos the primary march's hit position in
 *                world-local voxels, a the lowest-numbered axis whose normal bit is set (the integer coordinate of the hit
 *                face's plane); 0 for every other pixel
 *   h            {0.0625, 0.25, 0.375, 0.25, 0.0625}
 * Pass i = 0 .. passes - 1 has tap spacing s = 1 << i and gives a filterable p, of colour c_p,
 *   sum = {0,0,0}; wsum = 0
 *   for dy = -2..2, for dx = -2..2 (both ascending):  q = p + s (dx, dy); skipped when outside the traced area or
 *                                                     key(q) != key(p) or guide(q) != guide(p)
 *       w = h[dy + 2] * h[dx + 2]
 *       if sigma_color != 0:  sg = sigma_color / (float)(1u << i);  d = c_q - c_p per channel;
 *                             d2 = (d.r * d.r + d.g * d.g) + d.b * d.b;  w = w * ((sg * sg) / ((sg * sg) + d2))
 *       sum.ch = sum.ch + w * c_q.ch;  wsum = wsum + w
 *   out = sum / wsum per channel
 * in strict binary32, in this order, nothing contracted; a NaN or infinite colour takes no special path.  Two pixels that
 * agree on key and guide lie on the same voxel face, whose face-shaded material colour is one value: the filter averages
 * irradiance, and never across a face's edge.  An accumulation's sum stays unfiltered (the filter works on the frame's mean:
 * K accumulated frames, denoised, are one denoised frame of K times the samples, bit for bit), and changing the setting does
 * not restart it.  opts NULL or passes == 0: off, the default — frames are byte for byte what they are without this call and
 * nothing is launched or allocated.  passes > 5, a negative, NaN or infinite sigma_color, flags or _reserved not 0:
 * VRT_ERR_INVALID_ARG; passes > 0 on a sharded, tile-major or multi-device context (no neighbouring pixels to read):
 * VRT_ERR_STATE.  A refused call changes nothing.  A timed frame's GPU time (vrt_get_stats, VRT_RENDER_TIMED) includes the
 * guide launch and the passes.  Suggested: passes 5, sigma_color 0 (docs/KERNELS.md has the sweep). */
typedef struct vrt_denoise_opts {
    uint32_t passes;      /* 0 = off (the default); 1..5 a-trous passes, tap spacing 1, 2, 4, 8, 16 pixels */
    float    sigma_color; /* colour stop of pass 0, halved every pass; 0 = no colour stop */
    uint32_t flags;       /* 0 */
    uint32_t _reserved;   /* 0 */
} vrt_denoise_opts;   /* 16 B */
int vrt_set_denoise(vrt_ctx *ctx, const vrt_denoise_opts *opts);
/* Diagnostic: the guide words of the last denoised frame, width * height of them row-major (0 beyond the traced area).
 * Synchronises.  VRT_ERR_STATE before the first denoised frame (and after a resize until the next one). */
int vrt_read_guide(vrt_ctx *ctx, uint32_t *guide);
/* Self-test of the filter's pass kernels on a frame of the caller's choosing.  The arguments are vrth_denoise's (vrt_host.h):
 * rgb w*h*3 f32, ids and guide w*h words, row-major, w the stride of a row; the traced area is the first 8 (w / 8) x 8 (h / 8)
 * pixels.  The arrays go to `device` as one frame of texels (r, g, b, id word) and a second copy of it, and opts->passes passes run
 * between the two through the launcher a frame uses, with a frame's tap spacings, kernels per spacing and sigma per pass;
 * rgb_out w*h*3 f32 and ids_out w*h words (may be NULL) receive the colours and the id words of the copy the last pass wrote —
 * with passes == 0 the input.  By the definition above that is vrth_denoise's output to the bit (a NaN's sign and payload aside),
 * every id word is the caller's, all 32 bits of it, and a pixel no pass stores to — beyond the traced area, or everywhere when w or h
 * is below 8, which is legal — comes back with the caller's bytes whatever they are.  A null pointer other than ids_out, w or h
 * of 0, or options vrt_set_denoise refuses: VRT_ERR_INVALID_ARG; w * h above 2^24: VRT_ERR_OUT_OF_RANGE; a refused call writes
 * nothing.  Buffers and a stream of its own, freed on every path; synchronises.  Diagnostic only: no context needed, never part
 * of a frame. */
int vrt_selftest_denoise(int32_t device, const float *rgb, const uint32_t *ids, const uint32_t *guide, uint32_t w, uint32_t h,
                         const vrt_denoise_opts *opts, float *rgb_out, uint32_t *ids_out);

/* Exposure and tone mapping of presented path frames.  A path frame's radiance lies well outside [0, 1] (emission, the sun
 * term, the lamps); vrt_present / vrt_present_device quantise unorm8(clamp(c, 0, 1)), the live shader's textureStore, which is
 * right for the primary modes and clips a path frame.  vrt_set_tone_map puts an exposure E — the host's, or metered from every
 * frame — and a tone curve between the texel and that quantisation.  Build-defined, and defined exactly, in strict binary32,
 * nothing contracted:
 *   mapped frame  a VRT_MODE_PATH frame rendered while curve != VRT_TONE_OFF.  The whole setting is the frame's from vrt_render
 *                 on: a vrt_set_tone_map between render and present does not change what the frame presents as.  Primary and
 *                 primary + shadow frames are never mapped, and the fused presentation (vrt_set_presentation) is theirs alone.
 *   scope         vrt_present and vrt_present_device only.  vrt_read_output (all three outputs), vrt_device_output, a bound
 *                 output, the accumulation's sum, the denoiser's input and the id words are what they are without the setting,
 *                 and changing it does not restart the accumulation.
 *   the map       the blit quantises every texel it taps with unorm8(encode(curve(c * E))) per colour channel in place of
 *                 unorm8(c); alpha, the bilinear sample, the crosshair's blend and the final quantisation are unchanged.
 *                   x = c * E
 *                   LINEAR    y = x
 *                   REINHARD  w2 = white * white (once, on the host);
 *                             y = white != 0 ? (x * (1.0f + x / w2)) / (1.0f + x) : x / (1.0f + x)
 *                   FILMIC    y = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f)      (Narkowicz's ACES fit)
 *                   GAMMA2    y = sqrtf(clamp(y, 0, 1)), the clamp the quantisation's own: (y > 0 ? y : 0), then the smaller of it and 1
 *                 A NaN or an infinity takes no special path (a NaN quantises to 0).  Every curve maps 0 to 0.
 *   metering      VRT_TONE_AUTO: behind the frame's last launch on its own stream (the resolve of a multi-sample or accumulating
 *                 frame and the denoiser's passes included: the colours the frame's texels hold).  For every pixel of the traced
 *                 area 8 (W / 8) x 8 (H / 8):  lum = (0.2126f * r + 0.7152f * g) + 0.0722f * b;  skipped when !(lum > 0) or lum
 *                 is infinite;  otherwise counted in bin clamp((int)(bits(lum) >> 20) - 888, 0, 255): eight bins an octave from
 *                 2^-16 to 2^16, denormals and larger values in the end bins.  Then, once:
 *                   N = the bins' sum.  N == 0: target = the previous adapted exposure, or `exposure` if there is none
 *                   otherwise, in 64 bits, rank = min(N * percentile / 1000, N - 1); b = the lowest bin whose inclusive prefix
 *                   sum exceeds rank; before = the prefix sum below b; lo = as_float((b + 888) << 20), hi = as_float((b + 889) << 20);
 *                   frac = ((float)(uint32_t)(rank - before) + 0.5f) / (float)bins[b];  L = lo + (hi - lo) * frac;
 *                   target = (key / L) * exposure;  if (min_auto != 0 && target < min_auto) target = min_auto;  likewise max_auto
 *   adaptation    metered frames are ordered by their vrt_render calls, whatever stream or frame set each ran on.  The first one
 *                 since the adaptation started takes E = target; later ones E = target when adapt == 1, else
 *                 E = E_prev + (target - E_prev) * adapt.  The adaptation starts at vrt_create, at a vrt_set_tone_map that
 *                 changes any byte of the setting, and at vrt_resize_output — not at a change of camera, world or settings.
 *                 Without VRT_TONE_AUTO, E = exposure.
 * E stays on the device: the blit reads it from the frame set's word, and nothing on the render or present path waits for it.
 * opts NULL or curve == VRT_TONE_OFF: off, the default — every frame, launch and allocation is what it is without this call.
 * VRT_ERR_INVALID_ARG: an unknown curve or flag, _reserved not 0, any float negative, NaN or infinite, percentile > 1000,
 * min_auto > max_auto when both are set, VRT_TONE_AUTO with VRT_TONE_OFF; with a curve, exposure == 0; with VRT_TONE_AUTO, key == 0
 * or adapt outside (0, 1].  VRT_ERR_STATE: a curve on a sharded, tile-major or multi-device context (they cannot present, or
 * assemble their frame elsewhere).  A refused call changes nothing.  A timed frame's GPU time includes the metering. */
#define VRT_TONE_OFF      0u   /* default: present as without the setting */
#define VRT_TONE_LINEAR   1u   /* exposure only, then the existing clamp */
#define VRT_TONE_REINHARD 2u   /* extended Reinhard, per channel */
#define VRT_TONE_FILMIC   3u   /* Narkowicz's ACES fit, per channel */
#define VRT_TONE_AUTO     1u   /* flags: exposure metered from every path frame */
#define VRT_TONE_GAMMA2   2u   /* flags: square-root encode behind the curve */
typedef struct vrt_tone_map {
    uint32_t curve;       /* VRT_TONE_* */
    uint32_t flags;       /* VRT_TONE_AUTO | VRT_TONE_GAMMA2 */
    float    exposure;    /* manual: the factor E.  AUTO: a compensation multiplied onto the metered value.  finite, > 0 */
    float    white;       /* REINHARD: the value mapped to 1; 0 = plain x / (1 + x).  finite, >= 0 */
    float    key;         /* AUTO: the value the metered luminance is brought to (suggested 0.18).  finite, > 0 */
    float    adapt;       /* AUTO: 1 = follow at once; (0, 1): share of the way taken per metered frame */
    float    min_auto, max_auto;   /* AUTO: bounds of the adapted exposure's target; 0 = none.  finite, >= 0, min <= max when both set */
    uint32_t percentile;  /* AUTO: 0..1000, the rank metered, in thousandths (suggested 500) */
    uint32_t _reserved[3];/* 0 */
} vrt_tone_map;           /* 48 B */
int vrt_set_tone_map(vrt_ctx *ctx, const vrt_tone_map *opts);

typedef struct vrt_tone_info {
    float    exposure;    /* E of the last mapped frame */
    float    target;      /* AUTO: what that frame metered, before adaptation */
    float    luminance;   /* AUTO: L (0 when nothing was counted) */
    uint32_t bin;         /* AUTO: the bin that holds the rank (0 when nothing was counted) */
    uint64_t counted, skipped;   /* AUTO: pixels in the histogram / left out of it */
    uint32_t frames;      /* metered frames since the adaptation last started, that frame included */
    uint32_t _reserved;
} vrt_tone_info;          /* 40 B */
/* The last mapped frame's exposure and, with VRT_TONE_AUTO, what it metered (without: the other fields are 0).  Synchronises.
 * VRT_ERR_STATE before the first mapped frame (and after a resize until the next one). */
int vrt_get_tone_info(vrt_ctx *ctx, vrt_tone_info *out);
/* The 256 bins of the last metered frame.  Synchronises.  VRT_ERR_STATE before the first metered frame (and after a resize
 * until the next one). */
int vrt_read_tone_histogram(vrt_ctx *ctx, uint32_t bins[256]);

/* Direct sunlight for VRT_MODE_PATH: next-event estimation towards the scene's one light.  ray_sky's sun is a disc of
 * dot(dir, sun_dir) > 0.99, which a random bounce rarely leaves the world through; with vrt_set_sun_light every hit of a path
 * sends a ray to the sun instead.  The primary modes ignore the setting and stay byte for byte what they are.  Build-defined,
 * and defined exactly — the body of ray_color's loop, in strict binary32, nothing contracted:
 *   1  mc and the emission term (vrt_write_emission) as without the setting: (mc * e) * thr
 *   2  the sun term, on every hit — the primary segment's and the last allowed segment's included — whose voxel is not 0 and
 *      not a liquid:
 *        so = pos + norm * bias per component (the bounce origin; the shadow ray's origin of VRT_MODE_PRIMARY_SHADOW)
 *        sd = normalize(sun_pos - f32(world.min) - so)
 *        c  = dot(norm, sd);  only if c > 0 (a zero normal or a NaN gives no ray): march ray_world(so, sd), start nudge included
 *        unoccluded = the march does not hit: liquids are passed, running out of steps counts as occluded, a ray that starts
 *        or ends outside the world is unoccluded
 *        if unoccluded:  k = settings.sun_intensity * strength;  w = k * c;  light.ch += (mc.ch * w) * thr.ch
 *      mc is the face-shaded colour (or the step-count grey), never the coat's colour
 *   3  everything behind it unchanged, in the order it has: the pass-through draw, the coat's draw, the direction, thr *= tint.
 *      The sun term draws nothing: the RNG stream, every path direction, the id words and vrt_read_steps' counts are those of
 *      the frame without the setting
 *   4  a segment other than the primary that misses takes ray_sky with add = +0.0f (the sky of a scene whose sun_intensity
 *      is 0): its surface received the sun in step 2, and the disc is not counted twice.  The primary segment's miss still
 *      shows the disc.  Specular glints of the sun are lost
 *   5  a sample's light is its terms in segment order — within a segment the emission term, then the sun term — the sky last;
 *      a frame's light is its samples' lights in sample order, divided by spp.  VRT_RENDER_ACCUMULATE keeps its identity (K
 *      frames of s spp are one frame of K * s spp, bit for bit); the denoiser's key and guide are unchanged
 *   6  vrt_stats.secondary_rays counts every sun ray marched as well; a stats frame's steps and node_visits include the sun
 *      marches; a timed frame's ms_secondary includes the sun launches
 * opts NULL or strength +0 / -0: off, the default — frames are byte for byte those of a context that never called this, the
 * same kernels run, and nothing is launched or allocated.  strength negative, NaN or infinite, flags or _reserved not 0, a
 * null context: VRT_ERR_INVALID_ARG; a refused call changes nothing.  A call that changes the setting (off is 16 zero bytes)
 * restarts the accumulation; one that does not, does not.  A multi-device context replicates the setting; a shard context keeps
 * its own. */
typedef struct {
    float    strength;      /* 0 = off (the default); the sun term's factor on settings.sun_intensity */
    uint32_t flags;         /* 0 */
    uint32_t _reserved[2];  /* 0 */
} vrt_sun_light;            /* 16 B */
int vrt_set_sun_light(vrt_ctx *ctx, const vrt_sun_light *opts);

/* Water for VRT_MODE_PATH: a surface that reflects, a body that absorbs.  Without the setting every segment of a path passes the
 * material table's liquids as if they were air, and all a frame keeps of a lake is VRT_ID_WATER in the id word.  The primary modes
 * ignore the setting and stay byte for byte what they are.  Build-defined, and defined exactly — per path segment with origin o
 * (world-local), direction d and throughput thr, in strict binary32, nothing contracted:
 *   1  wet or dry, decided afresh at the start of every segment, the primary's included (there is no per-path state): the segment
 *      is wet when the voxel at floor(o) is a liquid of the context's material table (ids >= 255 share entry 255).  The voxel is
 *      vrt_get_voxels' answer: 0 outside the world box (a NaN is outside), 0 where chunk_roots holds no chunk
 *   2  a dry segment is marched with the empty liquid set: a liquid voxel stops the ray like a solid, and the hit carries that
 *      voxel, its position and its face normal.  water_dist is 0
 *   3  a wet segment is marched with the table's liquid set, as every segment is without the setting.  w = its water_dist.  Before
 *      anything else of the segment — the sky's weight, the emission and sun terms, the lobes:
 *        thr.ch *= vexp_neg(absorb[ch] * w)        always, w == 0 included
 *      vexp_neg(t) = e^-t in + - *, floor and integer operations (csrc/both/water_math.h states it operation for operation; the
 *      host's vrth_water_transmittance compiles the same text): exactly 1 for t = 0, +0 from t = 128 on and already where e^-t
 *      rounds to it (t above about 103.98), a NaN for a NaN; results below 2^-126 are rounded to nearest even like any other
 *   4  the surface event — a dry segment's hit whose voxel is a liquid of the table:
 *        u = rng_next(rng)                          the event's only draw
 *        c = |dot(norm, d)|;  m = 1 - c;  m5 = (m * m) * (m * m) * m;  F = reflectance + (1 - reflectance) * m5
 *        u < F:      d'.k = d.k - 2 * norm.k * dot(norm, d);  o'.k = pos.k + norm.k * bias      (the bounce origin)
 *        otherwise:  d' = d;  o' = pos
 *      thr is unchanged.  The event gives off no emission, sends no sun ray and draws nothing else (no pass-through draw, no coat
 *      draw).  It costs one of the path's max_ray_bounces segments, as a pass through a translucent voxel does
 *   5  every other hit and every miss: the text of the frame without the setting, word for word — emission term, sun term
 *      (vrt_set_sun_light: its ray passes liquids and is not attenuated), pass-through draw, coat draw, direction, thr *= tint; a
 *      later miss of a sun-lit frame takes the sky without the disc
 *   6  the texel's id word is that of the primary segment's own march: a dry camera that looks at a lake gets the water voxel and
 *      its face (vrt_cast_rays picks the same voxel: liquids stop cast_ray), VRT_ID_WATER clear; a wet camera gets what it got
 *      before.  The denoiser's guide is taken from the same march, so key and guide agree: the guide of a lake seen from above is
 *      the water face's plane
 *   7  a sample's light is its terms in segment order, the sky last; a frame's, its samples' in sample order, / spp.
 *      VRT_RENDER_ACCUMULATE keeps its identity (K frames of s spp are one frame of K * s spp, bit for bit).  vrt_stats.
 *      secondary_rays counts a surface event's continuation as the bounce segment it is; vrt_set_denoise, vrt_set_tone_map, the
 *      emission, polish and translucency tables, shard and multi-device contexts compose
 * A water frame runs one lane = path launch per segment, one sample per chain, as a sun-lit frame does: the pool kernel's march
 * cells have the table's liquid set baked in.  Not built: refraction, the surface seen from below and total internal reflection (a
 * wet segment leaves the water silently), absorption along sun rays, caustics.
 * Does not compose yet: with the setting on, vrt_render of a VRT_MODE_PATH frame (max_ray_bounces > 0) while vrt_set_lamp_light or
 * vrt_set_camera_sampling is on returns VRT_ERR_STATE, names the pair in vrt_last_error, enqueues nothing and leaves the last frame
 * readable.
 * opts NULL or flags == 0: off, the default — frames are byte for byte those of a context that never called this, the same kernels
 * run, and nothing is launched, planned or allocated differently.  A null context, an absorb that is negative, NaN or infinite,
 * a reflectance outside [0, 1] or NaN (the floats are checked whatever flags says), a flag bit other than VRT_WATER_ON,
 * _reserved not 0: VRT_ERR_INVALID_ARG; a refused call changes nothing.  A call that changes the setting (off is 32 zero bytes; -0
 * is kept as +0) restarts the accumulation; one that does not, does not.  A multi-device context replicates the setting; a shard
 * context keeps its own. */
typedef struct {
    float    absorb[3];     /* absorption per voxel length, per channel: finite, >= 0 */
    float    reflectance;   /* the surface's reflectance at normal incidence, in [0, 1] */
    uint32_t flags;         /* 0 = off (the default), VRT_WATER_ON */
    uint32_t _reserved[3];  /* 0 */
} vrt_water_optics;         /* 32 B */
#define VRT_WATER_ON 1u
int vrt_set_water_optics(vrt_ctx *ctx, const vrt_water_optics *opts);

/* Refraction for water: Snell's law at the surface, and the surface seen from below.  The setting acts only in frames in which
 * vrt_set_water_optics is on (a water frame); with water optics off it is kept and changes nothing.  With it, a path that enters
 * the water is bent, and a wet segment that reaches the water's face from inside ends there: it is mirrored back (always, past the
 * critical angle: total internal reflection) or bent out into the air.  Build-defined, and defined exactly — in a water frame with
 * ior != 0, in strict binary32, nothing contracted, sqrt correctly rounded; eta = 1.0f / ior is formed once on the host;
 * normalize(v) = v / sqrt(dot(v, v)) is the path kernels' own; dot(a, b) = a.x * b.x + a.y * b.y + a.z * b.z, summed left to right;
 * bias = 0.002 (the bounce origin's):
 *   A  entering.  In the transmitted branch of the water contract's step 4 (u >= F), and only there, the direction is bent; the
 *      draw, F, the reflected branch and o' = pos are unchanged:
 *        dn = dot(norm, d);  c = |dn|;  nn.k = dn < 0 ? norm.k : -norm.k
 *        s2 = (eta * eta) * (1 - c * c);  ct = sqrt(1 - s2);  g = eta * c - ct
 *        d' = normalize(eta * d.k + g * nn.k)       per component a multiply, a multiply, an add
 *      With ior >= 1 the radicand is never negative.  A zero normal (a dry segment whose start nudge lands it in a liquid) gives
 *      d' = normalize(eta * d).  ior = 1 gives normalize(d): such a frame may differ from the frame without the setting in last bits
 *   B  the span walk, on every wet segment, ahead of the absorption of step 3.  cast_ray's DDA as vrt_cast_rays runs it
 *      (csrc/both/cast_dda.h: cast_setup(o, d), then cast_step), quirks included, from the segment's origin o along d; its first
 *      voxel is floor(o), the liquid that made the segment wet.  Up to max_span steps; after each, v is the voxel at the DDA's
 *      position as vrt_get_voxels answers (0 outside the world box, 0 where there is no chunk).  The walk ends at the first v that
 *      is not a liquid of the table; dist is that step's dist.  There is an underside event when the walk ended within max_span
 *      steps, v == 0, and dist is finite and >= 0.  In every other case — the walk ended on a solid voxel, it was still in liquid
 *      after max_span steps, dist was not finite — there is none, and the segment is word for word what it is with the setting off
 *   C  the underside event.  n.k = (float)(prev.k - m.k), m the air voxel and prev the voxel before it: the face's normal, back
 *      into the water.  x.k = o.k + d.k * dist (a multiply, then an add).  The segment's march is still the frame's own: a primary
 *      segment's id word, vrt_read_steps and a stats frame's steps, node_visits and hits are that march's, and the walk's steps are
 *      counted nowhere (the kernels may skip the march of a later segment that ends in an event where nothing counts it).  Nothing
 *      else of the march is used:
 *        thr.ch *= vexp_neg(absorb[ch] * dist)      in place of the march's water_dist
 *        on the path's last allowed segment: the path ends, nothing is drawn, no light is added
 *        u = rng_next(rng)                          the event's only draw
 *        dn = dot(n, d);  c = |dn|;  s2 = (ior * ior) * (1 - c * c)
 *        !(s2 < 1): total internal reflection (also for a NaN);  otherwise
 *            ct = sqrt(1 - s2);  mm = 1 - ct;  m5 = (mm * mm) * (mm * mm) * mm;  F = reflectance + (1 - reflectance) * m5
 *        reflected (total, or u < F):  d'.k = d.k - 2 * n.k * dn;  o'.k = x.k + n.k * bias          (back into the water)
 *        otherwise:  g = ior * c - ct;  d' = normalize(ior * d.k + g * n.k);  o'.k = x.k - n.k * bias  (out into the air)
 *      The event adds no emission, sends no sun ray and draws nothing else; thr is otherwise unchanged.  It costs one of the path's
 *      segments; vrt_stats.secondary_rays counts its continuation as the bounce segment it is.  The next segment decides wet or
 *      dry afresh from floor(o'), as every segment does
 *   D  everything else is the water contract's.  The sun term is unchanged: its ray passes liquids, unbent and unattenuated.  The
 *      sums, VRT_RENDER_ACCUMULATE's identity, the denoiser's key and guide (both from the primary segment's own march), tone
 *      mapping, the three tables, shard and multi-device contexts compose as they do for a water frame, and the pairs a water
 *      frame refuses (vrt_set_lamp_light, vrt_set_camera_sampling) are refused exactly as without the setting
 * A refracting frame is planned and launched as a water frame; its two trace launches run a pair of kernels of their own.  Still
 * not built: caustics, absorption along sun rays, dispersion.
 * opts NULL or ior +0 / -0: off, the default — frames are byte for byte those of a context that never called this, the same
 * kernels run, and nothing is launched, planned or allocated differently.  A null context, an ior that is NaN, negative, infinite,
 * or not 0 and outside [1, 4], max_span above 1024, flags or _reserved not 0: VRT_ERR_INVALID_ARG; a refused call changes nothing.
 * A call that changes the setting (off is 16 zero bytes; max_span 0 and 64 are the same setting) restarts the accumulation; one
 * that does not, does not.  A multi-device context replicates the setting; a shard context keeps its own. */
typedef struct {
    float    ior;           /* 0 = off (the default); otherwise the water's index of refraction relative to air, in [1, 4] */
    uint32_t max_span;      /* the unit voxels a wet segment's span walk may cross; 0 = 64; at most 1024 */
    uint32_t flags;         /* 0 */
    uint32_t _reserved;     /* 0 */
} vrt_water_refraction;     /* 16 B */
int vrt_set_water_refraction(vrt_ctx *ctx, const vrt_water_refraction *opts);

/* Haze for VRT_MODE_PATH: air that scatters light.  Without the setting the space between surfaces is a vacuum; with it every
 * segment of a path may end in a scatter event before it reaches what its march found, and a sun-lit frame sends a sun ray from
 * there: fog, aerial perspective, shafts of light.  The medium is homogeneous and fills the world box; its phase function is
 * isotropic.  The primary modes ignore the setting and stay byte for byte what they are.  Build-defined, and defined exactly — in
 * a haze frame (density != 0 and max_ray_bounces > 0), per path segment with origin o (world-local), direction d and throughput
 * thr, in strict binary32, nothing contracted, sqrt and division correctly rounded:
 *   1  the march is unchanged.  The segment is marched as the frame without the setting marches it: R.  The primary segment's id
 *      word, vrt_read_steps, the denoiser's key and guide, vrt_stats.hits and a stats frame's counts are that march's
 *   2  the distance draw.  u = rng_next(rng) on every segment, the primary and the last allowed one included, ahead of every other
 *      draw of the segment, whatever follows:
 *        uc = u < 1e-10f ? 1e-10f : u               (rng_next_u2's clamp)
 *        t = (-vlog(uc)) * inv                      inv = 1.0f / density, formed once on the host
 *      vlog is the path kernels' logarithm (csrc/both/haze_math.h states it operation for operation; the host's vrth_haze_distance
 *      compiles the same text)
 *   3  the segment's length in the haze, L:
 *        on R.hit (running out of steps is a hit, as in ray_world):  v.k = R.pos.k - o.k;  L = sqrt((v.x*v.x + v.y*v.y) + v.z*v.z)
 *        on a miss, the exit from the world box:  e.k = (world_max - o.k) / d.k where d.k > 0, (0.0f - o.k) / d.k where d.k < 0,
 *        +inf otherwise;  L = min(e.x, min(e.y, e.z)) with fminf's semantics        (vrth_haze_exit)
 *        L = 0 if any o.k is <= 0 or >= world_max or a NaN: the origin ray_world treats as outside
 *   4  the scatter event happens iff t < L (a NaN gives none).  x.k = o.k + d.k * t (a multiply, an add).  The march's hit is not
 *      used: no emission term, no sun ray of the hit, no pass-through or coat draw, no sky.
 *        thr'.ch = thr.ch * albedo[ch]
 *        if vrt_set_sun_light is on:  sd = normalize(sun_pos - f32(world.min) - x);  q = (sd.x*sd.x + sd.y*sd.y) + sd.z*sd.z;
 *          only if q > 0.5f (a zero or a NaN gives no ray): march ray_world(x, sd), start nudge included, exactly as a hit's sun
 *          ray; if unoccluded:  k = settings.sun_intensity * strength;  w = k * 0.25f;  light.ch += (albedo[ch] * w) * thr.ch
 *          with thr the throughput before the event (the isotropic phase function against the sun term's Lambert convention: k / 4).
 *          The ray is sent on the last allowed segment too
 *        d' = rng_next_dir(rng) (its six draws);  o' = x
 *      The event costs one of the path's max_ray_bounces segments; vrt_stats.secondary_rays counts its continuation as the bounce
 *      segment it is and its sun ray as a sun ray
 *   5  no event: behind the draw, the segment is word for word the segment of the frame without the setting — sun-lit, emissive,
 *      polished or translucent as that frame is.  A sun-lit frame's later misses take the sky without the disc; that covers the
 *      segment behind a scatter event, whose sun was sampled at the event
 *   6  a sample's light is its terms in segment order; a frame's, its samples' in sample order, / spp.  VRT_RENDER_ACCUMULATE keeps
 *      its identity (K frames of s spp are one frame of K * s spp, bit for bit).  vrt_set_denoise, vrt_set_tone_map, the emission,
 *      polish and translucency tables, shard and multi-device contexts compose as for a water frame
 * A haze frame runs one lane = path launch per segment, one sample per chain, as a sun-lit frame does.  Not built: height falloff,
 * an anisotropic phase function, haze along sun rays (they are not attenuated), a march cut short at t.
 * Does not compose yet: with the setting on, vrt_render of a VRT_MODE_PATH frame (max_ray_bounces > 0) while vrt_set_water_optics,
 * vrt_set_lamp_light or vrt_set_camera_sampling is on returns VRT_ERR_STATE, names vrt_set_haze and the other setter in
 * vrt_last_error, enqueues nothing and leaves the last frame readable.  With haze off the refusals that exist are what they are.
 * opts NULL or density +0 / -0: off, the default — frames are byte for byte those of a context that never called this, the same
 * kernels run, and nothing is launched, planned or allocated differently.  A null context, a density that is NaN, negative,
 * infinite, or not 0 and outside [2^-20, 64], an albedo outside [0, 1] or NaN (checked whatever density is), flags or _reserved
 * not 0: VRT_ERR_INVALID_ARG; a refused call changes nothing.  A call that changes the setting (off is 32 zero bytes; -0 is kept
 * as +0) restarts the accumulation; one that does not, does not.  A multi-device context replicates the setting; a shard context
 * keeps its own. */
typedef struct {
    float    density;       /* 0 = off (the default); extinction per voxel length */
    float    albedo[3];     /* per channel, in [0, 1]: what a scatter event keeps */
    uint32_t flags;         /* 0 */
    uint32_t _reserved[3];  /* 0 */
} vrt_haze;                 /* 32 B */
int vrt_set_haze(vrt_ctx *ctx, const vrt_haze *opts);

/* Camera sampling for VRT_MODE_PATH: a primary ray of its own for every sample — sub-pixel jitter (a box pixel filter, which
 * is what removes the stair steps of voxel edges as samples accumulate) and a thin lens (depth of field).  Without it every
 * sample of a pixel starts with the pixel's one ray.  The primary modes ignore the setting and stay byte for byte what they
 * are.  Build-defined, and defined exactly, in strict binary32, nothing contracted.  The setting is on when pixel_spread or
 * aperture is not 0:
 *   1  a sample's RNG is seeded as without the setting; ahead of everything else it takes four draws, u1, u2, u3, u4 = rng_next
 *      in that order — on every sample of every pixel, whichever of the two floats is 0
 *   2  fx = f32(px) + (u1 - 0.5) * pixel_spread,  fy = f32(py) + (u2 - 0.5) * pixel_spread;
 *      x = (fx * 2) / proj_size.x - 1,  y = (fy * 2) / proj_size.y - 1; the products with inv_proj_mat and inv_view_mat follow as
 *      in create_ray_from_screen;  d = normalize(w)
 *   3  aperture == 0 (a pinhole):  o' = origin = cam.pos - f32(world.min),  d' = d.  Otherwise
 *        r = aperture * sqrt(u3);  lx = r * cos2pi(u4);  ly = r * cos2pi(u4 + 0.75)    (cos2pi: the normal deviates' quadrant-and-
 *        polynomial cosine; its argument may pass 1)
 *        right.k = inv_view_mat[4k + 0],  up.k = inv_view_mat[4k + 1]  (k = 0, 1, 2: the images of eye-space x and y, as they are)
 *        F.k = origin.k + d.k * focus_distance;  o'.k = (origin.k + right.k * lx) + up.k * ly;  d' = normalize(F - o')
 *   4  the sample's primary segment is ray_world(o', d'), an ordinary segment: the start nudge, the test for lying outside the
 *      world.  A primary miss takes ray_sky(o', d') with the sun's disc (under vrt_set_sun_light too: later misses do not show
 *      it).  Everything behind the march is unchanged and in its order: emission term, sun term, pass-through draw, coat draw,
 *      direction, throughput.  A sample's light is its terms in segment order, the sky last; a frame's light is its samples'
 *      lights in sample order, divided by spp.  VRT_RENDER_ACCUMULATE keeps its identity (K frames of s spp are one frame of
 *      K * s spp, bit for bit): the four draws hang on the global sample index through the seed
 *   5  the id word, vrt_read_steps' primary counts, vrt_stats.hits and the denoiser's key and guide are those of the frame with
 *      the setting off: they come from the pixel's own pinhole ray, which the launch that holds the frame's first sample marches
 *      once more and shades nothing from.  A stats frame's steps, node_visits, primary_steps and primary_node_visits count that
 *      march and every sample's own primary march
 *   6  max_ray_bounces == 0 still gives zeros
 * opts NULL, or pixel_spread and aperture both +0 / -0: off, the default — frames are byte for byte those of a context that
 * never called this, the same kernels run, and nothing more is launched or allocated.  A null context, one of the three floats
 * negative, NaN or infinite, pixel_spread > 8, aperture != 0 with focus_distance == 0, flags != 0: VRT_ERR_INVALID_ARG; a refused
 * call changes nothing.  A call that changes the setting (off is 16 zero bytes; with aperture == 0 focus_distance is not
 * compared) restarts the accumulation; one that does not, does not.  A multi-device context replicates the setting; a shard
 * context keeps its own. */
typedef struct {
    float    pixel_spread;    /* width of the box pixel filter in pixels; 0 = every sample through the pixel's own ray */
    float    aperture;        /* lens radius in voxels; 0 = pinhole */
    float    focus_distance;  /* distance along each pixel's ray at which the image is sharp; read only when aperture != 0 */
    uint32_t flags;           /* 0 */
} vrt_camera_sampling;        /* 16 B */
int vrt_set_camera_sampling(vrt_ctx *ctx, const vrt_camera_sampling *opts);

/* Lamp light for VRT_MODE_PATH: next-event estimation towards the world's emissive voxels (vrt_write_emission).  A lamp of a
 * few voxels is found by a random bounce a handful of times in a thousand; with vrt_set_lamp_light every hit of a path sends a
 * ray to a point of a lamp face instead.  The primary modes ignore the setting and stay byte for byte what they are.
 *
 * The lamp list.  A lamp face is face f of a unit voxel p of the world with voxel id v for which emission[min(v,255)] != 0, v is
 * not 0 and not a liquid of the material table, and the unit voxel across the face is passable: air, a liquid, outside the
 * world box, or in a chunk whose chunk_roots entry is 0.  f = 2 * axis + side: 0 = -x, 1 = +x, 2 = -y, 3 = +y, 4 = -z, 5 = +z.
 * The list holds the lamp faces of the whole world by ascending depth-3 cell index (x fastest, as vrt_read_accel's grid), then
 * ascending u = (x&3) | (y&3)<<2 | (z&3)<<4 inside the cell, then ascending f; every unit voxel of a large leaf is looked at on
 * its own.  It is derived on the GPU from the derived tables, the liquid set and the emission table, on the stream of the frame
 * that needs it and without a host round trip, whenever one of the three changed since its last build; each frame set in
 * flight has a list of its own.  It is capped at 2^20 entries (VRT_LAMP_CAP, read by vrt_create, overrides the cap): a world
 * with more faces lists the first `cap` in order, and vrt_lamp_info.faces still counts them all.  N is the list's length.
 *
 * Build-defined, and defined exactly — the body of ray_color's loop on a hit, in a lamp-lit frame (strength != 0,
 * max_ray_bounces > 0), in strict binary32, nothing contracted:
 *   1  mc as without the setting
 *   2  the emission term (mc * e) * thr is added only while the path is direct: a path starts direct, stays direct through
 *      pass-throughs (vrt_write_translucency) and stops being direct at its first bounce; after that the lamps are counted by
 *      step 5 and not twice.  A lamp seen through a pane still shines
 *   3  the sun term (vrt_set_sun_light) unchanged, if the sun is on
 *   4  three draws u1, u2, u3 = rng_next, in that order, on every hit of every segment — the last allowed segment's included —
 *      whatever the voxel and whatever N is, ahead of the pass-through draw, the coat's draw and the direction's six draws
 *      (camera sampling's four draws stay first)
 *   5  the lamp term, only if the hit voxel is not 0 and not a liquid, and N > 0:
 *        so = pos + norm * bias                                  (the bounce origin, as the sun term's)
 *        j = min((uint32_t)(u1 * (float)N), N - 1);  L = list[j];  a = L.face >> 1;  s = L.face & 1
 *        q[a] = (float)L.pos[a] + (float)s;  the other two axes b < c:  q[b] = (float)L.pos[b] + u2;  q[c] = (float)L.pos[c] + u3
 *        v = q - so;  d2 = (v.x*v.x + v.y*v.y) + v.z*v.z;  ld = normalize(v)
 *        c = dot(norm, ld);  cl = s ? -ld[a] : ld[a]
 *        only if c > 0 && cl > 0 (a NaN gives no ray): march ray_world(so, ld), start nudge included
 *        unoccluded = the march hits AND (int)floor(hit pos) == L.pos on all three axes (liquids are passed; running out of
 *        steps counts as occluded)
 *        g = (c * cl) / d2;  if (max_geometry != 0 && g > max_geometry) g = max_geometry
 *        k = ((strength * emission[min(L.voxel,255)]) * 0.318309886f) * (float)N;  w = k * g
 *        lc = materials[min(L.voxel,255)].color with hit_color's face factors for face L.face in hit_color's order (x faces
 *        * 0.5, z faces * 0.7, face 2 * 0.2); show_step_count's grey is not applied to lc
 *        if unoccluded:  light.ch += ((mc.ch * lc.ch) * w) * thr.ch
 *   6  everything behind it unchanged and in its order
 *   7  within a segment: emission, sun, lamp.  A sample's terms go in segment order, the sky last; samples in sample order;
 *      / spp.  VRT_RENDER_ACCUMULATE keeps its identity.  The id words, vrt_read_steps' primary counts and the denoiser's key
 *      and guide are those of the frame with the setting off.  Mirror glints of lamps are lost, as the sun's are
 *   8  vrt_stats.secondary_rays counts the lamp rays marched; a stats frame's steps and node_visits include their marches; a
 *      timed frame's ms_secondary includes their launches
 * With scatter = 1 the bounce normalize(norm + rng_next_dir) is cosine-weighted, a face has area 1 and is picked with
 * probability 1 / N: at strength 1 the term is the expectation of the emission term the next segment would have added.
 * opts NULL or strength +0 / -0: off, the default — frames are byte for byte those of a context that never called this, the
 * same kernels run, and nothing is launched, built or allocated.  A null context, strength or max_geometry negative, NaN or
 * infinite, flags or _reserved not 0: VRT_ERR_INVALID_ARG; a refused call changes nothing.  A lamp-lit path frame of a world
 * that keeps no derived tables: VRT_ERR_STATE, nothing enqueued.  A call that changes the setting restarts the accumulation.
 * A multi-device context replicates the setting and every device builds its own identical list; a shard context keeps its own. */
typedef struct {
    float    strength;      /* 0 = off (the default); 1 = matched to what a diffuse path finds by chance */
    float    max_geometry;  /* 0 = no clamp; otherwise the geometry factor g is clamped to it (fireflies in corners) */
    uint32_t flags;         /* 0 */
    uint32_t _reserved;     /* 0 */
} vrt_lamp_light;           /* 16 B */
int vrt_set_lamp_light(vrt_ctx *ctx, const vrt_lamp_light *opts);

typedef struct { uint16_t pos[3]; uint16_t voxel; uint32_t face; uint32_t _reserved; } vrt_lamp;   /* 16 B, world-local voxel coordinates */
typedef struct { uint32_t listed; uint32_t cap; uint64_t faces; uint32_t builds; float last_build_ms; } vrt_lamp_info;   /* 24 B */
/* The list the last lamp-lit frame used: its length, the cap, the world's lamp faces (saturating at 2^64 - 1), the whole builds
 * of that frame set's list so far and what the last one took on the GPU.  Synchronises.  VRT_ERR_STATE before the first
 * lamp-lit frame. */
int vrt_get_lamp_info(vrt_ctx *ctx, vrt_lamp_info *out);
/* ... and its first min(cap, listed) entries into out (out may be NULL with cap 0); *n = listed.  Synchronises. */
int vrt_read_lamps(vrt_ctx *ctx, vrt_lamp *out, uint32_t cap, uint32_t *n);

/* Block until everything enqueued on the context's stream has finished. */
int vrt_synchronize(vrt_ctx *ctx);

/* Copy the last frame to host memory (synchronises). Any pointer may be NULL.
 * rgb: width*height*3 f32 row-major; ids: width*height id words; rgba8: what textureStore would have
 * put in the reference's rgba8unorm texture (ray_tracer.wgsl:179).
 * With shard_count > 1 only this context's tiles are defined; the rest reads as zero. */
int vrt_read_output(vrt_ctx *ctx, float *rgb, uint32_t *ids, uint8_t *rgba8);

/* ScreenShader::encode_pass (shader.rs:273-293, main.rs:454) into host memory: for every pixel of a screen_w x
 * screen_h target — any size: the reference renders its 1080 rows into whatever the window is (main.rs:175,206-210) —
 * fs_main of screen_shader.wgsl:43-65: the rgba8unorm result texture sampled at the pixel centre through the reference's
 * sampler (texture.rs:31-44: ClampToEdge, mag Nearest / min Linear, lod clamped to [1, 1] — a level of detail of 1
 * selects the minification filter, so the sample is bilinear at every window size and the texel itself at 1:1) blended
 * with the crosshair, written as unorm8 RGBA, screen_w*screen_h*4 bytes (synchronises).  Whole-frame contexts only. */
int vrt_present(vrt_ctx *ctx, const vrt_crosshair *crosshair, uint32_t screen_w, uint32_t screen_h, uint8_t *rgba8);

/* The same, left on the device, and asynchronous: the blit is enqueued behind the frame it presents, on that frame's stream
 * (the caller's after vrt_set_stream), so a host that draws and presents frame after frame (main.rs:452-454) keeps its
 * frames in flight — nothing is copied to the host and nothing waits.  *rgba8_device points at screen_w*screen_h*4 bytes of
 * the screen buffer of the frame's set: valid until the present of the frame vrt_set_frames_in_flight frames later (the
 * next one with one frame in flight) — with a declared presentation (vrt_set_presentation) until that frame is RENDERED: its own launch
 * stores into the buffer — or vrt_destroy.  For a host that hands the image to its window system through GPU
 * interop (a 1080p frame is 8 MB of PCIe traffic otherwise).  vrt_synchronize before reading it from another stream. */
int vrt_present_device(vrt_ctx *ctx, const vrt_crosshair *crosshair, uint32_t screen_w, uint32_t screen_h, void **rgba8_device,
                       uint64_t *bytes);

/* The blit folded into the frame's own launch.  The reference's compute pass stores rgba8unorm (ray_tracer.wgsl:179) and its
 * blit follows in the same submission, every frame (main.rs:452-454); here the frame is a 16-byte parity texel per pixel and
 * vrt_present* a second launch that reads it again.  vrt_set_presentation declares what the frames that follow will be presented
 * with: while the window has the texture's size, that size is whole 8x8 tiles, every pixel samples its own texel's centre (to
 * 1e-4 of a texel: 1920x1080, 2560x1440, 3840x2160, ... — found once per size) and every tap of the pixels the crosshair can reach
 * lies in the pixel's own tile, a plain primary / primary + shadow frame of a whole-frame context ALSO stores the window's
 * pixel — fs_main's byte: the texel quantised, the crosshair blended in — into the screen buffer of its frame set, and
 * vrt_present_device / vrt_present with the declared crosshair and size after such a frame launch nothing.  Every other frame,
 * window size or crosshair takes the blit's own launch as before: the declaration never changes a result, only who stores it.
 * flags: VRT_PRESENT_SKIP_TEXELS — such a frame stores the window's pixel ONLY (4 bytes per pixel written instead of 20): a
 * host that presents and never reads back.  vrt_read_output, vrt_present* with another crosshair or size and vrt_assemble
 * sources then find no texels for that frame and return VRT_ERR_STATE.  crosshair NULL: off (the default). */
#define VRT_PRESENT_SKIP_TEXELS 1u
int vrt_set_presentation(vrt_ctx *ctx, const vrt_crosshair *crosshair, uint32_t screen_w, uint32_t screen_h, uint32_t flags);

int vrt_get_stats(vrt_ctx *ctx, vrt_stats *out);

/* New relative to the reference: what ISSUING a frame costs the host, averaged over the vrt_render calls since the previous call
 * of this function (wall-clock microseconds of the calling thread; nothing here waits for a device).  A multi-GPU frame period
 * cannot fall below it, and it cannot be read off a frame loop's own clock once the loop is ahead of its GPUs.  For a multi-device
 * context: the calling thread issues for device_ids[0] while one thread per other device issues for that device (all on the
 * calling thread when the ordinals repeat — a one-GPU rehearsal — or with VRT_GROUP_THREADS=0), then waits for them, then
 * enqueues the waits for the messages, the assembly and an event. */
typedef struct {
    uint32_t frames;            /* vrt_render calls averaged (0: none since the previous call; every figure below is then 0) */
    uint32_t devices;           /* 1, or the devices of a multi-device context */
    uint32_t issuing_threads;   /* threads issuing beside the caller (0: the caller issues for every device in turn) */
    uint32_t _reserved;
    double render_us;           /* the whole vrt_render call */
    double root_issue_us;       /* multi-device: the caller's own issue for device_ids[0] */
    double shard_issue_us_mean; /* ... one other device's issue (its thread's job, or its turn on the caller), mean over devices */
    double shard_issue_us_max;  /* ... the slowest of them, per frame */
    double join_wait_us;        /* ... the caller waiting for the issuing threads after its own issue (0 without threads) */
    double tail_us;             /* ... behind the join: [the stream waits for the messages,] the assembly's launch, the event record */
    double message_waits_us;    /* ... of tail_us, the N - 1 stream waits for the messages when the caller makes them (no issuing threads:
                                 * with threads every thread makes its own, inside its job) */
} vrt_issue_profile;
int vrt_get_issue_profile(vrt_ctx *ctx, vrt_issue_profile *out);

/* Self-test of the kernels' exact-arithmetic shortcuts (csrc/vrt_march.h: division and square root without the general
 * case's scaling and special-value handling, taken when every operand's magnitude is in [2^-30, 2^30]): n pseudo-random
 * operand sets (seed) on `device`, each computed both ways; *mismatches = results whose bits differ (0 on a correct
 * build).  The composites choose their form per wave of 64 consecutive sets: seven waves of eight lie wholly in the band
 * (its two ends included) and run the refined form against the general text, the eighth holds the sets outside it.
 * Diagnostic only; no context needed. */
int vrt_selftest_exact_math(int32_t device, uint32_t n, uint32_t seed, uint64_t *mismatches);

/* The values themselves: what the kernels' exact-arithmetic functions return for operands the caller chose, for a
 * reference that is not the GPU.  Diagnostic only; no context needed.  The kernel calls the functions the frame kernels
 * call (csrc/vrt_march.h, vrt_path_common.h).
 *   Operand set i runs on lane i % 64 of wave i / 64, and lanes past n are inactive: several of these functions choose
 *   their form per wave (one ballot), so THE CALLER COMPOSES WHOLE WAVES — what set i returns may depend on sets
 *   64 * (i / 64) .. 64 * (i / 64) + 63.  Words are 32-bit patterns (floats by their bits), in planes of n:
 *   word k of set i is in[k * n + i], result word k is out[k * n + i].  `flag` is 1 when the set's wave took the refined
 *   form, from the predicate and constants the function itself uses.
 *     op                       in                 out
 *     VRT_MATH_DIV             n, d               div_refined(n, d, rcp_refined(d)): n / d for d inside the band, n inside it or +-0
 *     VRT_MATH_SQRT            x                  sqrt_banded(x)
 *     VRT_MATH_UNIT_STEPS      x, y, z            unit_steps: x, y, z, flag
 *     VRT_MATH_NORMALIZE       x, y, z            normalize_wave: x, y, z, flag
 *     VRT_MATH_LENS_DIV        n, d               the lens ray's divide (lens_div), flag
 *     VRT_MATH_LENS_SQRT       x                  the lens ray's square root (lens_sqrt_of), flag
 *     VRT_MATH_RNG_NEXT        state              state after the draw, the uniform
 *     VRT_MATH_RNG_NEXT_U2     state              state after the draw, the uniform clamped to 1e-10
 *     VRT_MATH_LOG_BANDED      x                  vlog_t<true>(x) (what the kernels call: vlog)
 *     VRT_MATH_LOG_GENERAL     x                  vlog_t<false>(x)
 *     VRT_MATH_COS2PI          u                  vcos2pi(u)
 *     VRT_MATH_RNG_DIR         state              state after the six draws, x, y, z, flags: bit 0 the three square roots',
 *                                                 bit 1 the normalisation's
 *     VRT_MATH_TRUNC2I         x                  trunc2i(x)
 *     VRT_MATH_FLR2I           x                  flr2i(x)
 *     VRT_MATH_ABS_MUL         a, b               |a| * b
 *     VRT_MATH_MIN3_F32        a, b, c            min3_f32(a, b, c)
 *     VRT_MATH_MIN3_BITS       a, b, c            min3_u32(a - 1, b - 1, c - 1) + 1 (the step's branch tree on bit patterns)
 *     VRT_MATH_BFI             mask, a, b         (mask & a) | (~mask & b)
 *     VRT_MATH_LOW_BITS        a, b               low_bits_of<3>, <7>, <15>, <31>(a, b)
 *     VRT_MATH_OR_AND          a, b, c            a | (b & c)
 *     VRT_MATH_EXP_NEG         a, w               vexp_neg(a * w): vrt_set_water_optics' transmittance of absorb a over water_dist w,
 *                                                 the product formed in binary32 as the kernels form it (csrc/both/water_math.h)
 *     VRT_MATH_MAD_I24         a, b, c            mad_i24(a, b, c); b is a scalar operand: every set of a wave uses the b of
 *                                                 the wave's first set
 * Returns VRT_ERR_INVALID_ARG, and writes nothing, for a null pointer, n == 0, n > VRT_MATH_MAX_SETS or an unknown op. */
#define VRT_MATH_DIV 0u
#define VRT_MATH_SQRT 1u
#define VRT_MATH_UNIT_STEPS 2u
#define VRT_MATH_NORMALIZE 3u
#define VRT_MATH_LENS_DIV 4u
#define VRT_MATH_LENS_SQRT 5u
#define VRT_MATH_RNG_NEXT 6u
#define VRT_MATH_RNG_NEXT_U2 7u
#define VRT_MATH_LOG_BANDED 8u
#define VRT_MATH_LOG_GENERAL 9u
#define VRT_MATH_COS2PI 10u
#define VRT_MATH_RNG_DIR 11u
#define VRT_MATH_TRUNC2I 12u
#define VRT_MATH_FLR2I 13u
#define VRT_MATH_ABS_MUL 14u
#define VRT_MATH_MIN3_F32 15u
#define VRT_MATH_MIN3_BITS 16u
#define VRT_MATH_BFI 17u
#define VRT_MATH_LOW_BITS 18u
#define VRT_MATH_OR_AND 19u
#define VRT_MATH_MAD_I24 20u
#define VRT_MATH_EXP_NEG 21u
#define VRT_MATH_OPS 22u
#define VRT_MATH_MAX_SETS (1u << 26)
int vrt_selftest_math_values(int32_t device, uint32_t op, uint32_t n, const uint32_t *in, uint32_t *out);

/* New relative to the reference: the lookup tables the default march derives on the device from the node pool
 * and chunk_roots (brought up to date before the next frame: only the chunks a vrt_write_nodes range or a changed
 * vrt_write_chunk_roots slot touched, the whole world after a resize or a write that touches many chunks; DESIGN.md §HBM
 * layout).  `available` = 0 while a rebuild is pending or when the world is too large for them (variant 0 then runs
 * as variant 2).  While edits arrive every frame set in flight keeps its own copy of the tables, brought up to date on its
 * own stream with the chunks dirtied since its last frame (an edit then does not wait for the frame in flight); the
 * figures below are those of the copy the last frame used, vrt_read_accel returns the first copy, brought up to date. */
typedef struct {
    uint32_t available;
    uint32_t world_size_chunks;
    uint64_t cells;        /* depth-3 cells in the grid: (8S)^3, 4 B each (+ a zero border on the device) */
    uint64_t bricks;       /* bricks of the pool in use (64 x 2 B each): every chunk's region — its split cells plus slack
                            * for edits — and the regions of chunks that outgrew theirs */
    uint64_t bytes;
    uint32_t builds;       /* whole-world builds since vrt_create (first frame, resized / recentred grid) */
    float last_build_ms;   /* hipEvent time of the last whole-world build */
    uint32_t chunk_builds; /* chunks rebuilt alone since vrt_create: a vrt_write_nodes range or a changed chunk_roots slot
                            * rebuilds only the chunks it touches, stream-ordered, with no host round trip (every copy of the
                            * tables rebuilds every dirtied chunk once: the count of the copy that has rebuilt most) */
    uint32_t ordered_frames; /* (not about the tables) frames since vrt_create whose tiles were launched longest first: one-frame-at-a-time
                            * contexts, a view at rest or a view a camera step away from the frame before */
} vrt_accel_info;
int vrt_get_accel_info(vrt_ctx *ctx, vrt_accel_info *out);

/* Copy the tables to host memory for inspection (synchronises): grid[cells] entries, x-major over the whole world
 * (lo = leaf size - 1; air leaf: 0xFF800000 | lo; other leaf: voxel << 16 | lo; split depth-3 cell: 0x80000000 | brick * 64 < 0xFF800000),
 * bricks[bricks * 64] entries ((x&3) | (y&3) << 2 | (z&3) << 4 inside the cell; voxel << 1 | lo, lo = 1 for a size-2
 * leaf).  Either pointer may be NULL. */
int vrt_read_accel(vrt_ctx *ctx, uint32_t *grid, uint16_t *bricks);

/* The march cells the path trace's bounce launches read (one 16-byte entry per depth-3 cell: the cell grid's entry, the
 * size-2 mask of a split cell — bit (u >> 1) & 31, u = (x&3) | (y&3) << 2 | (z&3) << 4 —, and 64 bits "a ray passes voxel
 * u": air, or a liquid of the material table they were built with), gathered through their chunk directory and blocks
 * into cells[(8S)^3][4], x-major over the whole world, for inspection (synchronises).  *direct = 1 when the world is small
 * enough to be kept without a directory.  VRT_ERR_STATE when the tables are not up to date or this world keeps none. */
int vrt_read_march_cells(vrt_ctx *ctx, uint32_t *cells, uint32_t *direct);

/* The sun marks (docs/NUMERICS.md "Lit stops"): a primary + shadow frame of the default march stops a shadow ray at a cell from
 * which every ray towards the sun leaves the world through air; the marks live in the cell grid's air-leaf entries (which
 * vrt_read_accel returns without them) and are made again, lazily, when the tables or the sun's position changed and have then stood
 * still for four frames (frames in between trace their shadow rays to the end, as a context without marks does) — not when equal
 * settings are rewritten.  *passes: lit passes launched so far; *min_leaf: the smallest leaf (in voxels) the last such frame's marks
 * cover, 0 when it had none (sun inside the world or too low beside it, world too large for the step budget, VRT_SUN_MARKS=0);
 * *lit_trips: the wave trip count up to which a mark stops a ray; lit[(8S)^3], x-major over the whole world: 1 for a lit cell of the
 * table set the last frame used (synchronises).  Every pointer may be NULL. */
int vrt_get_sun_marks(vrt_ctx *ctx, uint32_t *passes, uint32_t *min_leaf, uint32_t *lit_trips, uint8_t *lit);

/* The voxel marks, for inspection (docs/NUMERICS.md "Lit stops", the voxels of split cells): with every lit pass a table set also
 * gets a copy of its brick pool in which the air voxels of split cells that see lit cells through air carry a mark, and the shadow
 * rays of such a frame read that copy (VRT_LIT_VOXELS=0: they never do; vrt_read_accel returns the bricks themselves as ever).
 * *passes: such passes launched so far; *layers: the voxel layers a voxel's walk may take, of the last such frame, 0 when it read
 * the plain bricks; *lit_trips: the wave trip count up to which a voxel's mark stopped a ray of that frame (vrt_get_sun_marks'
 * less the voxel marks' step budget; a cell's mark goes on stopping it up to vrt_get_sun_marks' own); lit[(32S)^3], x-major over
 * the whole world's voxels: 1 for a voxel that holds the mark in the copy the table set of the last frame was last given, read from
 * the copy itself (synchronises).  A world that holds the mark's voxel id in a brick gets a copy without marks, and its frames go
 * back to the plain bricks — from the first frame that finds that pass over, which differs from run to run: the frames are the same
 * bytes either way, *layers of the frames in between is K or 0.  Every pointer may be NULL. */
int vrt_read_lit_voxels(vrt_ctx *ctx, uint32_t *passes, uint32_t *layers, uint32_t *lit_trips, uint8_t *lit);

/* The dark voxel marks, for inspection (docs/NUMERICS.md "Dark stops", the voxels of split cells): where a pass makes the copy of the
 * brick pool above, the air voxels of split cells from which every ray towards the sun meets solid voxels, or cells with the dark
 * mark below, within a few voxel layers hold a solid voxel id (0x7FFE) in the copy, and a shadow ray that reads it there is
 * occluded (VRT_DARK_VOXEL_LAYERS: the voxel layers a voxel's walk may take; 0: no such marks).  Like the dark marks they depend on
 * which materials are liquids.  *passes: such passes launched
 * so far; *layers: those layers of the copy the last frame's shadow rays read, 0 when it held no such marks or the frame read the
 * plain bricks; dark[(32S)^3], indexed like vrt_read_lit_voxels' lit: 1 for a voxel that is air in the bricks and holds the mark in
 * the copy (synchronises).  vrt_read_accel returns the bricks themselves as ever.  Every pointer may be NULL. */
int vrt_read_dark_voxels(vrt_ctx *ctx, uint32_t *passes, uint32_t *layers, uint8_t *dark);

/* The dark marks (docs/NUMERICS.md "Dark stops"): behind every lit pass the all-air cells from which every ray towards the sun meets
 * a closed layer of solid voxels are marked too, and a shadow ray of such a frame that stands in one stops there as occluded
 * (VRT_DARK_MARKS=0: no such marks; VRT_DARK_DEPTH: the layers a cell's corridor is walked over).  The marks depend on which
 * materials are liquids: a change of the liquid set makes them again, like a moved sun.  *passes: dark passes launched so far; *count:
 * the dark cells of the table set the last frame used; *used: 1 when that frame's shadow rays stopped at them; dark[(8S)^3], indexed
 * like vrt_get_sun_marks' lit: 1 for a dark cell (count and dark synchronise).  Every pointer may be NULL. */
int vrt_get_dark_marks(vrt_ctx *ctx, uint32_t *passes, uint32_t *count, uint32_t *used, uint8_t *dark);

/* The trips the last frame that noted them took per tile (longest tiles first, above: a context that renders one frame at a time
 * notes them on the second plain frame of a view at rest): cost[tiles], the wave's trips through its primary and its shadow march
 * loop; cost[t] is tile t of this context's tiles, counted row by row over the screen's 8 x 8 tiles (a sharded context: its own tiles in that
 * order), whatever order the frame launched them in (synchronises).  VRT_ERR_STATE when no frame has noted any. */
int vrt_read_tile_cost(vrt_ctx *ctx, uint32_t *cost);

/* The order the next frame of this view launches its tiles in: order[tiles], the t-th wave of the launch takes tile order[t] (numbered
 * as vrt_read_tile_cost numbers them).  *dilated = 0 for the exact order of a view at rest — tiles by descending class
 * min(cost >> 1, 63), screen order within a class —, 1 for a moving view's order of 4 x 4-tile blocks by the largest cost within
 * VRT_TILE_ORDER_RADIUS blocks (may be NULL).  Synchronises.  VRT_ERR_STATE while the context holds no order: before a frame has made
 * one, with more than one frame in flight, after a resize, under VRT_TILE_ORDER=0.  Diagnostic only. */
int vrt_read_tile_order(vrt_ctx *ctx, uint32_t *order, uint32_t *dilated);

/* Self-test of the kernels that make those orders, on costs of the caller's choosing: cost[tiles_x * tiles_y] goes to `device`,
 * order[tiles_x * tiles_y] comes back (0xFFFFFFFF where the kernels wrote nothing).  radius < 0: the exact order, as a view at rest
 * gets it (tiles_x * tiles_y tiles in a row); radius 1..6: the block order dilated over that many blocks.  The launchers, class
 * width and thread count are the ones a frame uses.  VRT_ERR_OUT_OF_RANGE, nothing written, for a frame the block order refuses (more
 * than 8 192 blocks, more than 255 blocks a side, radius above 6) and for more than 2^28 tiles; a null pointer, a zero size or radius 0: VRT_ERR_INVALID_ARG.
 * Diagnostic only; no context needed. */
int vrt_selftest_tile_order(int32_t device, const uint32_t *cost, uint32_t tiles_x, uint32_t tiles_y, int32_t radius, uint32_t *order);

/* Per-pixel march-loop iteration counts of the last frame (primary | shadow << 16); the frame must
 * have been rendered with opts.stats = 1.  Numeric twin of the reference's F2 step-count heat-map
 * (main.rs:368-370, ray_tracer.wgsl:311-314). */
int vrt_read_steps(vrt_ctx *ctx, uint32_t *steps);

/* ---- world queries ---- */

/* The client's voxel pick (clientdesktop/src/main.rs:320-325): common::math::cast_ray (common/src/math.rs:153-226) with
 * collides(p) = world.get_voxel(p) is a non-empty voxel (client/src/world.rs:352-357), batched, one ray per lane, bit for bit.
 * "Collides": p lies inside [min, min + 32 * size_in_chunks) of the context's vrt_world_data on every axis, its chunk's
 * chunk_roots entry is not 0 (0 = no chunk) and the leaf find_node reaches there holds a voxel other than 0 (liquids collide).
 * The DDA is the reference's in strict binary32, quirks included: a component of dir that is zero or -0 makes its unit step
 * NaN or inf, ties take the y branch, a NaN or negative max_dist takes no step.  Where the reference would loop forever or
 * overflow i32 the query is REJECTED instead of run: max_dist +inf or above 2^20, a start component that is not finite or
 * whose magnitude is 2^24 or more.  Nothing else is rejected. */
typedef struct {
    float start[3];
    float max_dist;
    float dir[3];
    uint32_t _reserved;
} vrt_ray_query;  /* 32 B */

#define VRT_RAY_MISS 0u
#define VRT_RAY_HIT 1u
#define VRT_RAY_REJECTED 2u
typedef struct {
    int32_t pos[3];   /* HitResult.pos: the voxel hit */
    int32_t face[3];  /* HitResult.face: the voxel before it minus pos (the face the ray entered through) */
    float dist;       /* the DDA's dist at the hit, inf included; a NaN is stored as 0x7FC00000 (f32::NAN: the sign and payload
                       * of a NaN that a division makes are the platform's — x86 makes 0xFFC00000 — not the reference's) */
    uint32_t status;  /* VRT_RAY_*; every other field is 0 for a miss or a rejected query */
} vrt_ray_hit;  /* 32 B */

/* n queries from host memory, n results into host memory.  Ordered on the context's stream (vrt_set_stream) behind every
 * earlier call — a cast sees every vrt_write_* before it, with no frame in between — and waits for its own work only.  A cast
 * changes nothing a frame left behind (vrt_read_output, vrt_present*, vrt_get_stats).  n = 0 does nothing.  A multi-device
 * context casts on device_ids[0]. */
int vrt_cast_rays(vrt_ctx *ctx, const vrt_ray_query *queries, uint32_t n, vrt_ray_hit *out);
/* The same with device memory (n vrt_ray_query in, n vrt_ray_hit out, 4-byte aligned), asynchronous on the context's stream. */
int vrt_cast_rays_device(vrt_ctx *ctx, const void *queries_device, uint32_t n, void *out_device);

/* The client's collisions (clientdesktop/src/main.rs:316-319: player.update(&moves, |bb| world.get_collisions_w(bb, &voxels))):
 * clip_aabb_movement (client/src/player.rs:202-244) over ClientWorld::get_collisions_w (client/src/world.rs:369-391) and
 * Aabb::expand / translate / clip_{y,x,z}_collide (common/src/math.rs:18-126), batched, one box per lane, in strict binary32,
 * every component of the answer the reference's bits.
 * A voxel is a world box [p, p + 1] when it is SOLID: materials[min(v, 255)].is_empty == 0 && .is_liquid == 0 of the context's
 * material table (Material::construct fills both from the voxel's state, graphics/mod.rs:38-46) — liquids do not collide here,
 * unlike in vrt_cast_rays.  Outside the world box, or in a chunk whose chunk_roots entry is 0, get_voxel is Err and v is
 * Voxel::EMPTY (0), looked up in the table like any other voxel.
 * The boxes of Aabb b are gathered as get_collisions_w does: for x in floor(b.from.x)..ceil(b.to.x) { for y { for z, and the
 * clipping loop takes them in that order (y, then x, then z against the unmoved box, EPSILON = 0.00001): the answer is the
 * sequential loop's, quirks included — a box that rests on the floor and moves down is answered with +1e-5, not 0.
 * flags & VRT_BOX_AUTOJUMP is clip_aabb_movement's autojump (Player::update passes true); other bits are ignored.
 * A query is REJECTED instead of run in two cases, and only then: one of its nine floats is not finite or has a magnitude of
 * 2^23 or more (every sum of expand and translate then stays below 2^24, where the casts to i32 and p as f32 + 1.0 are exact);
 * or the first gather's range, (ceil(to) - floor(from)) multiplied over the axes of from/to expanded by mv, holds more than
 * VRT_BOX_MAX_VOXELS voxels (the reference would allocate without bound; the second gather's range is the same size within one
 * layer of y). */
typedef struct {
    float from[3];   /* Aabb.from */
    uint32_t flags;  /* VRT_BOX_AUTOJUMP */
    float to[3];     /* Aabb.to */
    uint32_t _r0;
    float mv[3];     /* the movement asked for (Player::update: frame_vel) */
    uint32_t _r1;
} vrt_box_query;  /* 48 B */
#define VRT_BOX_AUTOJUMP 1u
#define VRT_BOX_MAX_VOXELS 4096u

#define VRT_BOX_MOVED 0u    /* ran; mv = mv_clipped */
#define VRT_BOX_REJECTED 2u /* every other field is 0 */
#define VRT_BOX_CLIPPED_X 1u /* vrt_box_move.flags: mv_clipped != mv on that axis after the first pass (!eq, -0 == 0) */
#define VRT_BOX_CLIPPED_Y 2u
#define VRT_BOX_CLIPPED_Z 4u
#define VRT_BOX_STEPPED_UP 8u /* the autojump was taken: mv.y = clipped y + 1.0, mv.x / mv.z are the second pass's */
typedef struct {
    float mv[3];       /* clip_aabb_movement's result */
    uint32_t status;   /* VRT_BOX_MOVED or VRT_BOX_REJECTED */
    uint32_t flags;    /* VRT_BOX_CLIPPED_* | VRT_BOX_STEPPED_UP */
    uint32_t boxes[2]; /* boxes[p]: the solid voxels pass p gathered (boxes[1] = 0 when the second pass did not run) */
    uint32_t _reserved;
} vrt_box_move;  /* 32 B */

/* n queries from host memory, n results into host memory; ordering and scope are vrt_cast_rays's: on the context's stream behind
 * every earlier call — a clip sees every vrt_write_nodes, vrt_write_chunk_roots and vrt_write_materials before it, with no frame
 * in between — waiting for its own work only, and leaving everything a frame left behind (vrt_read_output, vrt_present*,
 * vrt_get_stats, the accumulation) as it was.  n = 0 does nothing.  A multi-device context answers on device_ids[0]; a sharded
 * context holds the whole world and answers alone. */
int vrt_clip_moves(vrt_ctx *ctx, const vrt_box_query *queries, uint32_t n, vrt_box_move *out);
/* The same with device memory (n vrt_box_query in, n vrt_box_move out, 4-byte aligned), asynchronous on the context's stream. */
int vrt_clip_moves_device(vrt_ctx *ctx, const void *queries_device, uint32_t n, void *out_device);

/* ClientWorld::get_voxel (client/src/world.rs:352-357), batched, one position per lane: check_bounds — the position lies inside
 * [min, min + 32 * size_in_chunks) of the context's vrt_world_data on every axis, else VRT_VOXEL_OUT_OF_BOUNDS — then the chunk —
 * a chunk_roots entry of 0 is "no chunk", VRT_VOXEL_NO_CHUNK, as in vrt_cast_rays — then the voxel of the leaf find_node reaches.
 * Any int32 coordinate is legal: the box test is made on unsigned differences and nothing overflows.  (The reference's own
 * check_bounds lets the 31 voxels past each far face through — max_voxel is the last voxel of the chunk after the grid — and
 * then finds no chunk there: vrth_world_get_voxel answers NoChunk where this call answers OUT_OF_BOUNDS.  Either way no voxel.) */
#define VRT_VOXEL_OK 0u
#define VRT_VOXEL_OUT_OF_BOUNDS 1u /* SetVoxelErr::PosOutOfBounds, the number vrth_world_get_voxel returns */
#define VRT_VOXEL_NO_CHUNK 3u      /* SetVoxelErr::NoChunk */
typedef struct {
    uint16_t voxel;  /* 0 unless status == VRT_VOXEL_OK */
    uint16_t status; /* VRT_VOXEL_* */
} vrt_voxel_at;  /* 4 B */

/* n positions (n x 3 int32: x, y, z in world voxel coordinates) from host memory, n results into host memory.  Ordering and
 * scope are vrt_cast_rays's: on the context's stream behind every earlier call — a look-up sees every vrt_write_nodes and
 * vrt_write_chunk_roots before it, with no frame in between — waiting for its own work only, and leaving everything a frame left
 * behind (vrt_read_output, vrt_present*, vrt_get_stats, the accumulation) as it was.  n = 0 does nothing.  A multi-device context
 * answers on device_ids[0]; a sharded context holds the whole world and answers alone. */
int vrt_get_voxels(vrt_ctx *ctx, const int32_t *pos, uint32_t n, vrt_voxel_at *out);
/* The same with device memory (n x 3 int32 in, n vrt_voxel_at out, 4-byte aligned), asynchronous on the context's stream. */
int vrt_get_voxels_device(vrt_ctx *ctx, const void *pos_device, uint32_t n, void *out_device);

/* ClientWorld::highest_vox_at (client/src/world.rs:359-366), batched, one column per lane: the largest y in
 * [min.y, min.y + 32 * size_in_chunks) at which the voxel of column (x, z) counts.
 * A voxel counts when its id is not 0 (Voxel::is_empty: liquids count) — or, with VRT_COLUMN_SOLID, when it is SOLID as in
 * vrt_clip_moves: materials[min(v, 255)].is_empty == 0 && .is_liquid == 0 of the context's material table, so water over sand
 * answers the sand.  A position in a chunk whose chunk_roots entry is 0 holds Voxel::EMPTY.  Voxel 0 never counts, whatever
 * entry 0 of the table says: highest_vox_at never reports air.
 * Without VRT_COLUMN_FROM_Y the scan starts at the top of the world, min.y + 32 * size_in_chunks - 1: highest_vox_at itself.
 * With it the scan starts at min(from_y, top of the world): a from_y that lies on a counting voxel answers that voxel, and a
 * from_y below min.y is NONE.  x or z outside the world box is OUTSIDE.  Other bits of flags have no meaning and are ignored.
 * No query is rejected: every int32 is legal in every field, and a scan ends after the 32 * size_in_chunks voxels of a column
 * at the latest (the kernel steps over whole leaves that do not count: docs/KERNELS.md). */
#define VRT_COLUMN_FROM_Y 1u /* start at min(from_y, top of the world) instead of at the top */
#define VRT_COLUMN_SOLID 2u  /* a voxel counts when it is solid, not merely non-empty */
typedef struct {
    int32_t x, z;
    int32_t from_y;  /* read with VRT_COLUMN_FROM_Y only */
    uint32_t flags;  /* VRT_COLUMN_FROM_Y | VRT_COLUMN_SOLID */
} vrt_column_query;  /* 16 B */

#define VRT_COLUMN_NONE 0u    /* nothing counts in the range; y = world.min[1] - 1, voxel = 0 */
#define VRT_COLUMN_FOUND 1u
#define VRT_COLUMN_OUTSIDE 2u /* x or z outside the world box; y = 0, voxel = 0 */
typedef struct {
    int32_t y;       /* the highest counting voxel's y */
    uint32_t voxel;  /* its id */
    uint32_t status; /* VRT_COLUMN_* */
    uint32_t _reserved; /* 0 */
} vrt_column_top;  /* 16 B */

/* n queries from host memory, n results into host memory; ordering and scope are vrt_get_voxels's, and with VRT_COLUMN_SOLID
 * the call sees every vrt_write_materials before it as well. */
int vrt_column_tops(vrt_ctx *ctx, const vrt_column_query *queries, uint32_t n, vrt_column_top *out);
/* The same with device memory (n vrt_column_query in, n vrt_column_top out, 4-byte aligned), asynchronous on the context's stream. */
int vrt_column_tops_device(vrt_ctx *ctx, const void *queries_device, uint32_t n, void *out_device);

/* The whole world from above: the column top of every (x, z) of the world box, (32 * size_in_chunks)^2 entries,
 * map[(z - min.z) * 32 * size_in_chunks + (x - min.x)] (x fastest).  flags: 0 or VRT_COLUMN_SOLID, anything else is
 * VRT_ERR_INVALID_ARG; with VRT_COLUMN_SOLID the material table is read in enqueue order, as vrt_column_tops reads it. */
typedef struct {
    int32_t y;       /* no voxel of the column counts: world.min[1] - 1 */
    uint32_t voxel;  /* ... and 0 */
} vrt_top_entry;  /* 8 B */
/* Into host memory; ordered as vrt_column_tops, waits for its own work only. */
int vrt_read_top_map(vrt_ctx *ctx, uint32_t flags, vrt_top_entry *map);
/* Into device memory (8-byte aligned), asynchronous on the context's stream. */
int vrt_top_map_device(vrt_ctx *ctx, uint32_t flags, void *map_device);

/* ---- the chunk source: world generation on the device ---- */

/* What the server answers request_missing_chunks with (client/src/lib.rs:80-118: GiveChunkData -> create_chunk), built on
 * the device.  The specification is the host generator, csrc/host/worldgen.hpp: chunk i's nodes are, word for word,
 * build_svo_bottom_up(WorldGen{seed}.fill_dense(chunk_pos[i])) — vrth_svo_build_bottom_up(vrth_gen_dense(seed, pos)) of
 * include/vrt_host.h; a uniform chunk is its one node.  chunk_pos: n x int32[3], every coordinate in (-2^26, 2^26) (fill_dense
 * computes pos * 32 in int32), else VRT_ERR_INVALID_ARG before any work.  nodes: cap_nodes u16 words; offsets: n + 1 entries,
 * chunk i's nodes are nodes[offsets[i] .. offsets[i+1]).
 *  - n = 0: offsets[0] = 0, VRT_OK.
 *  - A chunk whose tree build_svo_bottom_up refuses (4096 mixed cells or more: a node index past 32767) gets an empty range; the
 *    others are still produced, and the call returns VRT_ERR_OUT_OF_RANGE.
 *  - cap_nodes too small: VRT_ERR_OOM with every offset written (offsets[n] = the words needed) and nodes untouched.
 * Runs on the context's stream behind every earlier call, in batches of 2048 chunks, and waits for its own results.  It touches
 * nothing else of the context: the node pool, chunk_roots, the derived tables and frames in flight stay as they are — the ranges
 * go to the pool through create_chunk on the host and vrt_write_nodes, as the reference's flow has it.  A
 * multi-device context generates on device_ids[0]. */
int vrt_generate_chunks(vrt_ctx *ctx, uint32_t seed, const int32_t *chunk_pos, uint32_t n, uint16_t *nodes, uint64_t cap_nodes,
                        uint64_t *offsets);
/* The builder alone: n caller blocks dense[x + 32*(y + 32*z)] (n x 32768 u16, any id 0..0xFFFF) -> their nodes, word for word
 * vrth_svo_build_bottom_up.  Results and errors as vrt_generate_chunks's. */
int vrt_build_chunks(vrt_ctx *ctx, const uint16_t *dense, uint32_t n, uint16_t *nodes, uint64_t cap_nodes, uint64_t *offsets);

/* Editing chunks that exist: the server's feature placement (server/src/world/mod.rs:28-55 World::place_features pushes every
 * placement of a BuiltFeature through Svo::set_node, one voxel at a time) and a client's brush, for a batch of chunks at once.
 * A shape is one call of BuiltFeature (server/src/world/gen.rs): trees, cacti, spikes and lakes (gen.rs:357-485) are built
 * from nothing else. */
#define VRT_SHAPE_POINT  0u  /* BuiltFeature::set_voxel(a)                    gen.rs:312-316 */
#define VRT_SHAPE_LINE   1u  /* place_line(a, b): common::math::walk_line     gen.rs:318-322, math.rs:228-324 */
#define VRT_SHAPE_SPHERE 2u  /* place_sphere(a, r)                            gen.rs:342-347 */
#define VRT_SHAPE_DISC   3u  /* place_disc(a, r, height)                      gen.rs:349-354 */
typedef struct {
    uint32_t kind;     /* VRT_SHAPE_* */
    uint32_t voxel;    /* 0 .. 0x7FFF; 0 carves (Voxel::EMPTY, the lake's upper discs) */
    int32_t  a[3];     /* the point / line start / centre, world voxel coordinates */
    int32_t  b[3];     /* LINE: the end; otherwise ignored */
    float    r;        /* SPHERE, DISC */
    uint32_t height;   /* DISC */
} vrt_shape;           /* 40 B */

/* n chunks in, the same chunks with m shapes applied out.  Chunk i sits at chunk_pos[3i..]; its tree is
 * nodes_in[offsets_in[i] .. offsets_in[i+1]) with child addresses relative to its own node 0 — a GiveChunkData payload, a
 * region-file chunk, or a pool range from vrth_world_chunk_state; an all-air chunk is the one word 0.  The result for chunk i is,
 * word for word, vrth_svo_build_bottom_up(D_i), D_i being vrth_svo_to_dense of its input tree with the shapes applied in order
 * 0 .. m-1 (a later shape overwrites an earlier one: BuiltFeature's map in its call order) restricted to the chunk's 32^3 voxels;
 * placements that fall in none of the n chunks are dropped (the reference logs a warning there).  changed[i] = 1 iff D_i differs
 * anywhere from the expanded input, compared after all shapes.  nodes_out, cap_nodes, offsets_out, a refused tree and VRT_ERR_OOM
 * are vrt_build_chunks's (changed is written in those cases too), and so are the batches of 2048 chunks and what the call leaves
 * alone: everything else of the context.  n = 0: offsets_out[0] = 0.  m = 0 re-canonicalises the trees; every changed is 0.
 * A shape's voxels are the reference's, in strict binary32:
 *  - POINT: a.  LINE: a, then LineWalker until the major axis reaches b (an axis where a and b are equal never moves).
 *  - SPHERE: every p with a - (int32_t)r <= p <= a + (int32_t)r per axis and d2 < r * r, d = ((float)p + 0.5f) - ((float)a + 0.5f)
 *    per axis, d2 = (d.x*d.x + d.y*d.y) + d.z*d.z: r = 0 places nothing, r = 0.4 the centre only.
 *  - DISC: the same test (the distance is three-dimensional, as in the reference) over a - ((int32_t)r, 0, (int32_t)r) ..
 *    a + ((int32_t)r, (int32_t)height - 1, (int32_t)r); height = 0 places nothing.
 * VRT_ERR_INVALID_ARG before anything is enqueued, with the outputs untouched, for: a null pointer that is needed; an unknown
 * kind; voxel > 0x7FFF; r negative, NaN or >= 32768; height > 32768; a coordinate of a, of b (LINE) or of 32 * chunk_pos outside
 * (-2^22, 2^22); a LINE whose largest dist exceeds 4096; offsets_in that decrease, or a range that is empty or longer than 32761;
 * a tree that is not well-formed (a child block that leaves the chunk's own range, a split node at depth 5).
 * VRT_ERR_OUT_OF_RANGE before any work for m > 65535, or when the (chunk, shape) pairs whose boxes intersect exceed 2^20. */
int vrt_edit_chunks(vrt_ctx *ctx, const int32_t *chunk_pos, uint32_t n, const uint16_t *nodes_in, const uint64_t *offsets_in,
                    const vrt_shape *shapes, uint32_t m, uint16_t *nodes_out, uint64_t cap_nodes, uint64_t *offsets_out,
                    uint8_t *changed);

/* ---- device-side plumbing for a host that owns streams / device memory (torch, RCCL) ---- */

/* Use the caller's hipStream_t for all subsequent work (NULL = the context's own stream). */
int vrt_set_stream(vrt_ctx *ctx, void *hip_stream);

/* The device output is one 16-byte texel per pixel slot: {r, g, b as f32, id word as u32}.
 * Unsharded: texel[height][width] row-major.  Sharded: the compact tile-major shard buffer
 * texel[tiles_padded][64] (tile t_local <-> the context's t_local-th screen tile in increasing order; pixel p of a
 * tile = (p&7, p>>3)); tiles_padded = ceil(total_tiles / P) is the largest count of any rank >= 1, so every gathered
 * message has the same size (with equal shares also rank 0's). */

/* Render into caller-owned device memory (e.g. a torch tensor handed to an RCCL gather) instead of the
 * context's own buffer: `texels` must hold the byte count vrt_device_output reports and be 16-byte
 * aligned.  NULL restores the context's buffer; vrt_resize_output drops the binding.  With a result size that is
 * not whole 8x8 tiles the frame's last columns / rows are never written (vrt_config.width): a row-major caller buffer
 * should start out zero, as the context's own buffers do, and the same goes for the dst of vrt_assemble*. */
int vrt_bind_output(vrt_ctx *ctx, void *texels);

/* Device pointer and size in bytes of the buffer frames are currently written to. */
int vrt_device_output(vrt_ctx *ctx, void **texels, uint64_t *bytes);

/* Number of 8x8 tiles this context traces, the padded per-rank count used for equal-sized gathers
 * (ceil(total_tiles / P)) and the total. */
int vrt_shard_info(vrt_ctx *ctx, uint32_t *tiles_local, uint32_t *tiles_padded, uint32_t *tiles_total);

/* On the gather root: scatter the shard_count gathered tile-major buffers (rank r's texels start at
 * gathered + r*rank_stride_bytes; 0 = densely packed, tiles_padded*64*16 bytes apart) into the
 * row-major device frame dst = texel[height][width].  A root created with VRT_FLAG_ROW_MAJOR has already written
 * its own tiles there: slot 0 of `gathered` is then ignored.  Asynchronous on the context's stream. */
int vrt_assemble(vrt_ctx *ctx, const void *gathered, uint64_t rank_stride_bytes, void *dst);

/* The same for VRT_FLAG_COMPACT messages (8 bytes per pixel slot; stride 0 = tiles_padded*64*8 bytes apart): the root —
 * a VRT_FLAG_ROW_MAJOR shard context holding the same camera / settings / world / materials as the senders — shades
 * every gathered pixel with the code the sender would have run, under the uniforms current at this call, and writes the
 * texel into dst. */
int vrt_assemble_compact(vrt_ctx *ctx, const void *gathered, uint64_t rank_stride_bytes, void *dst);

#ifdef __cplusplus
}
#endif
#endif

// vrt_path.hip — wavefront path trace (VRT_MODE_PATH) for gfx950.
//
// Structure after the reference's stale, never-dispatched path tracer
// (clientdesktop/src/graphics/path_tracer.wgsl: rng_next* :56-76, ray_color :149-194, seed :328) on top of the
// live march of ray_tracer.wgsl; the deliberate differences (bounce origin outside the hit voxel, clamped
// log argument, water neither stops nor tints a segment) are DESIGN.md §Path trace and are the same in
// oracle/vrt_oracle.c:trace_path.  Emission (path_tracer.wgsl:183-184) is a per-material table of the context's own,
// vrt_write_emission, 0 everywhere until a caller writes it; the kernels that add it are the EMIT instantiations below,
// chosen by the host only for a context with an entry that is not 0 (a table of zeros runs the kernels that have no
// emission term).  The coat of the same Material (:28-31, :175-185) is vrt_write_polish's table behind it, and the kernels
// that flip its coin are the path_polished_* ones below, chosen only for a context with a chance that is not 0.  The struct's
// last field, translucency (:29, :167-173), is vrt_write_translucency's table behind that one; the path_translucent_* kernels
// draw first whether a hit lets the path through, and are chosen only for a context with such a chance.  oracle/
// keeps none of them; the tests' references are tests/emission_ref.c, tests/polish_ref.c and tests/translucent_ref.c.  log and cos are
// spelled out in + - * / so that host and device agree to the bit: a one-ulp different bounce direction eventually hits a
// different voxel.
//
// One launch per bounce: bounce 0 traces the primary rays; every later bounce reads the compacted buffer of
// paths that are still alive (same per-segment ballot compaction as the shadow hit buffer), marches them and
// appends the survivors to the other buffer.  A pixel's path has exactly one owner lane per bounce, so
// radiance accumulates into the pixel's texel with plain read-modify-writes.
#include <cstdlib>

#include "vrt_path_common.h"
#include "vrt_path_sun.h"
#include "both/lens_math.h"

namespace vrt {

static_assert(kHitSegments == 256, "a launch's first workgroup (256 threads) clears the next launch's 256 segment cursors");

static inline size_t lds_bytes_path(const FrameParams &P, bool lds_roots) { return (24u + (lds_roots ? P.n_roots : 0u)) * 4u; }

#define VRT_PRIMARY_KERNEL path_primary_kernel
#define VRT_PRIMARY_POLISH 0
#define VRT_PRIMARY_TRANSLUCENT 0
#include "vrt_path_primary.h"
#undef VRT_PRIMARY_KERNEL
#undef VRT_PRIMARY_POLISH
#undef VRT_PRIMARY_TRANSLUCENT
#define VRT_PRIMARY_KERNEL path_polished_primary_kernel
#define VRT_PRIMARY_POLISH 1
#define VRT_PRIMARY_TRANSLUCENT 0
#include "vrt_path_primary.h"
#undef VRT_PRIMARY_KERNEL
#undef VRT_PRIMARY_POLISH
#undef VRT_PRIMARY_TRANSLUCENT
#define VRT_PRIMARY_KERNEL path_translucent_primary_kernel
#define VRT_PRIMARY_POLISH 0
#define VRT_PRIMARY_TRANSLUCENT 1
#include "vrt_path_primary.h"
#undef VRT_PRIMARY_KERNEL
#undef VRT_PRIMARY_POLISH
#undef VRT_PRIMARY_TRANSLUCENT
#define VRT_PRIMARY_KERNEL path_sunlit_primary_kernel   // (vrt_set_sun_light: coat and pass-through read from the launch)
#define VRT_PRIMARY_POLISH 0
#define VRT_PRIMARY_TRANSLUCENT 0
#define VRT_PRIMARY_SUN
#include "vrt_path_primary.h"
#undef VRT_PRIMARY_KERNEL
#undef VRT_PRIMARY_POLISH
#undef VRT_PRIMARY_TRANSLUCENT
#undef VRT_PRIMARY_SUN
#define VRT_LENS_KERNEL path_lens_primary_kernel   // (vrt_set_camera_sampling: a primary ray of its own for every sample)
#include "vrt_path_lens.h"
#undef VRT_LENS_KERNEL
#define VRT_LENS_KERNEL path_lens_sun_primary_kernel
#define VRT_LENS_SUN
#include "vrt_path_lens.h"
#undef VRT_LENS_KERNEL
#undef VRT_LENS_SUN

// One segment of a path: its march, then path_after_march.
template <int MARCH, bool LDS_ROOTS, bool STATS, bool EMIT, bool POLISH, bool TRANSLUCENT>
__device__ __forceinline__ bool path_segment(const FrameParams &P, const uint32_t *s_roots, const uint32_t *s_liquid,
                                             PathState &st, MarchResult &R, V3 &light, bool &lit) {
    R = march<MARCH, LDS_ROOTS, STATS>(P, s_roots, s_liquid, st.origin, st.dir);
    return path_after_march<EMIT, POLISH, TRANSLUCENT>(P, st, R, light, lit);
}

#define VRT_BOUNCE_KERNEL path_bounce_kernel
#define VRT_BOUNCE_POLISH 0
#define VRT_BOUNCE_TRANSLUCENT 0
#include "vrt_path_bounce.h"
#undef VRT_BOUNCE_KERNEL
#undef VRT_BOUNCE_POLISH
#undef VRT_BOUNCE_TRANSLUCENT
#define VRT_BOUNCE_KERNEL path_polished_bounce_kernel
#define VRT_BOUNCE_POLISH 1
#define VRT_BOUNCE_TRANSLUCENT 0
#include "vrt_path_bounce.h"
#undef VRT_BOUNCE_KERNEL
#undef VRT_BOUNCE_POLISH
#undef VRT_BOUNCE_TRANSLUCENT
#define VRT_BOUNCE_KERNEL path_translucent_bounce_kernel
#define VRT_BOUNCE_POLISH 0
#define VRT_BOUNCE_TRANSLUCENT 1
#include "vrt_path_bounce.h"
#undef VRT_BOUNCE_KERNEL
#undef VRT_BOUNCE_POLISH
#undef VRT_BOUNCE_TRANSLUCENT
#define VRT_BOUNCE_KERNEL path_sunlit_bounce_kernel
#define VRT_BOUNCE_POLISH 0
#define VRT_BOUNCE_TRANSLUCENT 0
#define VRT_BOUNCE_SUN
#include "vrt_path_bounce.h"
#undef VRT_BOUNCE_KERNEL
#undef VRT_BOUNCE_POLISH
#undef VRT_BOUNCE_TRANSLUCENT
#undef VRT_BOUNCE_SUN

}  // namespace vrt
#include "vrt_path_lamp.h"   // (vrt_set_lamp_light: kernels of their own, behind everything they share with the others)
namespace vrt {

// ------------------------------------------------------------------------------------------------
// Bounce b >= 1 over the MARCH CELLS (vrt_accel.hip; the default for plain frames of worlds that have them): the pool
// kernel above with a march loop that has ONE load per step and no dependent load at all.
//
// What held the pool kernel at a quarter of its issue rate was the pair of dependent loads of a step in a split cell —
// cell entry, then the voxel's brick entry: 290 + 515 cycles of a 2 200-cycle wave-step, half of them L1 misses
// (profiles/r02_path_pmc_summary.txt) — on the critical path of every ray, and a launch lasts as long as its longest
// chain of steps.  A march cell answers both questions of a step from one 16-byte entry: the leaf's size (a leaf
// cell's lo, or the split cell's size-2 mask) and whether the voxel stops the ray (64 bits; liquids are transparent to
// a path segment, so they count as air — the tables are built with the material table's liquid set).  Which voxel it
// stopped on is only asked after the march, at full width, from the brick (phase C).
// Also new here: phase C takes the rays that hit and the rays that missed in separate batches (a wave executes both sides of that branch otherwise: ~510 + ~130 vector
// instructions per ray), and on the last bounce the rays that hit are not shaded at all (their bounce would be dropped).
// Every ray executes the arithmetic the other kernels execute for it: bit-identical frames (tests).
// ------------------------------------------------------------------------------------------------



// KB: batches of 64 rays in a wave's pool.  4 (256 rays, 32 waves per CU) everywhere but for small worlds with two frames in flight:
// there 5 (320 rays, 28 waves per CU) — fewer dry tails per ray, and the four wave slots a CU keeps free let the next frame's primary
// launch start beside this one: C4 + 2.8 % (one frame at a time - 2.2 %, C5 - 3.8 %: profiles/r05_pool_k5.txt)
#define VRT_CELLS_KERNEL path_bounce_cells_kernel
#define VRT_CELLS_EMIT 0
#define VRT_CELLS_POLISH 0
#define VRT_CELLS_TRANSLUCENT 0
#include "vrt_path_cells.h"
#undef VRT_CELLS_KERNEL
#undef VRT_CELLS_EMIT
#undef VRT_CELLS_POLISH
#undef VRT_CELLS_TRANSLUCENT
#define VRT_CELLS_KERNEL path_emissive_cells_kernel
#define VRT_CELLS_EMIT 1
#define VRT_CELLS_POLISH 0
#define VRT_CELLS_TRANSLUCENT 0
#include "vrt_path_cells.h"
#undef VRT_CELLS_KERNEL
#undef VRT_CELLS_EMIT
#undef VRT_CELLS_POLISH
#undef VRT_CELLS_TRANSLUCENT
#define VRT_CELLS_KERNEL path_polished_cells_kernel
#define VRT_CELLS_EMIT 1
#define VRT_CELLS_POLISH 1
#define VRT_CELLS_TRANSLUCENT 0
#include "vrt_path_cells.h"
#undef VRT_CELLS_KERNEL
#undef VRT_CELLS_EMIT
#undef VRT_CELLS_POLISH
#undef VRT_CELLS_TRANSLUCENT
#define VRT_CELLS_KERNEL path_translucent_cells_kernel
#define VRT_CELLS_EMIT 1
#define VRT_CELLS_POLISH 0
#define VRT_CELLS_TRANSLUCENT 1
#include "vrt_path_cells.h"
#undef VRT_CELLS_KERNEL
#undef VRT_CELLS_EMIT
#undef VRT_CELLS_POLISH
#undef VRT_CELLS_TRANSLUCENT


// The end of a launch chain of several samples: the running sum plus the chain's planes, in sample order — the order the
// one-sample-per-chain launches add them in and the oracle's — and the division once the last chain is in.  A plain frame's
// sum is its output (mean == sum: divided in place); an accumulating frame's is the context's (VRT_RENDER_ACCUMULATE), kept
// undivided, and the last chain also stores the mean into the frame's output.  first: the chain holds the sum's first sample.
__global__ void path_chain_finish_kernel(Texel *sum, Texel *mean, const Texel *acc, uint32_t n, uint32_t chain, uint32_t first, uint32_t last,
                                         float count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint4 t = acc[i];   // the chain's first sample: the sum's first (light and id word as they are), or one more term
    if (!first) {
        const uint4 o = sum[i];
        t.x = __float_as_uint(__uint_as_float(o.x) + __uint_as_float(t.x));
        t.y = __float_as_uint(__uint_as_float(o.y) + __uint_as_float(t.y));
        t.z = __float_as_uint(__uint_as_float(o.z) + __uint_as_float(t.z));
        t.w = o.w;
    }
    for (uint32_t s = 1; s < chain; s++) {
        const uint4 a = acc[(size_t)s * n + i];
        t.x = __float_as_uint(__uint_as_float(t.x) + __uint_as_float(a.x));
        t.y = __float_as_uint(__uint_as_float(t.y) + __uint_as_float(a.y));
        t.z = __float_as_uint(__uint_as_float(t.z) + __uint_as_float(a.z));
    }
    if (!last || mean != sum) sum[i] = t;
    if (last) {
        t.x = __float_as_uint(__uint_as_float(t.x) / count);
        t.y = __float_as_uint(__uint_as_float(t.y) / count);
        t.z = __float_as_uint(__uint_as_float(t.z) / count);
        mean[i] = t;
    }
}

// An accumulating frame of one-sample chains (VRT_RENDER_ACCUMULATE; spp 1, stats, literal, no march cells): behind each of its
// samples, the sample's light (its own in `out`: the sample's first segment stored the texel, or added to the zeros left here)
// joins the context's sum — stored when it is the sum's first, else added: the order a frame of all the samples adds them in.
// The frame's last sample leaves the mean in `out`; an earlier one leaves zero light for the next sample to add to.  The id word
// is the frame's own, in both.  64 bytes a pixel, all of them NON-TEMPORAL (store_streaming, vrt_device.h): the pass runs beside
// the next frame's march, whose table loads hit the L2 only while 133 MB of texels (1080p) do not push their lines out.
__device__ __forceinline__ uint4 load_streaming(const Texel *p) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 t = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
    return make_uint4(t.x, t.y, t.z, t.w);
}

__global__ void path_accum_resolve_kernel(Texel *out, Texel *sum, uint32_t n, uint32_t first, uint32_t last, float count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint4 t = load_streaming(out + i);
    if (!first) {
        const uint4 o = load_streaming(sum + i);
        t.x = __float_as_uint(__uint_as_float(o.x) + __uint_as_float(t.x));
        t.y = __float_as_uint(__uint_as_float(o.y) + __uint_as_float(t.y));
        t.z = __float_as_uint(__uint_as_float(o.z) + __uint_as_float(t.z));
    }
    store_streaming(sum + i, t);
    if (last) {
        t.x = __float_as_uint(__uint_as_float(t.x) / count);
        t.y = __float_as_uint(__uint_as_float(t.y) / count);
        t.z = __float_as_uint(__uint_as_float(t.z) / count);
    } else {
        t.x = t.y = t.z = 0u;
    }
    store_streaming(out + i, t);
}

// rgb /= spp after the last sample
__global__ void path_finish_kernel(Texel *out, uint32_t n, float spp) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint4 t = out[i];
    t.x = __float_as_uint(__uint_as_float(t.x) / spp);
    t.y = __float_as_uint(__uint_as_float(t.y) / spp);
    t.z = __float_as_uint(__uint_as_float(t.z) / spp);
    out[i] = t;
}


// The path trace marches with the grid march when the derived tables exist (P.grid), else with the ancestor-cache walk;
// `literal` (air flagged liquid, vrt_frames.hip) with the shader's text.  TAIL: the template arguments after the first three
// (empty: the kernel's defaults, no emission)
// VRT_PATH_ARGS: the kernel's arguments (P; a sun-lit frame's kernels: P, S)
#define VRT_PATH_LAUNCH(kernel, TAIL)                                                                                     \
    do {                                                                                                                  \
        const bool lds = (!P.grid || literal) && P.n_roots <= kLdsRootsMax;                                               \
        const size_t sh = lds_bytes_path(P, lds);                                                                         \
        if (literal) {                                                                                                    \
            if (lds) { if (stats) hipLaunchKernelGGL((kernel<1, true, true TAIL>), grid, block, sh, st, VRT_PATH_ARGS); else hipLaunchKernelGGL((kernel<1, true, false TAIL>), grid, block, sh, st, VRT_PATH_ARGS); } \
            else { if (stats) hipLaunchKernelGGL((kernel<1, false, true TAIL>), grid, block, sh, st, VRT_PATH_ARGS); else hipLaunchKernelGGL((kernel<1, false, false TAIL>), grid, block, sh, st, VRT_PATH_ARGS); } \
        } else if (P.grid) {                                                                                              \
            if (stats) hipLaunchKernelGGL((kernel<0, false, true TAIL>), grid, block, sh, st, VRT_PATH_ARGS);                         \
            else hipLaunchKernelGGL((kernel<0, false, false TAIL>), grid, block, sh, st, VRT_PATH_ARGS);                              \
        } else if (lds) {                                                                                                 \
            if (stats) hipLaunchKernelGGL((kernel<2, true, true TAIL>), grid, block, sh, st, VRT_PATH_ARGS);                          \
            else hipLaunchKernelGGL((kernel<2, true, false TAIL>), grid, block, sh, st, VRT_PATH_ARGS);                               \
        } else {                                                                                                          \
            if (stats) hipLaunchKernelGGL((kernel<2, false, true TAIL>), grid, block, sh, st, VRT_PATH_ARGS);                         \
            else hipLaunchKernelGGL((kernel<2, false, false TAIL>), grid, block, sh, st, VRT_PATH_ARGS);                              \
        }                                                                                                                 \
    } while (0)
#define VRT_PATH_ARGS P
#define VRT_PRIMARY_EMIT , false, true   // (MULTI, EMIT)
#define VRT_BOUNCE_EMIT , true                  // (EMIT)

// polish (vrt_write_polish; the frame plan gives it with emit): the kernels of the same three families that flip the coat's coin
// translucent (vrt_write_translucency; with emit as well): the path_translucent_* kernels, whatever polish says — they read on the
// device whether there is a coat
void launch_path_primary(const FrameParams &P, bool stats, bool literal, bool emit, bool polish, bool translucent, hipStream_t st) {
    if (P.tiles_local == 0) return;
    const dim3 grid((P.tiles_local + 3u) / 4u), block(256);
    if (P.acc) {   // several samples per launch chain: plain frames over the derived tables only (vrt_frames.hip)
        if (translucent) hipLaunchKernelGGL((path_translucent_primary_kernel<0, false, false, true, true>), grid, block, lds_bytes_path(P, false), st, P);
        else if (polish) hipLaunchKernelGGL((path_polished_primary_kernel<0, false, false, true, true>), grid, block, lds_bytes_path(P, false), st, P);
        else if (emit) hipLaunchKernelGGL((path_primary_kernel<0, false, false, true, true>), grid, block, lds_bytes_path(P, false), st, P);
        else hipLaunchKernelGGL((path_primary_kernel<0, false, false, true>), grid, block, lds_bytes_path(P, false), st, P);
        return;
    }
    if (translucent) VRT_PATH_LAUNCH(path_translucent_primary_kernel, VRT_PRIMARY_EMIT);
    else if (polish) VRT_PATH_LAUNCH(path_polished_primary_kernel, VRT_PRIMARY_EMIT);
    else if (emit) VRT_PATH_LAUNCH(path_primary_kernel, VRT_PRIMARY_EMIT);
    else VRT_PATH_LAUNCH(path_primary_kernel, );
}

// the pool kernel over the march cells (P.mblk): `segments` bounce segments in this one launch (every wave carries its own
// survivors from one to the next; P.path_in / P.path_out are the two buffers it goes back and forth between)
void launch_path_bounce_cells(const FrameParams &P, uint32_t refill_at, uint32_t segments, uint32_t pool_batches, bool emit, bool polish, bool translucent,
                              hipStream_t st) {
    if (P.tiles_local == 0 || segments == 0) return;
    const uint32_t refill = refill_at >= 1u && refill_at <= 64u ? refill_at : kPoolRefillAt;
    const uint32_t kb = (pool_batches == 5u && P.march_direct) ? 5u : 4u, entries = kb * 64u;   // (320-ray pools: direct worlds only)
    const uint32_t parts = (P.in_seg_cap + 4u * entries - 1u) / (4u * entries);
    const dim3 grid(kHitSegments * parts), block(256);
    const size_t sh = 8u * 4u + 4u * (entries * 16u + entries * 2u);   // per wave: the pool + a u16 order per entry
    const CellsLaunch L{P, refill, segments};
    if (translucent) {
        if (kb == 5u) hipLaunchKernelGGL((path_translucent_cells_kernel<true, 5u>), grid, block, sh, st, L);
        else if (P.march_direct) hipLaunchKernelGGL((path_translucent_cells_kernel<true, 4u>), grid, block, sh, st, L);
        else hipLaunchKernelGGL((path_translucent_cells_kernel<false, 4u>), grid, block, sh, st, L);
        return;
    }
    if (polish) {
        if (kb == 5u) hipLaunchKernelGGL((path_polished_cells_kernel<true, 5u>), grid, block, sh, st, L);
        else if (P.march_direct) hipLaunchKernelGGL((path_polished_cells_kernel<true, 4u>), grid, block, sh, st, L);
        else hipLaunchKernelGGL((path_polished_cells_kernel<false, 4u>), grid, block, sh, st, L);
        return;
    }
    if (emit) {
        if (kb == 5u) hipLaunchKernelGGL((path_emissive_cells_kernel<true, 5u>), grid, block, sh, st, L);
        else if (P.march_direct) hipLaunchKernelGGL((path_emissive_cells_kernel<true, 4u>), grid, block, sh, st, L);
        else hipLaunchKernelGGL((path_emissive_cells_kernel<false, 4u>), grid, block, sh, st, L);
        return;
    }
    if (kb == 5u) hipLaunchKernelGGL((path_bounce_cells_kernel<true, 5u>), grid, block, sh, st, L);
    else if (P.march_direct) hipLaunchKernelGGL((path_bounce_cells_kernel<true, 4u>), grid, block, sh, st, L);
    else hipLaunchKernelGGL((path_bounce_cells_kernel<false, 4u>), grid, block, sh, st, L);
}

void launch_path_bounce(const FrameParams &P, bool stats, bool literal, bool emit, bool polish, bool translucent, hipStream_t st) {
    if (P.tiles_local == 0) return;
    const dim3 grid(kHitSegments * (P.hit_seg_cap / 256u)), block(256);
    if (translucent) VRT_PATH_LAUNCH(path_translucent_bounce_kernel, VRT_BOUNCE_EMIT);
    else if (polish) VRT_PATH_LAUNCH(path_polished_bounce_kernel, VRT_BOUNCE_EMIT);
    else if (emit) VRT_PATH_LAUNCH(path_bounce_kernel, VRT_BOUNCE_EMIT);
    else VRT_PATH_LAUNCH(path_bounce_kernel, );
}
#undef VRT_PATH_ARGS
#define VRT_PATH_ARGS P, S

// vrt_set_sun_light: a sun-lit frame is one lane = path launch per segment (one sample per chain, the emission term carried), each
// followed by launch_path_sun over the records it appended
void launch_path_primary_sunlit(const FrameParams &P, const SunLaunch &S, bool stats, bool literal, hipStream_t st) {
    if (P.tiles_local == 0) return;
    const dim3 grid((P.tiles_local + 3u) / 4u), block(256);
    VRT_PATH_LAUNCH(path_sunlit_primary_kernel, VRT_PRIMARY_EMIT);
}

void launch_path_bounce_sunlit(const FrameParams &P, const SunLaunch &S, bool stats, bool literal, hipStream_t st) {
    if (P.tiles_local == 0) return;
    const dim3 grid(kHitSegments * (P.hit_seg_cap / 256u)), block(256);
    VRT_PATH_LAUNCH(path_sunlit_bounce_kernel, VRT_BOUNCE_EMIT);
}

// cells (the plan's sun_cells: a plain frame that was handed the march cells) — the occlusion-only march (vrt_path_sun.h); else
// march<>, which also counts.  The plan decides; nothing is asked again here
void launch_path_sun(const FrameParams &P, const SunLaunch &S, bool stats, bool literal, bool cells, hipStream_t st) {
    if (P.tiles_local == 0) return;
    const dim3 grid(kHitSegments * (S.seg_cap / 256u)), block(256);
    if (cells) {
        if (P.march_direct) hipLaunchKernelGGL((path_sun_cells_kernel<true>), grid, block, 0, st, P, S);
        else hipLaunchKernelGGL((path_sun_cells_kernel<false>), grid, block, 0, st, P, S);
        return;
    }
    VRT_PATH_LAUNCH(path_sun_kernel, );
}
#undef VRT_PATH_ARGS
#define VRT_PATH_ARGS P, L

// vrt_set_camera_sampling: bounce 0 of a frame with the setting on (vrt_path_lens.h); the launches behind it are the frame's own
void launch_path_primary_lens(const FrameParams &P, const LensLaunch &L, bool stats, bool literal, hipStream_t st) {
    if (P.tiles_local == 0) return;
    const dim3 grid((P.tiles_local + 3u) / 4u), block(256);
    if (P.acc) {   // several samples per launch chain: plain frames over the derived tables only
        hipLaunchKernelGGL((path_lens_primary_kernel<0, false, false, true>), grid, block, lds_bytes_path(P, false), st, P, L);
        return;
    }
    VRT_PATH_LAUNCH(path_lens_primary_kernel, );
}
#undef VRT_PATH_ARGS
#define VRT_PATH_ARGS P, L, S

void launch_path_primary_lens_sunlit(const FrameParams &P, const LensLaunch &L, const SunLaunch &S, bool stats, bool literal, hipStream_t st) {
    if (P.tiles_local == 0) return;
    const dim3 grid((P.tiles_local + 3u) / 4u), block(256);
    VRT_PATH_LAUNCH(path_lens_sun_primary_kernel, );
}
#undef VRT_PATH_ARGS
#define VRT_PATH_ARGS P, L, S, M
#define VRT_LAMP_PINHOLE , false
#define VRT_LAMP_SAMPLED , true

// vrt_set_lamp_light (vrt_path_lamp.h): a lamp-lit frame is one lane = path launch per segment, as a sun-lit one; each is followed by
// the sun launch, if the sun is on as well, and by launch_path_lamp_rays over the lamp records it appended.  sampled: the frame has
// vrt_set_camera_sampling on (L is read then)
void launch_path_primary_lamp(const FrameParams &P, const LensLaunch &L, const SunLaunch &S, const LampLaunch &M, bool sampled, bool stats, bool literal,
                              hipStream_t st) {
    if (P.tiles_local == 0) return;
    const dim3 grid((P.tiles_local + 3u) / 4u), block(256);
    if (sampled) VRT_PATH_LAUNCH(path_lamp_primary_kernel, VRT_LAMP_SAMPLED);
    else VRT_PATH_LAUNCH(path_lamp_primary_kernel, VRT_LAMP_PINHOLE);
}
#undef VRT_PATH_ARGS
#define VRT_PATH_ARGS P, S, M

void launch_path_bounce_lamp(const FrameParams &P, const SunLaunch &S, const LampLaunch &M, bool stats, bool literal, hipStream_t st) {
    if (P.tiles_local == 0) return;
    const dim3 grid(kHitSegments * (P.hit_seg_cap / 256u)), block(256);
    VRT_PATH_LAUNCH(path_lamp_bounce_kernel, );
}
#undef VRT_PATH_ARGS
#define VRT_PATH_ARGS P, M

void launch_path_lamp_rays(const FrameParams &P, const LampLaunch &M, bool stats, bool literal, hipStream_t st) {
    if (P.tiles_local == 0) return;
    const dim3 grid(kHitSegments * (M.seg_cap / 256u)), block(256);
    VRT_PATH_LAUNCH(path_lamp_rays_kernel, );
}
#undef VRT_LAMP_PINHOLE
#undef VRT_LAMP_SAMPLED
#undef VRT_PATH_ARGS
#undef VRT_PATH_LAUNCH
#undef VRT_PRIMARY_EMIT
#undef VRT_BOUNCE_EMIT

void launch_path_chain_finish(Texel *sum, Texel *mean, const Texel *acc, uint32_t n, uint32_t chain, bool first, bool last, uint32_t count,
                              hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(path_chain_finish_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, sum, mean, acc, n, chain, first ? 1u : 0u,
                       last ? 1u : 0u, (float)count);
}

void launch_path_accum_resolve(Texel *out, Texel *sum, uint32_t n, bool first, bool last, uint32_t count, hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(path_accum_resolve_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, out, sum, n, first ? 1u : 0u, last ? 1u : 0u,
                       (float)count);
}

void launch_path_finish(Texel *out, uint32_t n, uint32_t spp, hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(path_finish_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, out, n, (float)spp);
}

}  // namespace vrt

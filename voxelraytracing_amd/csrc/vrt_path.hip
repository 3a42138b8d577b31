// vrt_path.hip — wavefront path trace (VRT_MODE_PATH) for gfx950.
//
// Structure after the reference's stale, never-dispatched path tracer
// (clientdesktop/src/graphics/path_tracer.wgsl: rng_next* :56-76, ray_color :149-194, seed :328) on top of the
// live march of ray_tracer.wgsl; the deliberate differences (bounce origin outside the hit voxel, clamped
// log argument, water neither stops nor tints a segment) are DESIGN.md §Path trace and are the same in
// oracle/vrt_oracle.c:trace_path.  Emission (path_tracer.wgsl:183-184) is a per-material table of the context's own,
// vrt_write_emission, 0 everywhere until a caller writes it; the kernels that add it are the EMIT instantiations of the
// templates, chosen by the host only for a context with an entry that is not 0 (a table of zeros runs the kernels that have no
// emission term).  The coat of the same Material (:28-31, :175-185) is vrt_write_polish's table behind it, and the kernels
// that flip its coin are the POLISH instantiations, chosen only for a context with a chance that is not 0.  The struct's
// last field, translucency (:29, :167-173), is vrt_write_translucency's table behind that one; the TRANSLUCENT instantiations
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
#include <type_traits>

#include "vrt_path_common.h"
#include "vrt_path_primary.h"
#include "vrt_path_bounce.h"
#include "vrt_path_cells.h"
#include "vrt_path_sun.h"
#include "vrt_path_lens.h"
#include "vrt_path_lamp.h"   // (vrt_set_lamp_light: kernels of their own, behind everything they share with the others)
#include "vrt_path_water.h"  // (vrt_set_water_optics: a pair of their own again)
#include "vrt_path_refract.h"  // (vrt_set_water_refraction: that pair with the span walk and the bends)
#include "vrt_path_haze.h"   // (vrt_set_haze: a pair of their own with the distance draw behind the march)

namespace vrt {

static_assert(kHitSegments == 256, "a launch's first workgroup (256 threads) clears the next launch's 256 segment cursors");

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


// The march build of a launch, as the first three template arguments of its kernel: the path trace marches with the grid march
// when the derived tables exist (P.grid), else with the ancestor-cache walk; `literal` (air flagged liquid, vrt_frames.hip) with
// the shader's text; the root table in LDS where a march that reads it finds room.
template <int MARCH, bool LDS_ROOTS, bool STATS>
struct MarchBuild {
    static constexpr int march = MARCH;
    static constexpr bool lds_roots = LDS_ROOTS, stats = STATS;
};
static inline size_t lds_bytes_path(const FrameParams &P, bool lds_roots) { return (24u + (lds_roots ? P.n_roots : 0u)) * 4u; }

// launch(MarchBuild<...>{}, the launch's LDS bytes) for the build of this frame: ten of them
template <class F>
static void with_march_build(const FrameParams &P, bool stats, bool literal, F launch) {
    const bool lds = (!P.grid || literal) && P.n_roots <= kLdsRootsMax;
    const size_t sh = lds_bytes_path(P, lds);
    auto with_stats = [&](auto march, auto roots) {
        if (stats) launch(MarchBuild<march(), roots(), true>{}, sh);
        else launch(MarchBuild<march(), roots(), false>{}, sh);
    };
    auto with_roots = [&](auto march) {
        if (lds) with_stats(march, std::true_type{});
        else with_stats(march, std::false_type{});
    };
    if (literal) with_roots(std::integral_constant<int, 1>{});
    else if (P.grid) with_stats(std::integral_constant<int, 0>{}, std::false_type{});
    else with_roots(std::integral_constant<int, 2>{});
}

// The lobes of a frame's materials, as the EMIT, POLISH, TRANSLUCENT template arguments of its kernels.  polish (vrt_write_polish;
// the frame plan gives it with emit): the kernels that flip the coat's coin.  translucent (vrt_write_translucency; with emit as
// well): the kernels that draw first whether a hit lets the path through, whatever polish says — they read on the device whether
// there is a coat.
template <bool EMIT, bool POLISH, bool TRANSLUCENT>
struct Lobes {
    static constexpr bool emit = EMIT, polish = POLISH, translucent = TRANSLUCENT;
};
template <class F>
static void with_lobes(bool emit, bool polish, bool translucent, F launch) {
    if (translucent) launch(Lobes<true, false, true>{});
    else if (polish) launch(Lobes<true, true, false>{});
    else if (emit) launch(Lobes<true, false, false>{});
    else launch(Lobes<false, false, false>{});
}

static inline dim3 grid_of_tiles(const FrameParams &P) { return dim3((P.tiles_local + 3u) / 4u); }                              // a wave per tile
static inline dim3 grid_of_records(uint32_t seg_cap) { return dim3(kHitSegments * (seg_cap / 256u)); }   // a lane per record of every segment

void launch_path_primary(const FrameParams &P, bool stats, bool literal, bool emit, bool polish, bool translucent, hipStream_t st) {
    if (P.tiles_local == 0) return;
    const dim3 grid = grid_of_tiles(P), block(256);
    with_lobes(emit, polish, translucent, [&](auto lobes) {
        using L = decltype(lobes);
        if (P.acc) {   // several samples per launch chain: plain frames over the derived tables only (vrt_frames.hip)
            hipLaunchKernelGGL((path_primary_kernel<0, false, false, true, L::emit, L::polish, L::translucent>), grid, block, lds_bytes_path(P, false), st, P);
            return;
        }
        with_march_build(P, stats, literal, [&](auto build, size_t sh) {
            using B = decltype(build);
            hipLaunchKernelGGL((path_primary_kernel<B::march, B::lds_roots, B::stats, false, L::emit, L::polish, L::translucent>), grid, block, sh, st, P);
        });
    });
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
    const CellsLaunch C{P, refill, segments};
    with_lobes(emit, polish, translucent, [&](auto lobes) {
        using L = decltype(lobes);
        if (kb == 5u) hipLaunchKernelGGL((path_bounce_cells_kernel<true, 5u, L::emit, L::polish, L::translucent>), grid, block, sh, st, C);
        else if (P.march_direct) hipLaunchKernelGGL((path_bounce_cells_kernel<true, 4u, L::emit, L::polish, L::translucent>), grid, block, sh, st, C);
        else hipLaunchKernelGGL((path_bounce_cells_kernel<false, 4u, L::emit, L::polish, L::translucent>), grid, block, sh, st, C);
    });
}

void launch_path_bounce(const FrameParams &P, bool stats, bool literal, bool emit, bool polish, bool translucent, hipStream_t st) {
    if (P.tiles_local == 0) return;
    const dim3 grid = grid_of_records(P.hit_seg_cap), block(256);
    with_lobes(emit, polish, translucent, [&](auto lobes) {
        using L = decltype(lobes);
        with_march_build(P, stats, literal, [&](auto build, size_t sh) {
            using B = decltype(build);
            hipLaunchKernelGGL((path_bounce_kernel<B::march, B::lds_roots, B::stats, L::emit, L::polish, L::translucent>), grid, block, sh, st, P);
        });
    });
}

// vrt_set_sun_light: a sun-lit frame is one lane = path launch per segment (one sample per chain, the emission term carried), each
// followed by launch_path_sun over the records it appended
void launch_path_primary_sunlit(const FrameParams &P, const SunLaunch &S, bool stats, bool literal, hipStream_t st) {
    if (P.tiles_local == 0) return;
    const dim3 grid = grid_of_tiles(P), block(256);
    with_march_build(P, stats, literal, [&](auto build, size_t sh) {
        using B = decltype(build);
        hipLaunchKernelGGL((path_primary_kernel<B::march, B::lds_roots, B::stats, false, true, false, false, SunLaunch>), grid, block, sh, st, P, S);
    });
}

void launch_path_bounce_sunlit(const FrameParams &P, const SunLaunch &S, bool stats, bool literal, hipStream_t st) {
    if (P.tiles_local == 0) return;
    const dim3 grid = grid_of_records(P.hit_seg_cap), block(256);
    with_march_build(P, stats, literal, [&](auto build, size_t sh) {
        using B = decltype(build);
        hipLaunchKernelGGL((path_bounce_kernel<B::march, B::lds_roots, B::stats, true, false, false, SunLaunch>), grid, block, sh, st, P, S);
    });
}

// cells (the plan's sun_cells: a plain frame that was handed the march cells) — the occlusion-only march (vrt_path_sun.h); else
// march<>, which also counts.  The plan decides; nothing is asked again here
void launch_path_sun(const FrameParams &P, const SunLaunch &S, bool stats, bool literal, bool cells, hipStream_t st) {
    if (P.tiles_local == 0) return;
    const dim3 grid = grid_of_records(S.seg_cap), block(256);
    if (cells) {
        if (P.march_direct) hipLaunchKernelGGL((path_sun_cells_kernel<true>), grid, block, 0, st, P, S);
        else hipLaunchKernelGGL((path_sun_cells_kernel<false>), grid, block, 0, st, P, S);
        return;
    }
    with_march_build(P, stats, literal, [&](auto build, size_t sh) {
        using B = decltype(build);
        hipLaunchKernelGGL((path_sun_kernel<B::march, B::lds_roots, B::stats>), grid, block, sh, st, P, S);
    });
}

// vrt_set_camera_sampling: bounce 0 of a frame with the setting on (vrt_path_lens.h); the launches behind it are the frame's own
void launch_path_primary_lens(const FrameParams &P, const LensLaunch &L, bool stats, bool literal, hipStream_t st) {
    if (P.tiles_local == 0) return;
    const dim3 grid = grid_of_tiles(P), block(256);
    if (P.acc) {   // several samples per launch chain: plain frames over the derived tables only
        hipLaunchKernelGGL((path_lens_primary_kernel<0, false, false, true>), grid, block, lds_bytes_path(P, false), st, P, L);
        return;
    }
    with_march_build(P, stats, literal, [&](auto build, size_t sh) {
        using B = decltype(build);
        hipLaunchKernelGGL((path_lens_primary_kernel<B::march, B::lds_roots, B::stats>), grid, block, sh, st, P, L);
    });
}

void launch_path_primary_lens_sunlit(const FrameParams &P, const LensLaunch &L, const SunLaunch &S, bool stats, bool literal, hipStream_t st) {
    if (P.tiles_local == 0) return;
    const dim3 grid = grid_of_tiles(P), block(256);
    with_march_build(P, stats, literal, [&](auto build, size_t sh) {
        using B = decltype(build);
        hipLaunchKernelGGL((path_lens_primary_kernel<B::march, B::lds_roots, B::stats, false, SunLaunch>), grid, block, sh, st, P, L, S);
    });
}

// vrt_set_lamp_light (vrt_path_lamp.h): a lamp-lit frame is one lane = path launch per segment, as a sun-lit one; each is followed by
// the sun launch, if the sun is on as well, and by launch_path_lamp_rays over the lamp records it appended.  sampled: the frame has
// vrt_set_camera_sampling on (L is read then)
void launch_path_primary_lamp(const FrameParams &P, const LensLaunch &L, const SunLaunch &S, const LampLaunch &M, bool sampled, bool stats, bool literal,
                              hipStream_t st) {
    if (P.tiles_local == 0) return;
    const dim3 grid = grid_of_tiles(P), block(256);
    with_march_build(P, stats, literal, [&](auto build, size_t sh) {
        using B = decltype(build);
        if (sampled) hipLaunchKernelGGL((path_lamp_primary_kernel<B::march, B::lds_roots, B::stats, true>), grid, block, sh, st, P, L, S, M);
        else hipLaunchKernelGGL((path_lamp_primary_kernel<B::march, B::lds_roots, B::stats, false>), grid, block, sh, st, P, L, S, M);
    });
}

void launch_path_bounce_lamp(const FrameParams &P, const SunLaunch &S, const LampLaunch &M, bool stats, bool literal, hipStream_t st) {
    if (P.tiles_local == 0) return;
    const dim3 grid = grid_of_records(P.hit_seg_cap), block(256);
    with_march_build(P, stats, literal, [&](auto build, size_t sh) {
        using B = decltype(build);
        hipLaunchKernelGGL((path_lamp_bounce_kernel<B::march, B::lds_roots, B::stats>), grid, block, sh, st, P, S, M);
    });
}

void launch_path_lamp_rays(const FrameParams &P, const LampLaunch &M, bool stats, bool literal, hipStream_t st) {
    if (P.tiles_local == 0) return;
    const dim3 grid = grid_of_records(M.seg_cap), block(256);
    with_march_build(P, stats, literal, [&](auto build, size_t sh) {
        using B = decltype(build);
        hipLaunchKernelGGL((path_lamp_rays_kernel<B::march, B::lds_roots, B::stats>), grid, block, sh, st, P, M);
    });
}

// vrt_set_water_optics (vrt_path_water.h): a water frame is one lane = path launch per segment, as a sun-lit one; each is followed by
// the sun launch if the sun is on as well (S then has buffers).  Its LDS holds the empty liquid set besides the table's
void launch_path_primary_water(const FrameParams &P, const WaterLaunch &W, const SunLaunch &S, bool stats, bool literal, hipStream_t st) {
    if (P.tiles_local == 0) return;
    const dim3 grid = grid_of_tiles(P), block(256);
    const FrameParams D = dry_params(P);
    with_march_build(P, stats, literal, [&](auto build, size_t sh) {
        using B = decltype(build);
        hipLaunchKernelGGL((path_water_primary_kernel<B::march, B::lds_roots, B::stats>), grid, block, sh + 8u * 4u, st, P, D, W, S);
    });
}

void launch_path_bounce_water(const FrameParams &P, const WaterLaunch &W, const SunLaunch &S, bool stats, bool literal, hipStream_t st) {
    if (P.tiles_local == 0) return;
    const dim3 grid = grid_of_records(P.hit_seg_cap), block(256);
    const FrameParams D = dry_params(P);
    with_march_build(P, stats, literal, [&](auto build, size_t sh) {
        using B = decltype(build);
        hipLaunchKernelGGL((path_water_bounce_kernel<B::march, B::lds_roots, B::stats>), grid, block, sh + 8u * 4u, st, P, D, W, S);
    });
}

// vrt_set_water_refraction (vrt_path_refract.h): the same two launches of a water frame whose context has an index of refraction
void launch_path_primary_refract(const FrameParams &P, const WaterLaunch &W, const SunLaunch &S, const RefractLaunch &X, bool stats, bool literal,
                                 hipStream_t st) {
    if (P.tiles_local == 0) return;
    const dim3 grid = grid_of_tiles(P), block(256);
    const FrameParams D = dry_params(P);
    with_march_build(P, stats, literal, [&](auto build, size_t sh) {
        using B = decltype(build);
        hipLaunchKernelGGL((path_refract_primary_kernel<B::march, B::lds_roots, B::stats>), grid, block, sh + 8u * 4u, st, P, D, W, S, X);
    });
}

void launch_path_bounce_refract(const FrameParams &P, const WaterLaunch &W, const SunLaunch &S, const RefractLaunch &X, bool stats, bool literal,
                                hipStream_t st) {
    if (P.tiles_local == 0) return;
    const dim3 grid = grid_of_records(P.hit_seg_cap), block(256);
    const FrameParams D = dry_params(P);
    with_march_build(P, stats, literal, [&](auto build, size_t sh) {
        using B = decltype(build);
        hipLaunchKernelGGL((path_refract_bounce_kernel<B::march, B::lds_roots, B::stats>), grid, block, sh + 8u * 4u, st, P, D, W, S, X);
    });
}

// vrt_set_haze (vrt_path_haze.h): a haze frame is one lane = path launch per segment, as a sun-lit one; each is followed by the sun
// launch if the sun is on as well (S then has buffers)
void launch_path_primary_haze(const FrameParams &P, const HazeLaunch &H, const SunLaunch &S, bool stats, bool literal, hipStream_t st) {
    if (P.tiles_local == 0) return;
    const dim3 grid = grid_of_tiles(P), block(256);
    with_march_build(P, stats, literal, [&](auto build, size_t sh) {
        using B = decltype(build);
        hipLaunchKernelGGL((path_haze_primary_kernel<B::march, B::lds_roots, B::stats>), grid, block, sh, st, P, H, S);
    });
}

void launch_path_bounce_haze(const FrameParams &P, const HazeLaunch &H, const SunLaunch &S, bool stats, bool literal, hipStream_t st) {
    if (P.tiles_local == 0) return;
    const dim3 grid = grid_of_records(P.hit_seg_cap), block(256);
    with_march_build(P, stats, literal, [&](auto build, size_t sh) {
        using B = decltype(build);
        hipLaunchKernelGGL((path_haze_bounce_kernel<B::march, B::lds_roots, B::stats>), grid, block, sh, st, P, H, S);
    });
}

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

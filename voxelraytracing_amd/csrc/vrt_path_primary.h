// vrt_path_primary.h — bounce 0 of the path trace, for vrt_path.hip: path_primary_kernel, one template for the plain frame's
// kernel, the emissive one (EMIT: vrt_write_emission), the one that flips the coat's coin (POLISH: vrt_write_polish; built with
// EMIT alone), the one that draws first whether a hit lets the path through (TRANSLUCENT: vrt_write_translucency; EMIT alone
// again, the coat's draw under a word on the device) and the sun-lit one (SUN: vrt_set_sun_light, vrt_path_sun.h).
#pragma once

#include "vrt_path_common.h"
#include "vrt_path_sun.h"

namespace vrt {

// Bounce 0: primary rays of sample P.sample. Sample 0 initialises the texel {light, id}; later samples add.
// MULTI: the samples of a launch chain (P.acc, P.chain) share the primary march; otherwise one sample, straight into `out`
// EMIT: emissive hits add their light too (vrt_write_emission) — a later sample's texel is then written on those as well
// SUN: nothing, or SunLaunch — the kernel then takes one behind FrameParams, every hit that sees the sun appends a sun ray's
// record, and whether there is a coat or a pass-through draw is read from the launch (POLISH and TRANSLUCENT are then not read).
// Built with EMIT alone, never MULTI.
template <int MARCH, bool LDS_ROOTS, bool STATS, bool MULTI = false, bool EMIT = false, bool POLISH = false, bool TRANSLUCENT = false, class... SUN>
__global__ void __launch_bounds__(256) path_primary_kernel(FrameParams P, SUN... sun) {
    constexpr bool SUNLIT = sizeof...(SUN) != 0;
    const PathLds s = path_lds<STATS>();
    stage_lds(P, s.roots, s.liquid, LDS_ROOTS);

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t t_local = blockIdx.x * 4u + (threadIdx.x >> 6);
    const bool live = t_local < P.tiles_local;
    if (blockIdx.x == 0 && P.seg_clear) P.seg_clear[threadIdx.x * kSegStride] = 0u;   // kHitSegments == blockDim.x cursors
    if constexpr (SUNLIT) {
        if (blockIdx.x == 0) sun_launch(sun...).clear[threadIdx.x * kSegStride] = 0u;
    }
    if (!STATS && !live) return;
    MarchResult R;
    R.iters = 0; R.visits = 0; R.hit = false;
    if (live) {
        const uint32_t tile = shard_tile(t_local, P.shard_first, P.shard_run, P.shard_period);
        uint32_t px, py;
        tile_pixel(P, tile, lane, px, py);
        const uint32_t pixel_slot = P.tile_major ? t_local * 64u + lane : py * P.width + px;
        V3 origin, dir;
        create_ray(P, (int)px, (int)py, origin, dir);
        // every sample of a pixel starts with the same ray (the samples differ from their first bounce on: the RNG is not
        // asked before a hit), so the primary segment is marched once for all the samples of this launch chain
        R = march<MARCH, LDS_ROOTS, STATS, true>(P, s.roots, s.liquid, origin, dir);
        const uint32_t id0 = id_word(R);   // the id word of the primary segment
        for (uint32_t s_local = 0; s_local < (MULTI ? P.chain : 1u); s_local++) {
            const uint32_t sample = P.sample + s_local;
            PathState st;
            st.slot = pixel_slot;
            st.origin = origin;
            st.dir = dir;
            st.thr = V3{1.0f, 1.0f, 1.0f};
            st.rng = sample_seed(P, px, py, sample);
            V3 light{0.f, 0.f, 0.f};
            bool lit, alive, wants = false;
            V3 so, sd, term;   // a sun ray's record (thr is 1: before the hit)
            if constexpr (SUNLIT) {
                const SunLaunch &S = sun_launch(sun...);
                wants = sun_ray_of_hit(P, S, s.liquid, R.hit, R, st.thr, so, sd, term);
                alive = path_after_march_lobes<false>(P, S.lobes, st, R, light, lit) && !P.last_bounce;
            } else {
                alive = path_after_march<EMIT, POLISH, TRANSLUCENT>(P, st, R, light, lit) && !P.last_bounce;
            }
            if (MULTI) {
                // this sample's own plane: its light so far and, for the frame's first sample, the id word (0 otherwise);
                // the path's later segments find the plane through the slot
                st.slot += s_local * P.acc_slots;
                P.acc[st.slot] = make_uint4(__float_as_uint(light.x), __float_as_uint(light.y), __float_as_uint(light.z), sample == 0u ? id0 : 0u);
            } else if (P.sample == 0u) {
                P.out[st.slot] = make_uint4(__float_as_uint(light.x), __float_as_uint(light.y), __float_as_uint(light.z), id0);
            } else if (lit) {
                add_light(P.out, st.slot, light);
            }
            append_paths(P, alive, st, lane);
            if constexpr (SUNLIT) append_light_rays(sun_launch(sun...), wants, st.slot, so, sd, term, 0u, 0u, lane);
        }
        if (STATS && P.steps && P.sample == 0u) P.steps[pixel_slot] = R.iters;
    }
    if (STATS) {
        block_add(s.acc, 0, R.iters);
        block_add(s.acc, 1, R.visits);
        block_add(s.acc, 2, (R.hit && P.sample == 0u) ? 1ull : 0ull);
        __syncthreads();
        if (threadIdx.x == 0) {
            atomicAdd(&P.counters[kCtrSteps], s.acc[0]);
            atomicAdd(&P.counters[kCtrVisits], s.acc[1]);
            atomicAdd(&P.counters[kCtrPrimarySteps], s.acc[0]);
            atomicAdd(&P.counters[kCtrPrimaryVisits], s.acc[1]);
            atomicAdd(&P.counters[kCtrHits], s.acc[2]);
        }
    }
}

}  // namespace vrt

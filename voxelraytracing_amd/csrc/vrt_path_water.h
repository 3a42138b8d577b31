// vrt_path_water.h — water for the path trace (vrt_set_water_optics, include/vrt.h), for vrt_path.hip: the lane = path kernels of a
// water frame.  A segment that starts in a liquid voxel (water_voxel_at, vrt_water.h) is marched with the material table's liquid
// set, as every segment is without the setting, and its throughput is multiplied by e^(-absorb * water_dist) per channel
// (both/water_math.h) ahead of everything else; a segment that starts anywhere else is marched with the empty set, so that a liquid
// voxel stops it like a solid, and such a hit is a surface event: one draw against Schlick's reflectance, the path reflected off
// the face or sent on through it, nothing else.  Every other hit and every miss is path_after_march's and sun_ray_of_hit's text.
//
// One pair of kernels: coat and pass-through are read from the launch (path_after_march_lobes), and so is whether the frame is
// sun-lit too — it then takes a SunLaunch with buffers, appends sun rays as the sun-lit pair does, and is followed by the same
// launch_path_sun.  Both liquid sets are staged in LDS.  Primary rays share the camera's origin, so bounce 0 chooses once per wave;
// a bounce launch marches its dry lanes and then its wet lanes, each with a set and a range that are the same for every lane of the
// march — march_grid reads the range as scalar operands, so the dry segments' parameters are a kernel argument of their own, D
// (vrt_water.h: dry_params).
#pragma once

#include "both/water_math.h"
#include "vrt_path_common.h"
#include "vrt_path_sun.h"
#include "vrt_water.h"

namespace vrt {

// The LDS of a water launch (vrt_path.hip: lds_bytes_path + 32): PathLds' words, the empty liquid set between them and the root table
struct WaterLds {
    uint32_t *liquid, *dry, *roots;
    unsigned long long *acc;
};
template <bool STATS>
__device__ __forceinline__ WaterLds water_lds() {
    extern __shared__ uint32_t smem[];
    const WaterLds s{smem, smem + 24, smem + 32, reinterpret_cast<unsigned long long *>(smem + 8)};
    if (STATS && threadIdx.x < 8) s.acc[threadIdx.x] = 0ull;
    if (threadIdx.x < 8) s.dry[threadIdx.x] = 0u;
    return s;
}

// What follows a segment's march in a water frame (steps 3 to 5 of vrt_set_water_optics' contract).  wet: the segment started in a
// liquid.  Called by every lane that marched; true: the path goes on (st updated).  LATER: a segment behind the primary one —
// its miss takes the sky without the disc when the frame is sun-lit.  wants .. term: the sun ray's record, if the frame is sun-lit.
// (vrt_path_refract.h: refract_after_march restates this text behind its underside event, with the bend in the transmitted branch — a
// change here is made there too; the refracting frames with ior = 1 and the reference hold the two together.)
template <bool LATER>
__device__ __forceinline__ bool water_after_march(const FrameParams &P, const WaterLaunch &W, const SunLaunch &S, const uint32_t *s_liquid, bool wet,
                                                  PathState &st, const MarchResult &R, V3 &light, bool &lit, bool &wants, V3 &so, V3 &sd, V3 &term) {
    if (wet) {   // ahead of the sky's weight, the emission and sun terms, the lobes
        st.thr = V3{st.thr.x * vexp_neg(W.absorb[0] * R.water_dist), st.thr.y * vexp_neg(W.absorb[1] * R.water_dist),
                    st.thr.z * vexp_neg(W.absorb[2] * R.water_dist)};
    }
    const bool surface = !wet && R.hit && is_liquid(s_liquid, R.voxel);
    wants = false;   // (never at a surface event: its voxel is a liquid of the table, which sun_ray_of_hit asks)
    if (W.sun) wants = sun_ray_of_hit(P, S, s_liquid, R.hit, R, st.thr, so, sd, term);
    PathState next = st;
    bool alive = (LATER && W.sun) ? path_after_march_lobes<true>(P, W.lobes, next, R, light, lit) : path_after_march_lobes<false>(P, W.lobes, next, R, light, lit);
    if (surface) {   // the event's one draw; thr as it is, no emission, no sun ray
        const float u = rng_next(st.rng);
        const float dn = vdot(R.norm, st.dir);
        const float c = fabsf(dn), m = 1.0f - c, m5 = (m * m) * (m * m) * m;
        const float F = W.reflectance + (1.0f - W.reflectance) * m5;
        if (u < F) {
            st.origin = V3{R.pos.x + R.norm.x * kShadowBias, R.pos.y + R.norm.y * kShadowBias, R.pos.z + R.norm.z * kShadowBias};
            st.dir = V3{st.dir.x - 2.0f * R.norm.x * dn, st.dir.y - 2.0f * R.norm.y * dn, st.dir.z - 2.0f * R.norm.z * dn};
        } else {
            st.origin = R.pos;
        }
        light = V3{0.f, 0.f, 0.f};   // (a liquid with an emission entry: not here)
        lit = false;
        alive = true;
    } else {
        st = next;
    }
    return alive;
}

// Bounce 0 of a water frame: one sample per chain, straight into `out` (path_primary_kernel's sun-lit form with the choice of the
// liquid set in front of the march).
template <int MARCH, bool LDS_ROOTS, bool STATS>
__global__ void __launch_bounds__(256) path_water_primary_kernel(FrameParams P, FrameParams D, WaterLaunch W, SunLaunch S) {
    const WaterLds s = water_lds<STATS>();
    stage_lds(P, s.roots, s.liquid, LDS_ROOTS);

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t t_local = blockIdx.x * 4u + (threadIdx.x >> 6);
    const bool live = t_local < P.tiles_local;
    if (blockIdx.x == 0) {   // kHitSegments == blockDim.x cursors
        if (P.seg_clear) P.seg_clear[threadIdx.x * kSegStride] = 0u;
        if (W.sun) S.clear[threadIdx.x * kSegStride] = 0u;
    }
    if (!STATS && !live) return;
    MarchResult R;
    R.iters = 0; R.visits = 0; R.hit = false;
    if (live) {
        const uint32_t tile = shard_tile(t_local, P.shard_first, P.shard_run, P.shard_period);
        uint32_t px, py;
        tile_pixel(P, tile, lane, px, py);
        const uint32_t pixel_slot = P.tile_major ? t_local * 64u + lane : py * P.width + px;
        PathState st;
        create_ray(P, (int)px, (int)py, st.origin, st.dir);
        // the camera's voxel: the same for every lane (said to the compiler: the march's range operands are scalars)
        const bool wet = __builtin_amdgcn_readfirstlane((uint32_t)is_liquid(s.liquid, water_voxel_at(P, st.origin))) != 0u;
        if (wet) R = march<MARCH, LDS_ROOTS, STATS, true>(P, s.roots, s.liquid, st.origin, st.dir);
        else R = march<MARCH, LDS_ROOTS, STATS, true>(D, s.roots, s.dry, st.origin, st.dir);
        const uint32_t id0 = id_word(R);   // the id word of the primary segment's own march
        st.slot = pixel_slot;
        st.thr = V3{1.0f, 1.0f, 1.0f};
        st.rng = sample_seed(P, px, py, P.sample);
        V3 light{0.f, 0.f, 0.f};
        bool lit, wants;
        V3 so, sd, term;
        const bool alive = water_after_march<false>(P, W, S, s.liquid, wet, st, R, light, lit, wants, so, sd, term) && !P.last_bounce;
        if (P.sample == 0u) {
            P.out[st.slot] = make_uint4(__float_as_uint(light.x), __float_as_uint(light.y), __float_as_uint(light.z), id0);
        } else if (lit) {
            add_light(P.out, st.slot, light);
        }
        append_paths(P, alive, st, lane);
        if (W.sun) append_light_rays(S, wants, st.slot, so, sd, term, 0u, 0u, lane);
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

// Bounce b >= 1 of a water frame: lane = one live path of the in buffer.
template <int MARCH, bool LDS_ROOTS, bool STATS>
__global__ void __launch_bounds__(256) path_water_bounce_kernel(FrameParams P, FrameParams D, WaterLaunch W, SunLaunch S) {
    const WaterLds s = water_lds<STATS>();
    stage_lds(P, s.roots, s.liquid, LDS_ROOTS);

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t seg = blockIdx.x % kHitSegments, part = blockIdx.x / kHitSegments;
    if (blockIdx.x == 0) {
        if (P.seg_clear) P.seg_clear[threadIdx.x * kSegStride] = 0u;
        if (W.sun) S.clear[threadIdx.x * kSegStride] = 0u;
    }
    bool wants = false;   // a sun ray's record
    V3 so{0.f, 0.f, 0.f}, sd{0.f, 0.f, 0.f}, term{0.f, 0.f, 0.f};
    const uint32_t count = P.seg_in[seg * kSegStride];
    const uint32_t j = part * blockDim.x + threadIdx.x;
    const bool active = j < count;
    if (!STATS && part * blockDim.x >= count) return;
    MarchResult R;
    R.iters = 0; R.visits = 0; R.hit = false;
    R.pos = R.norm = V3{0.f, 0.f, 0.f};
    R.water_dist = 0.0f; R.voxel = 0u; R.trips = 0u;
    bool alive = false, wet = false;
    PathState st;
    st.slot = 0; st.rng = 0;
    st.origin = st.dir = st.thr = V3{0.f, 0.f, 0.f};
    if (active) {
        st = load_path(P, seg * P.hit_seg_cap + j);
        wet = is_liquid(s.liquid, water_voxel_at(P, st.origin));
    }
    // the dry lanes' march, then the wet lanes': the set and the range are the march's
    if (active && !wet) R = march<MARCH, LDS_ROOTS, STATS>(D, s.roots, s.dry, st.origin, st.dir);
    if (active && wet) R = march<MARCH, LDS_ROOTS, STATS>(P, s.roots, s.liquid, st.origin, st.dir);
    if (active) {
        V3 light{0.f, 0.f, 0.f};
        bool lit;
        alive = water_after_march<true>(P, W, S, s.liquid, wet, st, R, light, lit, wants, so, sd, term) && !P.last_bounce;
        if (lit) add_light(P.out, st.slot, light);
        if (STATS && P.steps && P.sample == 0u) P.steps[st.slot] += R.iters << 16;
    }
    append_paths(P, alive, st, lane);
    if (W.sun) append_light_rays(S, wants, st.slot, so, sd, term, 0u, 0u, lane);
    if (STATS) secondary_stats(P, s.acc, active, R);
}

}  // namespace vrt

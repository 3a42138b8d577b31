// vrt_path_haze.h — haze for the path trace (vrt_set_haze, include/vrt.h), for vrt_path.hip: the lane = path kernels of a haze
// frame.  Every segment is marched as the frame without the setting marches it; ahead of everything else it draws a distance t
// (both/haze_math.h: haze_distance), and where t is short of the segment's length in the haze — up to its hit, or to where it leaves
// the world box — the path scatters at x = o + d * t instead of meeting what the march found: thr *= albedo, a sun ray from x if the
// frame is sun-lit (the isotropic phase function: k / 4), a direction drawn uniformly.  A segment without an event is
// path_after_march's and sun_ray_of_hit's text behind that one draw.
//
// One pair of kernels, as the water pair is (vrt_path_water.h): coat and pass-through are read from the launch, and so is whether
// the frame is sun-lit — it then takes a SunLaunch with buffers and is followed by launch_path_sun, which marches a scatter event's
// record exactly as a hit's.  A segment appends the one or the other, never both: one record per slot per launch.
#pragma once

#include "both/haze_math.h"
#include "vrt_path_common.h"
#include "vrt_path_sun.h"

namespace vrt {

// What follows a segment's march in a haze frame (steps 2 to 5 of vrt_set_haze's contract).  Called by every lane that marched;
// true: the path goes on (st updated).  LATER: a segment behind the primary one — its miss takes the sky without the disc when the
// frame is sun-lit.  wants .. term: the sun ray's record, a hit's or an event's, if the frame is sun-lit.
// rng_next_dir and normalize_wave choose their forms by a ballot: the hit's text and the event's both run on copies, in every lane,
// and the lane selects behind them.
template <bool LATER>
__device__ __forceinline__ bool haze_after_march(const FrameParams &P, const HazeLaunch &H, const SunLaunch &S, const uint32_t *s_liquid, PathState &st,
                                                 const MarchResult &R, V3 &light, bool &lit, bool &wants, V3 &so, V3 &sd, V3 &term) {
    const V3 o = st.origin, d = st.dir, thr = st.thr;
    // step 2: the distance draw, ahead of every other draw of the segment
    const float t = haze_distance(rng_next(st.rng), H.inv);
    // step 3: the segment's length in the haze
    const float vx = R.pos.x - o.x, vy = R.pos.y - o.y, vz = R.pos.z - o.z;
    const float oa[3] = {o.x, o.y, o.z}, da[3] = {d.x, d.y, d.z};
    float L = R.hit ? sqrtf((vx * vx + vy * vy) + vz * vz) : haze_exit(oa, da, P.world_max);
    if (!haze_inside(o.x, o.y, o.z, P.world_max)) L = 0.0f;
    const bool event = t < L;   // (a NaN: none)

    // step 5, on copies: the segment of the frame without the setting, behind the one draw
    wants = false;
    if (H.sun) wants = sun_ray_of_hit(P, S, s_liquid, R.hit, R, thr, so, sd, term);
    PathState next = st;
    V3 hl{0.f, 0.f, 0.f};
    bool hlit;
    bool alive = (LATER && H.sun) ? path_after_march_lobes<true>(P, H.lobes, next, R, hl, hlit) : path_after_march_lobes<false>(P, H.lobes, next, R, hl, hlit);

    // step 4, on copies: the scatter event
    uint32_t rng = st.rng;
    const V3 nd = rng_next_dir(rng);
    const V3 x{o.x + d.x * t, o.y + d.y * t, o.z + d.z * t};
    V3 esd{0.f, 0.f, 0.f};
    if (H.sun) esd = normalize_wave(V3{P.sun_local[0] - x.x, P.sun_local[1] - x.y, P.sun_local[2] - x.z});
    if (event) {
        const float q = (esd.x * esd.x + esd.y * esd.y) + esd.z * esd.z;
        const float w = S.k * 0.25f;
        wants = H.sun && q > 0.5f;   // (a zero or a NaN: no ray)
        so = x;
        sd = esd;
        term = V3{(H.albedo[0] * w) * thr.x, (H.albedo[1] * w) * thr.y, (H.albedo[2] * w) * thr.z};
        st.thr = V3{thr.x * H.albedo[0], thr.y * H.albedo[1], thr.z * H.albedo[2]};
        st.origin = x;
        st.dir = nd;
        st.rng = rng;
        light = V3{0.f, 0.f, 0.f};   // (the march's hit is not used: no emission, no sky)
        lit = false;
        alive = true;
    } else {
        st = next;
        light = hl;
        lit = hlit;
    }
    return alive;
}

// Bounce 0 of a haze frame: one sample per chain, straight into `out` (path_primary_kernel's sun-lit form with the distance draw
// behind the march).
template <int MARCH, bool LDS_ROOTS, bool STATS>
__global__ void __launch_bounds__(256) path_haze_primary_kernel(FrameParams P, HazeLaunch H, SunLaunch S) {
    const PathLds s = path_lds<STATS>();
    stage_lds(P, s.roots, s.liquid, LDS_ROOTS);

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t t_local = blockIdx.x * 4u + (threadIdx.x >> 6);
    const bool live = t_local < P.tiles_local;
    if (blockIdx.x == 0) {   // kHitSegments == blockDim.x cursors
        if (P.seg_clear) P.seg_clear[threadIdx.x * kSegStride] = 0u;
        if (H.sun) S.clear[threadIdx.x * kSegStride] = 0u;
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
        R = march<MARCH, LDS_ROOTS, STATS, true>(P, s.roots, s.liquid, st.origin, st.dir);
        const uint32_t id0 = id_word(R);   // the id word of the primary segment's own march, event or not
        st.slot = pixel_slot;
        st.thr = V3{1.0f, 1.0f, 1.0f};
        st.rng = sample_seed(P, px, py, P.sample);
        V3 light{0.f, 0.f, 0.f};
        bool lit, wants;
        V3 so, sd, term;
        const bool alive = haze_after_march<false>(P, H, S, s.liquid, st, R, light, lit, wants, so, sd, term) && !P.last_bounce;
        if (P.sample == 0u) {
            P.out[st.slot] = make_uint4(__float_as_uint(light.x), __float_as_uint(light.y), __float_as_uint(light.z), id0);
        } else if (lit) {
            add_light(P.out, st.slot, light);
        }
        append_paths(P, alive, st, lane);
        if (H.sun) append_light_rays(S, wants, st.slot, so, sd, term, 0u, 0u, lane);
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

// Bounce b >= 1 of a haze frame: lane = one live path of the in buffer.
template <int MARCH, bool LDS_ROOTS, bool STATS>
__global__ void __launch_bounds__(256) path_haze_bounce_kernel(FrameParams P, HazeLaunch H, SunLaunch S) {
    const PathLds s = path_lds<STATS>();
    stage_lds(P, s.roots, s.liquid, LDS_ROOTS);

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t seg = blockIdx.x % kHitSegments, part = blockIdx.x / kHitSegments;
    if (blockIdx.x == 0) {
        if (P.seg_clear) P.seg_clear[threadIdx.x * kSegStride] = 0u;
        if (H.sun) S.clear[threadIdx.x * kSegStride] = 0u;
    }
    bool wants = false;   // a sun ray's record
    V3 so{0.f, 0.f, 0.f}, sd{0.f, 0.f, 0.f}, term{0.f, 0.f, 0.f};
    const uint32_t count = P.seg_in[seg * kSegStride];
    const uint32_t j = part * blockDim.x + threadIdx.x;
    const bool active = j < count;
    if (!STATS && part * blockDim.x >= count) return;
    MarchResult R;
    R.iters = 0; R.visits = 0; R.hit = false;
    bool alive = false;
    PathState st;
    st.slot = 0; st.rng = 0;
    st.origin = st.dir = st.thr = V3{0.f, 0.f, 0.f};
    if (active) {
        st = load_path(P, seg * P.hit_seg_cap + j);
        R = march<MARCH, LDS_ROOTS, STATS>(P, s.roots, s.liquid, st.origin, st.dir);
        V3 light{0.f, 0.f, 0.f};
        bool lit;
        alive = haze_after_march<true>(P, H, S, s.liquid, st, R, light, lit, wants, so, sd, term) && !P.last_bounce;
        if (lit) add_light(P.out, st.slot, light);
        if (STATS && P.steps && P.sample == 0u) P.steps[st.slot] += R.iters << 16;
    }
    append_paths(P, alive, st, lane);
    if (H.sun) append_light_rays(S, wants, st.slot, so, sd, term, 0u, 0u, lane);
    if (STATS) secondary_stats(P, s.acc, active, R);
}

}  // namespace vrt

// vrt_path_refract.h — refraction for water (vrt_set_water_refraction, include/vrt.h), for vrt_path.hip: the lane = path kernels of
// a water frame whose context has an index of refraction.  They are vrt_path_water.h's pair with three things added
// (both/refract_math.h holds the arithmetic, the host mirror's too):
//   A  a surface event's transmitted branch bends the direction (refract_enter);
//   B  a wet segment first walks cast_ray's DDA through the body of liquid it starts in, at most X.max_span unit voxels, to the
//      first voxel that is no liquid (refract_walk: water_voxel_at's look-up per step).  The walk runs in front of the march and
//      leaves three words — dist, the face, a flag — so nothing of it is live across the march;
//   C  where that voxel is air the segment ends in an underside event: absorbed over dist, then mirrored back into the water
//      (always, past the critical angle) or bent out into the air.  Nothing else of the segment's march is used; a bounce launch
//      that counts nothing does not march such a lane at all.
// Every other segment is the water pair's, word for word (refract_after_march's second half is water_after_march's text).
#pragma once

#include "both/refract_math.h"
#include "vrt_path_water.h"

namespace vrt {

// What the walk leaves: face = the axis the walk left the water along (0 x, 1 y, 2 z) | 4 where the normal back into the water
// points down that axis; dist: the exit's distance along the segment
struct SpanExit {
    bool event;
    uint32_t face;
    float dist;
};
__device__ __forceinline__ V3 span_normal(const SpanExit &e) {
    const float s = (e.face & 4u) ? -1.0f : 1.0f;
    const uint32_t a = e.face & 3u;
    return V3{a == 0u ? s : 0.0f, a == 1u ? s : 0.0f, a == 2u ? s : 0.0f};
}

// B.  Divergent per lane and short; called by the lanes whose segment is wet
__device__ __forceinline__ SpanExit refract_walk(const FrameParams &P, const uint32_t *s_liquid, uint32_t max_span, V3 o, V3 d) {
    const float o3[3] = {o.x, o.y, o.z}, d3[3] = {d.x, d.y, d.z};
    const WaterSpan w = water_span(
        o3, d3, max_span,
        [&](int32_t x, int32_t y, int32_t z) { return water_voxel_at(P, V3{(float)x + 0.5f, (float)y + 0.5f, (float)z + 0.5f}); },   // (exact: |x| < 2^23)
        [&](uint32_t v) { return is_liquid(s_liquid, v); });
    // n = prev - m: one axis, one unit
    const int32_t nx = w.prev[0] - w.m[0], ny = w.prev[1] - w.m[1], nz = w.prev[2] - w.m[2];
    const uint32_t axis = nx != 0 ? 0u : (ny != 0 ? 1u : 2u);
    return SpanExit{w.event, axis | ((nx + ny + nz) < 0 ? 4u : 0u), w.dist};
}

// water_after_march with A and C.  ev: the segment's walk (event false for a dry segment)
template <bool LATER>
__device__ __forceinline__ bool refract_after_march(const FrameParams &P, const WaterLaunch &W, const SunLaunch &S, const RefractLaunch &X,
                                                    const uint32_t *s_liquid, bool wet, const SpanExit &ev, PathState &st, const MarchResult &R, V3 &light,
                                                    bool &lit, bool &wants, V3 &so, V3 &sd, V3 &term) {
    if (wet && ev.event) {   // C: the underside event
        st.thr = V3{st.thr.x * vexp_neg(W.absorb[0] * ev.dist), st.thr.y * vexp_neg(W.absorb[1] * ev.dist), st.thr.z * vexp_neg(W.absorb[2] * ev.dist)};
        light = V3{0.f, 0.f, 0.f};
        lit = false;
        wants = false;
        if (P.last_bounce) return false;   // (nothing is drawn)
        const float u = rng_next(st.rng);
        const V3 n = span_normal(ev);
        const V3 x{st.origin.x + st.dir.x * ev.dist, st.origin.y + st.dir.y * ev.dist, st.origin.z + st.dir.z * ev.dist};
        const float d3[3] = {st.dir.x, st.dir.y, st.dir.z}, n3[3] = {n.x, n.y, n.z};
        float out[3];
        const int branch = refract_leave(X.ior, W.reflectance, d3, n3, u, out);
        const float side = branch == kRefractLeft ? -1.0f : 1.0f;   // (x - n * bias is x + (-n) * bias, bit for bit)
        st.origin = V3{x.x + (n.x * side) * kShadowBias, x.y + (n.y * side) * kShadowBias, x.z + (n.z * side) * kShadowBias};
        st.dir = V3{out[0], out[1], out[2]};
        return true;
    }
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
        } else {   // A
            const float d3[3] = {st.dir.x, st.dir.y, st.dir.z}, n3[3] = {R.norm.x, R.norm.y, R.norm.z};
            float out[3];
            refract_enter(X.eta, d3, n3, out);
            st.origin = R.pos;
            st.dir = V3{out[0], out[1], out[2]};
        }
        light = V3{0.f, 0.f, 0.f};   // (a liquid with an emission entry: not here)
        lit = false;
        alive = true;
    } else {
        st = next;
    }
    return alive;
}

// Bounce 0 of a refracting water frame: path_water_primary_kernel with the walk in front of a wet camera's march.  The wet choice
// stays the wave's, and the march is always run: the texel's id word and a stats frame's counts are its own
template <int MARCH, bool LDS_ROOTS, bool STATS>
__global__ void __launch_bounds__(256) path_refract_primary_kernel(FrameParams P, FrameParams D, WaterLaunch W, SunLaunch S, RefractLaunch X) {
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
        SpanExit ev{false, 0u, 0.0f};
        if (wet) {
            ev = refract_walk(P, s.liquid, X.max_span, st.origin, st.dir);
            R = march<MARCH, LDS_ROOTS, STATS, true>(P, s.roots, s.liquid, st.origin, st.dir);
        } else {
            R = march<MARCH, LDS_ROOTS, STATS, true>(D, s.roots, s.dry, st.origin, st.dir);
        }
        const uint32_t id0 = id_word(R);   // the id word of the primary segment's own march
        st.slot = pixel_slot;
        st.thr = V3{1.0f, 1.0f, 1.0f};
        st.rng = sample_seed(P, px, py, P.sample);
        V3 light{0.f, 0.f, 0.f};
        bool lit, wants;
        V3 so, sd, term;
        const bool alive = refract_after_march<false>(P, W, S, X, s.liquid, wet, ev, st, R, light, lit, wants, so, sd, term) && !P.last_bounce;
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

// Bounce b >= 1 of a refracting water frame: path_water_bounce_kernel with the wet lanes' walk in front of both marches.  A wet
// lane whose walk ends in an event is marched only where the march is counted (STATS)
template <int MARCH, bool LDS_ROOTS, bool STATS>
__global__ void __launch_bounds__(256) path_refract_bounce_kernel(FrameParams P, FrameParams D, WaterLaunch W, SunLaunch S, RefractLaunch X) {
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
    SpanExit ev{false, 0u, 0.0f};
    PathState st;
    st.slot = 0; st.rng = 0;
    st.origin = st.dir = st.thr = V3{0.f, 0.f, 0.f};
    if (active) {
        st = load_path(P, seg * P.hit_seg_cap + j);
        wet = is_liquid(s.liquid, water_voxel_at(P, st.origin));
    }
    if (active && wet) ev = refract_walk(P, s.liquid, X.max_span, st.origin, st.dir);
    // the dry lanes' march, then the wet lanes': the set and the range are the march's
    if (active && !wet) R = march<MARCH, LDS_ROOTS, STATS>(D, s.roots, s.dry, st.origin, st.dir);
    if (active && wet && (STATS || !ev.event)) R = march<MARCH, LDS_ROOTS, STATS>(P, s.roots, s.liquid, st.origin, st.dir);
    if (active) {
        V3 light{0.f, 0.f, 0.f};
        bool lit;
        alive = refract_after_march<true>(P, W, S, X, s.liquid, wet, ev, st, R, light, lit, wants, so, sd, term) && !P.last_bounce;
        if (lit) add_light(P.out, st.slot, light);
        if (STATS && P.steps && P.sample == 0u) P.steps[st.slot] += R.iters << 16;
    }
    append_paths(P, alive, st, lane);
    if (W.sun) append_light_rays(S, wants, st.slot, so, sd, term, 0u, 0u, lane);
    if (STATS) secondary_stats(P, s.acc, active, R);
}

}  // namespace vrt

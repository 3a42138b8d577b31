// vrt_path_lamp.h — lamp light for the path trace (vrt_set_lamp_light, include/vrt.h), for vrt_path.hip: the kernels of a lamp-lit
// frame.  Every hit takes three draws, picks an entry of the lamp list (vrt_lamp.hip) and a point of that face, and — where the
// face and the surface look at each other — appends a record: its texel's slot, the ray (the bounce origin, the direction to the
// point), the term ((mc * lc) * w) * thr and the lamp voxel's coordinates.  A launch of its own behind each trace launch marches
// the records and adds the terms of the rays that stop on their lamp voxel; stream order puts a segment's lamp term behind its
// emission and sun terms and ahead of the next segment's, one record per slot per launch keeps the read-modify-write plain.
//
// One pair of trace kernels carries the sun term too (vrt_path_sun.h's, under M.sun: the same for every lane) and reads coat and
// pass-through from the launch, as the sun-lit pair does; the primary kernel is built with and without camera sampling
// (vrt_path_lens.h's sample loop: the pixel's own pinhole ray is trip -1).  Kernels of their own: every kernel from before keeps
// its instruction stream (profiles/lamp_isa_diff.txt).  The path record's spare word — the third plane's .w —
// carries whether the path is still direct: its emissive hits count only until its first bounce, behind which the lamp term
// has them.
#pragma once

#include "vrt_path_common.h"
#include "vrt_path_sun.h"
#include "vrt_path_lens.h"

namespace vrt {

// what a hit's lane appends for the lamp launch
struct LampRay {
    bool wants;
    V3 so, ld, term;
    uint32_t pxy, pz;   // the lamp voxel: x | y << 16, z
};

// materials[min(voxel, 255)].color under hit_color's face factors for `face` (never the step-count grey)
__device__ __forceinline__ V3 lamp_face_color(const FrameParams &P, uint32_t voxel, uint32_t face) {
    const vrt_material *m = &P.mats[min(voxel, 255u)];
    V3 lc{m->color[0], m->color[1], m->color[2]};
    if ((face >> 1) == 0u) { lc.x *= 0.5f; lc.y *= 0.5f; lc.z *= 0.5f; }
    if ((face >> 1) == 2u) { lc.x *= 0.7f; lc.y *= 0.7f; lc.z *= 0.7f; }
    if (face == 2u) { lc.x *= 0.2f; lc.y *= 0.2f; lc.z *= 0.2f; }
    return lc;
}

// Step 5 of vrt_set_lamp_light's contract for one hit.  n: the list's length (the same for every lane); thr: the throughput
// before the hit; u1, u2, u3: the hit's three draws.
__device__ __forceinline__ LampRay lamp_ray_of_hit(const FrameParams &P, const LampLaunch &M, uint32_t n, const uint32_t *s_liquid, const MarchResult &R,
                                                   const V3 &thr, float u1, float u2, float u3) {
    LampRay r;
    const bool solid = R.hit && R.voxel != 0u && !is_liquid(s_liquid, R.voxel) && n != 0u;
    r.so = V3{R.pos.x + R.norm.x * kShadowBias, R.pos.y + R.norm.y * kShadowBias, R.pos.z + R.norm.z * kShadowBias};
    uint4 L = make_uint4(0u, 0u, 0u, 0u);
    if (solid) {
        const uint32_t j = min((uint32_t)(u1 * (float)n), n - 1u);   // (u1 <= 1, n <= 2^24, VRT_LAMP_CAP's most: in range)
        L = M.list[j];
    }
    const uint32_t px = L.x & 0xFFFFu, py = L.x >> 16, pz = L.y & 0xFFFFu, voxel = L.y >> 16, face = L.z;
    const uint32_t a = face >> 1, s = face & 1u;
    const float fs = (float)s;
    const V3 q{(float)px + (a == 0u ? fs : u2), (float)py + (a == 1u ? fs : (a == 0u ? u2 : u3)), (float)pz + (a == 2u ? fs : u3)};
    const V3 v{q.x - r.so.x, q.y - r.so.y, q.z - r.so.z};
    const float d2 = (v.x * v.x + v.y * v.y) + v.z * v.z;
    r.ld = normalize_wave(v);
    const float c = vdot(R.norm, r.ld);
    const float la = a == 0u ? r.ld.x : (a == 1u ? r.ld.y : r.ld.z);
    const float cl = s ? -la : la;
    float g = (c * cl) / d2;
    if (M.max_geometry != 0.0f && g > M.max_geometry) g = M.max_geometry;
    const float k = ((M.strength * emission_table(P.mats)[min(voxel, 255u)]) * 0.318309886f) * (float)n;
    const float w = k * g;
    const V3 mc = hit_color(P, R), lc = lamp_face_color(P, voxel, face);
    r.term = V3{((mc.x * lc.x) * w) * thr.x, ((mc.y * lc.y) * w) * thr.y, ((mc.z * lc.z) * w) * thr.z};
    r.pxy = L.x;
    r.pz = pz;
    r.wants = solid && c > 0.0f && cl > 0.0f;   // (a NaN: no ray)
    return r;
}

// What follows a segment's march in a lamp-lit frame (the hit's three draws are taken by the caller, ahead of this): the sky of a
// miss — without the disc for a later segment of a frame that is sun-lit too — or path_after_march with the emission term, kept
// only while the path is direct, and the coat's coin or the pass-through draw as the frame has them.  direct: in, the path
// before this hit; out, behind it — a pass-through keeps it, a bounce ends it.
template <bool LATER>
__device__ __forceinline__ bool path_after_march_lamp(const FrameParams &P, const LampLaunch &M, PathState &st, const MarchResult &R, V3 &light, bool &lit,
                                                      bool &direct) {
    if (!R.hit) {
        const V3 sky = (LATER && M.sun) ? ray_sky<false, true>(P, st.origin, st.dir) : ray_sky<false, false>(P, st.origin, st.dir);
        light = V3{sky.x * st.thr.x, sky.y * st.thr.y, sky.z * st.thr.z};
        lit = true;
        return false;
    }
    bool passes = false;
    if (M.lobes & kSunLobeTranslucent) {   // path_translucent_hit's own first draw and test, looked at ahead of it
        uint32_t peek = st.rng;
        passes = rng_next(peek) < translucency_table(P.mats)[min(R.voxel, 255u)].chance;
    }
    const bool alive = path_after_march_lobes(P, M.lobes, st, R, light, lit);
    if (!direct) lit = false;   // (behind the first bounce the lamp term has the lamps)
    if (!passes) direct = false;
    return alive;
}

// the launches' arguments in the kernarg segment (vrt_path_lens.h: fresh_kernarg), for the sample loop of the camera-sampling form
constexpr size_t kLampLensAt = kernarg_after(sizeof(FrameParams), alignof(LensLaunch));
constexpr size_t kLampSunAt = kernarg_after(kLampLensAt + sizeof(LensLaunch), alignof(SunLaunch));
constexpr size_t kLampAt = kernarg_after(kLampSunAt + sizeof(SunLaunch), alignof(LampLaunch));

// Bounce 0 of a lamp-lit frame: one sample per chain, straight into `out`.  LENS: vrt_set_camera_sampling is on — the sample's own
// primary ray from four draws, the pixel's pinhole ray marched once more for the id word by the launch of the frame's first sample.
template <int MARCH, bool LDS_ROOTS, bool STATS, bool LENS>
__global__ void __launch_bounds__(256) path_lamp_primary_kernel(FrameParams P, LensLaunch L, SunLaunch S, LampLaunch M) {
    const PathLds s = path_lds<STATS>();
    stage_lds(P, s.roots, s.liquid, LDS_ROOTS);

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t t_local = blockIdx.x * 4u + (threadIdx.x >> 6);
    const bool live = t_local < P.tiles_local;
    if (blockIdx.x == 0) {   // kHitSegments == blockDim.x cursors
        if (P.seg_clear) P.seg_clear[threadIdx.x * kSegStride] = 0u;
        M.clear[threadIdx.x * kSegStride] = 0u;
        if (M.sun) S.clear[threadIdx.x * kSegStride] = 0u;
    }
    if (!STATS && !live) return;
    uint32_t iters = 0, visits = 0;
    bool centre_hit = false;
    if (live) {
        const uint32_t tile = shard_tile(t_local, P.shard_first, P.shard_run, P.shard_period);
        uint32_t px, py;
        tile_pixel(P, tile, lane, px, py);
        const uint32_t pixel_slot = P.tile_major ? t_local * 64u + lane : py * P.width + px;
        uint32_t id0 = 0u;
        for (int s_local = (LENS && P.sample == 0u) ? -1 : 0; s_local < 1; s_local++) {
            const FrameParams &Q = LENS ? fresh_kernarg<FrameParams, 0>() : P;   // (this trip's: vrt_path_lens.h)
            // (the launches behind FrameParams always: read next to their use behind the march, not held in scalar registers across it)
            const LensLaunch &LQ = fresh_kernarg<LensLaunch, kLampLensAt>();
            const SunLaunch &SQ = fresh_kernarg<SunLaunch, kLampSunAt>();
            const LampLaunch &MQ = fresh_kernarg<LampLaunch, kLampAt>();
            PathState st;
            st.slot = pixel_slot;
            st.thr = V3{1.0f, 1.0f, 1.0f};
            st.rng = py * Q.width + px + (Q.sample_base + Q.sample) * (Q.width * Q.height) + Q.seed * 0x9E3779B9u;   // (sample_seed's text, vrt_path_common.h)
            MarchResult R;
            if (LENS) {
                if (s_local < 0) create_ray(Q, (int)px, (int)py, st.origin, st.dir);
                else lens_ray(Q, LQ, px, py, st.rng, st.origin, st.dir);
                R = march<MARCH, LDS_ROOTS, STATS>(Q, s.roots, s.liquid, st.origin, st.dir);
            } else {
                create_ray(Q, (int)px, (int)py, st.origin, st.dir);
                R = march<MARCH, LDS_ROOTS, STATS, true>(Q, s.roots, s.liquid, st.origin, st.dir);
            }
            if (STATS) {
                iters += R.iters;
                visits += R.visits;
            }
            if (!LENS || s_local < 0) {   // the id word of the pixel's own ray
                id0 = id_word(R);
                centre_hit = R.hit && Q.sample == 0u;
                if (STATS && Q.steps && Q.sample == 0u) Q.steps[pixel_slot] = R.iters;
            }
            if (LENS && s_local < 0) continue;
            const uint32_t n_lamps = __builtin_amdgcn_readfirstlane(*MQ.n);
            float u1 = 0.0f, u2 = 0.0f, u3 = 0.0f;
            if (R.hit) { u1 = rng_next(st.rng); u2 = rng_next(st.rng); u3 = rng_next(st.rng); }
            V3 so{0.f, 0.f, 0.f}, sd{0.f, 0.f, 0.f}, sterm{0.f, 0.f, 0.f};   // (thr is 1: before the hit)
            bool sun = false;
            if (MQ.sun) sun = sun_ray_of_hit(Q, SQ, s.liquid, R.hit, R, st.thr, so, sd, sterm);
            const LampRay lr = lamp_ray_of_hit(Q, MQ, n_lamps, s.liquid, R, st.thr, u1, u2, u3);
            V3 light{0.f, 0.f, 0.f};
            bool lit, direct = true;
            const bool alive = path_after_march_lamp<false>(Q, MQ, st, R, light, lit, direct) && !Q.last_bounce;
            if (Q.sample == 0u) {
                Q.out[st.slot] = make_uint4(__float_as_uint(light.x), __float_as_uint(light.y), __float_as_uint(light.z), id0);
            } else if (lit) {
                add_light(Q.out, st.slot, light);
            }
            append_paths(Q, alive, st, lane, direct);
            if (MQ.sun) append_light_rays(SQ, sun, st.slot, so, sd, sterm, 0u, 0u, lane);
            append_light_rays(MQ, lr.wants, st.slot, lr.so, lr.ld, lr.term, lr.pxy, lr.pz, lane);
        }
    }
    if (STATS) {
        block_add(s.acc, 0, iters);
        block_add(s.acc, 1, visits);
        block_add(s.acc, 2, centre_hit ? 1ull : 0ull);
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

// Bounce b >= 1 of a lamp-lit frame: lane = one live path of the in buffer.
template <int MARCH, bool LDS_ROOTS, bool STATS>
__global__ void __launch_bounds__(256) path_lamp_bounce_kernel(FrameParams P, SunLaunch S, LampLaunch M) {
    const PathLds s = path_lds<STATS>();
    stage_lds(P, s.roots, s.liquid, LDS_ROOTS);

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t seg = blockIdx.x % kHitSegments, part = blockIdx.x / kHitSegments;
    if (blockIdx.x == 0) {
        if (P.seg_clear) P.seg_clear[threadIdx.x * kSegStride] = 0u;
        M.clear[threadIdx.x * kSegStride] = 0u;
        if (M.sun) S.clear[threadIdx.x * kSegStride] = 0u;
    }
    const uint32_t count = P.seg_in[seg * kSegStride];
    const uint32_t j = part * blockDim.x + threadIdx.x;
    const bool active = j < count;
    if (!STATS && part * blockDim.x >= count) return;
    const uint32_t n_lamps = __builtin_amdgcn_readfirstlane(*M.n);
    MarchResult R;
    R.iters = 0; R.visits = 0; R.hit = false;
    bool alive = false, direct = false, sun = false;
    V3 so{0.f, 0.f, 0.f}, sd{0.f, 0.f, 0.f}, sterm{0.f, 0.f, 0.f};
    LampRay lr;
    lr.wants = false;
    lr.so = lr.ld = lr.term = V3{0.f, 0.f, 0.f};
    lr.pxy = lr.pz = 0u;
    PathState st;
    st.slot = 0; st.rng = 0;
    st.origin = st.dir = st.thr = V3{0.f, 0.f, 0.f};
    if (active) {
        st = load_path(P, seg * P.hit_seg_cap + j);
        direct = path_spare_word(P, seg * P.hit_seg_cap + j) != 0u;
        V3 light{0.f, 0.f, 0.f};
        bool lit;
        R = march<MARCH, LDS_ROOTS, STATS>(P, s.roots, s.liquid, st.origin, st.dir);
        float u1 = 0.0f, u2 = 0.0f, u3 = 0.0f;
        if (R.hit) { u1 = rng_next(st.rng); u2 = rng_next(st.rng); u3 = rng_next(st.rng); }
        if (M.sun) sun = sun_ray_of_hit(P, S, s.liquid, R.hit, R, st.thr, so, sd, sterm);   // (thr: before the hit)
        lr = lamp_ray_of_hit(P, M, n_lamps, s.liquid, R, st.thr, u1, u2, u3);
        alive = path_after_march_lamp<true>(P, M, st, R, light, lit, direct) && !P.last_bounce;
        if (lit) add_light(P.out, st.slot, light);
        if (STATS && P.steps && P.sample == 0u) P.steps[st.slot] += R.iters << 16;
    }
    append_paths(P, alive, st, lane, direct);
    if (M.sun) append_light_rays(S, sun, st.slot, so, sd, sterm, 0u, 0u, lane);
    append_light_rays(M, lr.wants, st.slot, lr.so, lr.ld, lr.term, lr.pxy, lr.pz, lane);
    if (STATS) secondary_stats(P, s.acc, active, R);
}

// The lamp launch: lane = one record of the trace launch in front of it, marched by march<> — which also counts: a stats frame's
// steps and node visits include the lamp marches, its secondary rays the lamp rays.  The term is added where the march stops on
// the record's lamp voxel.
template <int MARCH, bool LDS_ROOTS, bool STATS>
__global__ void __launch_bounds__(256) path_lamp_rays_kernel(FrameParams P, LampLaunch M) {
    const PathLds s = path_lds<STATS>();
    stage_lds(P, s.roots, s.liquid, LDS_ROOTS);
    const uint32_t seg = blockIdx.x % kHitSegments, part = blockIdx.x / kHitSegments;
    const uint32_t count = min(M.counts[seg * kSegStride], M.seg_cap);
    const uint32_t j = part * blockDim.x + threadIdx.x;
    const bool active = j < count;
    if (!STATS && part * blockDim.x >= count) return;
    MarchResult R;
    R.iters = 0; R.visits = 0; R.hit = false;
    if (active) {
        const uint32_t i = seg * M.seg_cap + j;
        const uint4 a = M.recs[i], b = M.recs[M.cap + i], c = M.recs[2u * M.cap + i];
        const V3 so{__uint_as_float(a.y), __uint_as_float(a.z), __uint_as_float(a.w)};
        const V3 ld{__uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z)};
        R = march<MARCH, LDS_ROOTS, STATS>(P, s.roots, s.liquid, so, ld);
        // (a hit position is inside the world: its floor is a small non-negative integer)
        const bool on_lamp = R.hit && (int)floorf(R.pos.x) == (int)(b.w & 0xFFFFu) && (int)floorf(R.pos.y) == (int)(b.w >> 16) &&
                             (int)floorf(R.pos.z) == (int)c.w;
        if (on_lamp) add_light(P.out, a.x, V3{__uint_as_float(c.x), __uint_as_float(c.y), __uint_as_float(c.z)});
    }
    if (STATS) {
        block_add(s.acc, 0, active ? R.iters : 0u);
        block_add(s.acc, 1, active ? R.visits : 0u);
        block_add(s.acc, 2, active ? 1ull : 0ull);
        __syncthreads();
        if (threadIdx.x == 0 && s.acc[2]) {
            atomicAdd(&P.counters[kCtrSteps], s.acc[0]);
            atomicAdd(&P.counters[kCtrVisits], s.acc[1]);
            atomicAdd(&P.counters[kCtrSecondary], s.acc[2]);
        }
    }
}

}  // namespace vrt

// vrt_path_lens.h — bounce 0 of a path frame with camera sampling (vrt_set_camera_sampling, include/vrt.h), for vrt_path.hip:
// path_lens_primary_kernel, and with a SunLaunch behind the LensLaunch the form for the frames of a context with vrt_set_sun_light
// as well (a sun ray's record from each sample's own hit).  A kernel of its own, as the lamp-lit ones are: a context with the
// setting off launches exactly what it launched.  Whether the frame has an emission term, a coat or a pass-through draw is read
// from the launch (L.lobes, S.lobes: scalar branches), not built as a family per combination.
//
// Every sample builds its own primary ray from four draws of its stream (csrc/both/lens_math.h, the text the host mirror
// compiles too) and marches it as an ordinary segment: its origin is no longer the camera's.  The pixel's own pinhole ray —
// what the id word, vrt_read_steps, the hit count and the denoiser's key come from — is marched by the launch that holds the
// frame's first sample and shaded by nobody.  It is trip -1 of the sample loop (P.sample == 0 is the same for every wave of a
// launch), so the kernel holds ONE inlined march: the centre ray's result is down to its id word before a sample's march
// begins, and nothing of a march is live across the loop's back edge but the counts of a stats frame.
#pragma once

#include "vrt_path_common.h"
#include "vrt_path_sun.h"
#include "both/lens_math.h"

namespace vrt {

// A sample's own primary ray (steps 1 to 3 of the contract): four draws, both/lens_math.h's two halves, the two normalisations.
// Called by every lane of the wave.  The two IEEE divides and the square root take vrt_march.h's refined forms when every lane's
// operands are in their range (a ballot each; a zero numerator is: +-0 / d is +-0 from either form) — proj_size is the frame's, a
// numerator is a pixel coordinate doubled, u3 is 0 once in 2^32 draws and at least 2^-32 otherwise.
__device__ __forceinline__ void lens_ray(const FrameParams &P, const LensLaunch &L, uint32_t px, uint32_t py, uint32_t &rng, V3 &origin, V3 &dir) {
    const float *proj_size = P.cam.proj_size, *ip = P.cam.inv_proj_mat, *iv = P.cam.inv_view_mat;
    const V3 cam{P.cam_origin[0], P.cam_origin[1], P.cam_origin[2]};
    const float u1 = rng_next(rng), u2 = rng_next(rng), u3 = rng_next(rng), u4 = rng_next(rng);
    auto div = [](float n, float d) { return lens_div(n, d); };   // (vrt_path_common.h)
    const LensV3 w = lens_pixel_dir(px, py, u1, u2, L.pixel_spread, proj_size, ip, iv, div);
    dir = normalize_wave(V3{w.x, w.y, w.z});
    origin = cam;
    if (L.aperture != 0.0f) {   // (the launch's: a scalar branch)
        auto sqrt_of = [](float x) { return lens_sqrt_of(x); };
        LensV3 o, v;
        lens_thin(LensV3{cam.x, cam.y, cam.z}, LensV3{dir.x, dir.y, dir.z}, u3, u4, L.aperture, L.focus_distance, iv, sqrt_of, o, v);
        origin = V3{o.x, o.y, o.z};
        dir = normalize_wave(V3{v.x, v.y, v.z});
    }
}

// A kernel argument — FrameParams, the first, at the start of the kernarg segment; the launches behind it, each at the next
// multiple of its alignment — through a pointer the compiler cannot see through.  The sample loop takes them anew per trip:
// what a trip reads of the frame is then scalar loads of that trip, next to their use, as in the kernels that have no loop.
// Read through the arguments themselves, every word the loop's body uses anywhere — the camera's 37, the march's descriptors,
// the sky's and the sun's constants — was hoisted in front of the loop and held in a scalar register across the march, more
// than there are: up to 43 were spilled.
template <class T, size_t OFFSET>
__device__ __forceinline__ const T &fresh_kernarg() {
    typedef const char __attribute__((address_space(4))) *Kernarg;
    typedef const T __attribute__((address_space(4))) *Arg;
    Kernarg q = (Kernarg)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(q));
    return *(const T *)(Arg)(q + OFFSET);
}
constexpr size_t kernarg_after(size_t end, size_t align) { return (end + align - 1) / align * align; }
constexpr size_t kLensLaunchAt = kernarg_after(sizeof(FrameParams), alignof(LensLaunch));
constexpr size_t kLensSunLaunchAt = kernarg_after(kLensLaunchAt + sizeof(LensLaunch), alignof(SunLaunch));

// MULTI: the samples of a launch chain (P.acc, P.chain), each into its own plane; otherwise one sample, straight into `out`
// SUN: nothing, or SunLaunch (vrt_path_primary.h)
template <int MARCH, bool LDS_ROOTS, bool STATS, bool MULTI = false, class... SUN>
__global__ void __launch_bounds__(256) path_lens_primary_kernel(FrameParams P, LensLaunch L, SUN... sun) {
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
    uint32_t iters = 0, visits = 0;   // (a stats frame: the centre march and every sample's own)
    bool centre_hit = false;
    if (live) {
        const uint32_t tile = shard_tile(t_local, P.shard_first, P.shard_run, P.shard_period);
        uint32_t px, py;
        tile_pixel(P, tile, lane, px, py);
        const uint32_t pixel_slot = P.tile_major ? t_local * 64u + lane : py * P.width + px;
        uint32_t id0 = 0u;
        const int chain = (int)(MULTI ? P.chain : 1u);
        for (int s_local = P.sample == 0u ? -1 : 0; s_local < chain; s_local++) {
            const FrameParams &Q = fresh_kernarg<FrameParams, 0>();   // (this trip's: see there)
            const LensLaunch &LQ = fresh_kernarg<LensLaunch, kLensLaunchAt>();
            const SunLaunch *SQ = nullptr;
            if constexpr (SUNLIT) SQ = &fresh_kernarg<SunLaunch, kLensSunLaunchAt>();
            const uint32_t sample = Q.sample + (uint32_t)s_local;
            PathState st;
            st.slot = pixel_slot;
            st.thr = V3{1.0f, 1.0f, 1.0f};
            if (s_local < 0) {
                create_ray(Q, (int)px, (int)py, st.origin, st.dir);
                st.rng = 0u;
            } else {
                st.rng = sample_seed(Q, px, py, sample);   // (the sample's first four draws are its ray's)
                lens_ray(Q, LQ, px, py, st.rng, st.origin, st.dir);
            }
            const MarchResult R = march<MARCH, LDS_ROOTS, STATS>(Q, s.roots, s.liquid, st.origin, st.dir);
            if (STATS) {
                iters += R.iters;
                visits += R.visits;
            }
            if (s_local < 0) {   // the id word of the pixel's own ray; nothing is shaded
                id0 = id_word(R);
                centre_hit = R.hit;
                if (STATS && Q.steps) Q.steps[pixel_slot] = R.iters;
                continue;
            }
            V3 light{0.f, 0.f, 0.f};
            bool lit, wants = false;
            V3 so, sd, term;   // a sun ray's record (thr is 1: before the hit)
            if constexpr (SUNLIT) wants = sun_ray_of_hit(Q, *SQ, s.liquid, R.hit, R, st.thr, so, sd, term);
            uint32_t lobes;
            if constexpr (SUNLIT) lobes = SQ->lobes;
            else lobes = LQ.lobes;
            const bool alive = path_after_march_lobes<false>(Q, lobes, st, R, light, lit) && !Q.last_bounce;
            if (MULTI) {
                st.slot += (uint32_t)s_local * Q.acc_slots;
                Q.acc[st.slot] = make_uint4(__float_as_uint(light.x), __float_as_uint(light.y), __float_as_uint(light.z), sample == 0u ? id0 : 0u);
            } else if (Q.sample == 0u) {
                Q.out[st.slot] = make_uint4(__float_as_uint(light.x), __float_as_uint(light.y), __float_as_uint(light.z), id0);
            } else if (lit) {
                add_light(Q.out, st.slot, light);
            }
            append_paths(Q, alive, st, lane);
            if constexpr (SUNLIT) append_light_rays(*SQ, wants, st.slot, so, sd, term, 0u, 0u, lane);
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

}  // namespace vrt

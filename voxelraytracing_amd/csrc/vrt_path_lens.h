// vrt_path_lens.h — bounce 0 of a path frame with camera sampling (vrt_set_camera_sampling, include/vrt.h), for vrt_path.hip,
// included there twice: as path_lens_primary_kernel and, with VRT_LENS_SUN defined, as path_lens_sun_primary_kernel (the frames
// of a context with vrt_set_sun_light as well: a SunLaunch behind the LensLaunch, a sun ray's record from each sample's own hit).
// Kernels of their own, as the sun-lit ones are: every kernel from before keeps its name and its instruction stream, and a
// context with the setting off launches exactly what it launched.  Whether the frame has an emission term, a coat or a
// pass-through draw is read from the launch (L.lobes, S.lobes: scalar branches), not built as a family per combination.
//
// Every sample builds its own primary ray from four draws of its stream (csrc/both/lens_math.h, the text the host mirror
// compiles too) and marches it as an ordinary segment: its origin is no longer the camera's.  The pixel's own pinhole ray —
// what the id word, vrt_read_steps, the hit count and the denoiser's key come from — is marched by the launch that holds the
// frame's first sample and shaded by nobody.  It is trip -1 of the sample loop (P.sample == 0 is the same for every wave of a
// launch), so the kernel holds ONE inlined march: the centre ray's result is down to its id word before a sample's march
// begins, and nothing of a march is live across the loop's back edge but the counts of a stats frame.
// In: VRT_LENS_KERNEL (the kernel's name).
#ifndef VRT_PATH_LENS_SHARED
#define VRT_PATH_LENS_SHARED   // (both/lens_math.h: included by vrt_path.hip, outside the namespace)

// A sample's own primary ray (steps 1 to 3 of the contract): four draws, both/lens_math.h's two halves, the two normalisations.
// Called by every lane of the wave.  The two IEEE divides and the square root take vrt_march.h's refined forms when every lane's
// operands are in their range (a ballot each; a zero numerator is: +-0 / d is +-0 from either form) — proj_size is the frame's, a
// numerator is a pixel coordinate doubled, u3 is 0 once in 2^32 draws and at least 2^-32 otherwise.
__device__ __forceinline__ void lens_ray(const FrameParams &P, const LensLaunch &L, uint32_t px, uint32_t py, uint32_t &rng, V3 &origin, V3 &dir) {
    const float *proj_size = P.cam.proj_size, *ip = P.cam.inv_proj_mat, *iv = P.cam.inv_view_mat;
    const V3 cam{P.cam_origin[0], P.cam_origin[1], P.cam_origin[2]};
    const float u1 = rng_next(rng), u2 = rng_next(rng), u3 = rng_next(rng), u4 = rng_next(rng);
    auto div = [](float n, float d) {
        if (__ballot(!((n == 0.0f || in_band(n)) && in_band(d))) == 0ull) return div_refined(n, d, rcp_refined(d));
        return n / d;
    };
    const LensV3 w = lens_pixel_dir(px, py, u1, u2, L.pixel_spread, proj_size, ip, iv, div);
    dir = normalize_wave(V3{w.x, w.y, w.z});
    origin = cam;
    if (L.aperture != 0.0f) {   // (the launch's: a scalar branch)
        auto sqrt_of = [](float x) {
            constexpr float kSqrtBandLo = 1.0e-28f;   // (sqrt_banded's range is [2^-96, inf))
            if (__ballot(!(x >= kSqrtBandLo)) == 0ull) return sqrt_banded(x);
            return sqrtf(x);
        };
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

// What follows a sample's primary march: path_after_march with the emission term carried (a table of zeros adds nothing and
// marks nothing lit: the frame of a context without emission is what its plain kernel makes it), and the coat's coin or the
// pass-through draw as the frame has them (L.lobes: the same for every lane)
__device__ __forceinline__ bool path_after_march_lens(const FrameParams &P, const LensLaunch &L, PathState &st, const MarchResult &R, V3 &light, bool &lit) {
    if (L.lobes & kSunLobeTranslucent) return path_after_march<true, false, true>(P, st, R, light, lit);
    if (L.lobes & kSunLobePolish) return path_after_march<true, true, false>(P, st, R, light, lit);
    return path_after_march<true, false, false>(P, st, R, light, lit);
}
#endif

#ifdef VRT_LENS_SUN
#define VRT_LENS_ARGS FrameParams P, LensLaunch L, SunLaunch S
#else
#define VRT_LENS_ARGS FrameParams P, LensLaunch L
#endif

// MULTI: the samples of a launch chain (P.acc, P.chain), each into its own plane; otherwise one sample, straight into `out`
template <int MARCH, bool LDS_ROOTS, bool STATS, bool MULTI = false>
__global__ void __launch_bounds__(256) VRT_LENS_KERNEL(VRT_LENS_ARGS) {
    extern __shared__ uint32_t smem[];
    uint32_t *s_liquid = smem, *s_roots = smem + 24;
    unsigned long long *s_acc = reinterpret_cast<unsigned long long *>(smem + 8);
    if (STATS && threadIdx.x < 8) s_acc[threadIdx.x] = 0ull;
    stage_lds(P, s_roots, s_liquid, LDS_ROOTS);

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t t_local = blockIdx.x * 4u + (threadIdx.x >> 6);
    const bool live = t_local < P.tiles_local;
    if (blockIdx.x == 0 && P.seg_clear) P.seg_clear[threadIdx.x * kSegStride] = 0u;   // kHitSegments == blockDim.x cursors
#ifdef VRT_LENS_SUN
    if (blockIdx.x == 0) S.clear[threadIdx.x * kSegStride] = 0u;
#endif
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
#ifdef VRT_LENS_SUN
            const SunLaunch &SQ = fresh_kernarg<SunLaunch, kLensSunLaunchAt>();
#endif
            const uint32_t sample = Q.sample + (uint32_t)s_local;
            PathState st;
            st.slot = pixel_slot;
            st.thr = V3{1.0f, 1.0f, 1.0f};
            if (s_local < 0) {
                create_ray(Q, (int)px, (int)py, st.origin, st.dir);
                st.rng = 0u;
            } else {
                // seed: vrt_path_primary.h's; the sample's first four draws are its ray's
                st.rng = py * Q.width + px + (Q.sample_base + sample) * (Q.width * Q.height) + Q.seed * 0x9E3779B9u;
                lens_ray(Q, LQ, px, py, st.rng, st.origin, st.dir);
            }
            const MarchResult R = march<MARCH, LDS_ROOTS, STATS>(Q, s_roots, s_liquid, st.origin, st.dir);
            if (STATS) {
                iters += R.iters;
                visits += R.visits;
            }
            if (s_local < 0) {   // the id word of the pixel's own ray, composed as shade() does; nothing is shaded
                id0 = R.voxel & VRT_ID_VOXEL_MASK;
                if (R.hit) id0 |= VRT_ID_HIT;
                if (R.norm.x != 0.0f) id0 |= VRT_ID_NX;
                if (R.norm.y != 0.0f) id0 |= VRT_ID_NY;
                if (R.norm.z != 0.0f) id0 |= VRT_ID_NZ;
                if (R.water_dist != 0.0f) id0 |= VRT_ID_WATER;
                centre_hit = R.hit;
                if (STATS && Q.steps) Q.steps[pixel_slot] = R.iters;
                continue;
            }
            V3 light{0.f, 0.f, 0.f};
            bool lit;
#ifdef VRT_LENS_SUN
            V3 so, sd, term;   // (thr is 1: before the hit)
            const bool sun = sun_ray_of_hit(Q, SQ, s_liquid, R.hit, R, st.thr, so, sd, term);
            const bool alive = path_after_march_sunlit<false>(Q, SQ, st, R, light, lit) && !Q.last_bounce;
#else
            const bool alive = path_after_march_lens(Q, LQ, st, R, light, lit) && !Q.last_bounce;
#endif
            if (MULTI) {
                st.slot += (uint32_t)s_local * Q.acc_slots;
                Q.acc[st.slot] = make_uint4(__float_as_uint(light.x), __float_as_uint(light.y), __float_as_uint(light.z), sample == 0u ? id0 : 0u);
            } else if (Q.sample == 0u) {
                Q.out[st.slot] = make_uint4(__float_as_uint(light.x), __float_as_uint(light.y), __float_as_uint(light.z), id0);
            } else if (lit) {
                uint4 t = Q.out[st.slot];
                t.x = __float_as_uint(__uint_as_float(t.x) + light.x);
                t.y = __float_as_uint(__uint_as_float(t.y) + light.y);
                t.z = __float_as_uint(__uint_as_float(t.z) + light.z);
                Q.out[st.slot] = t;
            }
            append_paths(Q, alive, st, lane);
#ifdef VRT_LENS_SUN
            append_sun_rays(SQ, sun, st.slot, so, sd, term, lane);
#endif
        }
    }
    if (STATS) {
        block_add(s_acc, 0, iters);
        block_add(s_acc, 1, visits);
        block_add(s_acc, 2, centre_hit ? 1ull : 0ull);
        __syncthreads();
        if (threadIdx.x == 0) {
            atomicAdd(&P.counters[kCtrSteps], s_acc[0]);
            atomicAdd(&P.counters[kCtrVisits], s_acc[1]);
            atomicAdd(&P.counters[kCtrPrimarySteps], s_acc[0]);
            atomicAdd(&P.counters[kCtrPrimaryVisits], s_acc[1]);
            atomicAdd(&P.counters[kCtrHits], s_acc[2]);
        }
    }
}
#undef VRT_LENS_ARGS

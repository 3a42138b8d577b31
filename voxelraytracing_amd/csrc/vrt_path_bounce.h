// vrt_path_bounce.h — the lane = path bounce kernel, for vrt_path.hip, included there three times: as path_bounce_kernel
// (VRT_BOUNCE_POLISH 0), as path_polished_bounce_kernel (VRT_BOUNCE_POLISH 1: vrt_write_polish; instantiated with EMIT
// alone) and as path_translucent_bounce_kernel (VRT_BOUNCE_TRANSLUCENT 1: vrt_write_translucency; EMIT alone), for the reasons
// vrt_path_primary.h gives.
// In: VRT_BOUNCE_KERNEL (the kernel's name), VRT_BOUNCE_POLISH, VRT_BOUNCE_TRANSLUCENT (0 or 1).
// A fourth time with VRT_BOUNCE_SUN defined, as path_sunlit_bounce_kernel (vrt_set_sun_light), as vrt_path_primary.h says; a miss
// of these segments takes the sky without the sun's disc.
#ifdef VRT_BOUNCE_SUN
#define VRT_BOUNCE_ARGS FrameParams P, SunLaunch S
#else
#define VRT_BOUNCE_ARGS FrameParams P
#endif

// Bounce b >= 1: lane = one live path of the in buffer.  EMIT: emissive hits add their light too (vrt_write_emission).
template <int MARCH, bool LDS_ROOTS, bool STATS, bool EMIT = false>
__global__ void __launch_bounds__(256) VRT_BOUNCE_KERNEL(VRT_BOUNCE_ARGS) {
#ifndef VRT_BOUNCE_SUN
    constexpr bool POLISH = VRT_BOUNCE_POLISH, TRANSLUCENT = VRT_BOUNCE_TRANSLUCENT;
#endif
    extern __shared__ uint32_t smem[];
    uint32_t *s_liquid = smem, *s_roots = smem + 24;
    unsigned long long *s_acc = reinterpret_cast<unsigned long long *>(smem + 8);
    if (STATS && threadIdx.x < 8) s_acc[threadIdx.x] = 0ull;
    stage_lds(P, s_roots, s_liquid, LDS_ROOTS);

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t seg = blockIdx.x % kHitSegments, part = blockIdx.x / kHitSegments;
    if (blockIdx.x == 0 && P.seg_clear) P.seg_clear[threadIdx.x * kSegStride] = 0u;
#ifdef VRT_BOUNCE_SUN
    if (blockIdx.x == 0) S.clear[threadIdx.x * kSegStride] = 0u;
    bool sun = false;
    V3 so{0.f, 0.f, 0.f}, sd{0.f, 0.f, 0.f}, term{0.f, 0.f, 0.f};
#endif
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
        const uint32_t i = seg * P.hit_seg_cap + j;
        const uint4 a = P.path_in[i], b = P.path_in[P.path_cap + i], c = P.path_in[2u * P.path_cap + i];
        st.slot = a.x;
        st.origin = V3{__uint_as_float(a.y), __uint_as_float(a.z), __uint_as_float(a.w)};
        st.dir = V3{__uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z)};
        st.rng = b.w;
        st.thr = V3{__uint_as_float(c.x), __uint_as_float(c.y), __uint_as_float(c.z)};
        V3 light{0.f, 0.f, 0.f};
        bool lit;
#ifdef VRT_BOUNCE_SUN
        R = march<MARCH, LDS_ROOTS, STATS>(P, s_roots, s_liquid, st.origin, st.dir);
        sun = sun_ray_of_hit(P, S, s_liquid, R.hit, R, st.thr, so, sd, term);   // (thr: before the hit)
        alive = path_after_march_sunlit<true>(P, S, st, R, light, lit) && !P.last_bounce;
#else
        alive = path_segment<MARCH, LDS_ROOTS, STATS, EMIT, POLISH, TRANSLUCENT>(P, s_roots, s_liquid, st, R, light, lit) && !P.last_bounce;
#endif
        if (lit) {
            uint4 t = P.out[st.slot];
            t.x = __float_as_uint(__uint_as_float(t.x) + light.x);
            t.y = __float_as_uint(__uint_as_float(t.y) + light.y);
            t.z = __float_as_uint(__uint_as_float(t.z) + light.z);
            P.out[st.slot] = t;
        }
        if (STATS && P.steps && P.sample == 0u) P.steps[st.slot] += R.iters << 16;
    }
    append_paths(P, alive, st, lane);
#ifdef VRT_BOUNCE_SUN
    append_sun_rays(S, sun, st.slot, so, sd, term, lane);
#endif
    if (STATS) {
        block_add(s_acc, 0, active ? R.iters : 0u);
        block_add(s_acc, 1, active ? R.visits : 0u);
        block_add(s_acc, 2, active ? 1ull : 0ull);
        __syncthreads();
        if (threadIdx.x == 0 && s_acc[2]) {
            atomicAdd(&P.counters[kCtrSteps], s_acc[0]);
            atomicAdd(&P.counters[kCtrVisits], s_acc[1]);
            atomicAdd(&P.counters[kCtrSecondary], s_acc[2]);
        }
    }
}
#undef VRT_BOUNCE_ARGS

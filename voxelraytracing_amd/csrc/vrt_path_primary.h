// vrt_path_primary.h — bounce 0 of the path trace, for vrt_path.hip, included there three times: as path_primary_kernel
// (VRT_PRIMARY_POLISH 0), as path_polished_primary_kernel (VRT_PRIMARY_POLISH 1: the frames of a context with a coat,
// vrt_write_polish; instantiated with EMIT alone) and as path_translucent_primary_kernel (VRT_PRIMARY_TRANSLUCENT 1: the frames of
// a context that lets paths through, vrt_write_translucency; EMIT alone again, the coat's draw under a word on the device).  A kernel of its own rather than one more template argument, as the pool
// kernel's body has it (vrt_path_cells.h): the plain and the emissive kernels keep their names and their instruction streams.
// In: VRT_PRIMARY_KERNEL (the kernel's name), VRT_PRIMARY_POLISH, VRT_PRIMARY_TRANSLUCENT (0 or 1).
// A fourth time with VRT_PRIMARY_SUN defined, as path_sunlit_primary_kernel (vrt_set_sun_light, vrt_path_sun.h): the kernel takes a
// SunLaunch behind FrameParams, every hit that sees the sun appends a sun ray's record, and whether there is a coat or a
// pass-through draw is read from the launch (the other two macros are then not read).  Instantiated with EMIT alone, never MULTI.
#ifdef VRT_PRIMARY_SUN
#define VRT_PRIMARY_ARGS FrameParams P, SunLaunch S
#else
#define VRT_PRIMARY_ARGS FrameParams P
#endif

// Bounce 0: primary rays of sample P.sample. Sample 0 initialises the texel {light, id}; later samples add.
// MULTI: the samples of a launch chain (P.acc, P.chain) share the primary march; otherwise one sample, straight into `out`
// EMIT: emissive hits add their light too (vrt_write_emission) — a later sample's texel is then written on those as well
template <int MARCH, bool LDS_ROOTS, bool STATS, bool MULTI = false, bool EMIT = false>
__global__ void __launch_bounds__(256) VRT_PRIMARY_KERNEL(VRT_PRIMARY_ARGS) {
#ifndef VRT_PRIMARY_SUN
    constexpr bool POLISH = VRT_PRIMARY_POLISH, TRANSLUCENT = VRT_PRIMARY_TRANSLUCENT;
#endif
    extern __shared__ uint32_t smem[];
    uint32_t *s_liquid = smem, *s_roots = smem + 24;
    unsigned long long *s_acc = reinterpret_cast<unsigned long long *>(smem + 8);
    if (STATS && threadIdx.x < 8) s_acc[threadIdx.x] = 0ull;
    stage_lds(P, s_roots, s_liquid, LDS_ROOTS);

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t t_local = blockIdx.x * 4u + (threadIdx.x >> 6);
    const bool live = t_local < P.tiles_local;
    if (blockIdx.x == 0 && P.seg_clear) P.seg_clear[threadIdx.x * kSegStride] = 0u;   // kHitSegments == blockDim.x cursors
#ifdef VRT_PRIMARY_SUN
    if (blockIdx.x == 0) S.clear[threadIdx.x * kSegStride] = 0u;
#endif
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
        R = march<MARCH, LDS_ROOTS, STATS, true>(P, s_roots, s_liquid, origin, dir);
        uint32_t id0 = R.voxel & VRT_ID_VOXEL_MASK;   // the id word of the primary segment, composed as shade() does
        if (R.hit) id0 |= VRT_ID_HIT;
        if (R.norm.x != 0.0f) id0 |= VRT_ID_NX;
        if (R.norm.y != 0.0f) id0 |= VRT_ID_NY;
        if (R.norm.z != 0.0f) id0 |= VRT_ID_NZ;
        if (R.water_dist != 0.0f) id0 |= VRT_ID_WATER;
        for (uint32_t s_local = 0; s_local < (MULTI ? P.chain : 1u); s_local++) {
            const uint32_t sample = P.sample + s_local;
            PathState st;
            st.slot = pixel_slot;
            st.origin = origin;
            st.dir = dir;
            st.thr = V3{1.0f, 1.0f, 1.0f};
            // seed: path_tracer.wgsl:328 (y*W + x) + the per-sample stride and frame seed of SURVEY §8d; an accumulating frame's
            // samples continue the accumulation's (P.sample_base: 0 otherwise)
            st.rng = py * P.width + px + (P.sample_base + sample) * (P.width * P.height) + P.seed * 0x9E3779B9u;
            V3 light{0.f, 0.f, 0.f};
            bool lit;
#ifdef VRT_PRIMARY_SUN
            V3 so, sd, term;   // (thr is 1: before the hit)
            const bool sun = sun_ray_of_hit(P, S, s_liquid, R.hit, R, st.thr, so, sd, term);
            const bool alive = path_after_march_sunlit<false>(P, S, st, R, light, lit) && !P.last_bounce;
#else
            const bool alive = path_after_march<EMIT, POLISH, TRANSLUCENT>(P, st, R, light, lit) && !P.last_bounce;
#endif
            if (MULTI) {
                // this sample's own plane: its light so far and, for the frame's first sample, the id word (0 otherwise);
                // the path's later segments find the plane through the slot
                st.slot += s_local * P.acc_slots;
                P.acc[st.slot] = make_uint4(__float_as_uint(light.x), __float_as_uint(light.y), __float_as_uint(light.z), sample == 0u ? id0 : 0u);
            } else if (P.sample == 0u) {
                P.out[st.slot] = make_uint4(__float_as_uint(light.x), __float_as_uint(light.y), __float_as_uint(light.z), id0);
            } else if (lit) {
                uint4 t = P.out[st.slot];
                t.x = __float_as_uint(__uint_as_float(t.x) + light.x);
                t.y = __float_as_uint(__uint_as_float(t.y) + light.y);
                t.z = __float_as_uint(__uint_as_float(t.z) + light.z);
                P.out[st.slot] = t;
            }
            append_paths(P, alive, st, lane);
#ifdef VRT_PRIMARY_SUN
            append_sun_rays(S, sun, st.slot, so, sd, term, lane);
#endif
        }
        if (STATS && P.steps && P.sample == 0u) P.steps[pixel_slot] = R.iters;
    }
    if (STATS) {
        block_add(s_acc, 0, R.iters);
        block_add(s_acc, 1, R.visits);
        block_add(s_acc, 2, (R.hit && P.sample == 0u) ? 1ull : 0ull);
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
#undef VRT_PRIMARY_ARGS

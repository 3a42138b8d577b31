// vrt_path_bounce.h — the lane = path bounce kernel, for vrt_path.hip: path_bounce_kernel, one template for the same five forms as
// vrt_path_primary.h's (plain, EMIT, POLISH, TRANSLUCENT, SUN); a miss of a sun-lit frame's later segments takes the sky without
// the sun's disc.
#pragma once

#include "vrt_path_common.h"
#include "vrt_path_sun.h"

namespace vrt {

// One segment of a path: its march, then path_after_march.  (A function between the kernel and the two: called from the kernel's
// body, the grid march's compiled code comes out two instructions apart — docs/KERNELS.md, one template per family.)
template <int MARCH, bool LDS_ROOTS, bool STATS, bool EMIT, bool POLISH, bool TRANSLUCENT>
__device__ __forceinline__ bool path_segment(const FrameParams &P, const uint32_t *s_roots, const uint32_t *s_liquid,
                                             PathState &st, MarchResult &R, V3 &light, bool &lit) {
    R = march<MARCH, LDS_ROOTS, STATS>(P, s_roots, s_liquid, st.origin, st.dir);
    return path_after_march<EMIT, POLISH, TRANSLUCENT>(P, st, R, light, lit);
}

// Bounce b >= 1: lane = one live path of the in buffer.  EMIT: emissive hits add their light too (vrt_write_emission).
template <int MARCH, bool LDS_ROOTS, bool STATS, bool EMIT = false, bool POLISH = false, bool TRANSLUCENT = false, class... SUN>
__global__ void __launch_bounds__(256) path_bounce_kernel(FrameParams P, SUN... sun) {
    constexpr bool SUNLIT = sizeof...(SUN) != 0;
    const PathLds s = path_lds<STATS>();
    stage_lds(P, s.roots, s.liquid, LDS_ROOTS);

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t seg = blockIdx.x % kHitSegments, part = blockIdx.x / kHitSegments;
    if (blockIdx.x == 0 && P.seg_clear) P.seg_clear[threadIdx.x * kSegStride] = 0u;
    if constexpr (SUNLIT) {
        if (blockIdx.x == 0) sun_launch(sun...).clear[threadIdx.x * kSegStride] = 0u;
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
        V3 light{0.f, 0.f, 0.f};
        bool lit;
        if constexpr (SUNLIT) {
            const SunLaunch &S = sun_launch(sun...);
            R = march<MARCH, LDS_ROOTS, STATS>(P, s.roots, s.liquid, st.origin, st.dir);
            wants = sun_ray_of_hit(P, S, s.liquid, R.hit, R, st.thr, so, sd, term);   // (thr: before the hit)
            alive = path_after_march_lobes<true>(P, S.lobes, st, R, light, lit) && !P.last_bounce;
        } else {
            alive = path_segment<MARCH, LDS_ROOTS, STATS, EMIT, POLISH, TRANSLUCENT>(P, s.roots, s.liquid, st, R, light, lit) && !P.last_bounce;
        }
        if (lit) add_light(P.out, st.slot, light);
        if (STATS && P.steps && P.sample == 0u) P.steps[st.slot] += R.iters << 16;
    }
    append_paths(P, alive, st, lane);
    if constexpr (SUNLIT) append_light_rays(sun_launch(sun...), wants, st.slot, so, sd, term, 0u, 0u, lane);
    if (STATS) secondary_stats(P, s.acc, active, R);
}

}  // namespace vrt

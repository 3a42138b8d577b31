// vrt_path_sun.h — direct sunlight for the path trace (vrt_set_sun_light, include/vrt.h), for vrt_path.hip: what the kernels
// of a sun-lit frame share.  Every hit on a solid voxel whose face looks at the sun appends a record — its texel's slot, the
// shadow ray's origin and direction (shadow_kernel's: the bounce origin, towards P.sun_local) and the term (mc * (k * c)) * thr —
// to a compacted buffer of the frame set's own, segmented and appended to as the path buffers are (append_light_rays); a launch of
// its own right behind each trace launch marches the records and adds the term of the unoccluded ones to the slot's texel.
// Stream order puts the term behind the segment's emission term and ahead of the next segment's; one record per slot per launch
// keeps the plain read-modify-write free of races.
//
// The march of a plain frame over the march cells (sun_occluded_cells) asks one thing of a step: may the ray pass this voxel?
// That is bit u of the cell's last two words, so a step is one 16-byte load — no brick, no normal, no voxel id — and the step
// arithmetic is vrt_path_cells.h's take_step, operation for operation (a position one ulp off eventually meets another voxel).
// Sun rays are finite (a direction that is not gives c > 0 false: no ray), so the general step of a NaN camera has no
// counterpart here.  Plain HIP: the loop has no hand-written instruction.
#pragma once

#include "vrt_path_common.h"

namespace vrt {

// Step 2 of vrt_set_sun_light's contract for one hit.  Called by every lane of the wave (normalize_wave chooses per wave);
// true: this lane sends a sun ray.  thr: the throughput before the hit.
__device__ __forceinline__ bool sun_ray_of_hit(const FrameParams &P, const SunLaunch &S, const uint32_t *s_liquid, bool hit, const MarchResult &R,
                                               const V3 &thr, V3 &so, V3 &sd, V3 &term) {
    const bool solid = hit && R.voxel != 0u && !is_liquid(s_liquid, R.voxel);
    so = V3{R.pos.x + R.norm.x * kShadowBias, R.pos.y + R.norm.y * kShadowBias, R.pos.z + R.norm.z * kShadowBias};
    sd = normalize_wave(V3{P.sun_local[0] - so.x, P.sun_local[1] - so.y, P.sun_local[2] - so.z});
    const float c = vdot(R.norm, sd);
    const V3 mc = hit_color(P, R);
    const float w = S.k * c;
    term = V3{(mc.x * w) * thr.x, (mc.y * w) * thr.y, (mc.z * w) * thr.z};
    return solid && c > 0.0f;   // (a zero normal or a NaN: no ray)
}

// the SunLaunch of a kernel built with one: the trailing argument pack (nothing, or SunLaunch) of the templates that have a sun-lit form
__device__ __forceinline__ const SunLaunch &sun_launch(const SunLaunch &S) { return S; }

// Is the ray from `origin` along `dir` (finite both) stopped before it leaves the world?  ray_world's answer — its hit flag — over the
// march cells: liquids are passed (the cells' "passes" bits are built with the material table's liquid set), running out of the
// 500 lookups counts as stopped, a ray that starts outside the world is not.
template <bool DIRECT>
__device__ __forceinline__ bool sun_occluded_cells(const FrameParams &P, V3 origin, V3 dir) {
    const TableBuf mb = table_buffer(P.mblk, P.mblk_bytes), db = table_buffer(P.cdir, P.cdir_bytes);
    // the chunk directory: [S][S+1][S+1] with a zero border; a direct world: [4S][4S+1][4S+1] lines of 128 bytes
    const uint32_t drow = (P.grid_dim / 8u + 1u) * 4u, dslab = (P.grid_dim / 8u + 1u) * drow;
    const uint32_t row128 = (P.grid_dim / 2u + 1u) * 128u, slab128 = (P.grid_dim / 2u + 1u) * row128;
    const float world_max = P.world_max;
    const V3 unit = unit_steps(dir);
    const float ux = unit.x, uy = unit.y, uz = unit.z;
    constexpr uint32_t kTwo23 = 0x4B000000u;
    const uint32_t mxm = kTwo23 | (dir.x >= 0.0f ? 0x007FFFFFu : 0u), mym = kTwo23 | (dir.y >= 0.0f ? 0x007FFFFFu : 0u),
                   mzm = kTwo23 | (dir.z >= 0.0f ? 0x007FFFFFu : 0u);
    const float cx = dir.x >= 0.0f ? -8388607.0f : -8388608.0f, cy = dir.y >= 0.0f ? -8388607.0f : -8388608.0f,
                cz = dir.z >= 0.0f ? -8388607.0f : -8388608.0f;
    V3 pos = nudged(origin, dir);
    if ((pos.x <= 0.0f || pos.y <= 0.0f || pos.z <= 0.0f) || (pos.x >= world_max || pos.y >= world_max || pos.z >= world_max)) return false;
    int vx = trunc2i(pos.x), vy = trunc2i(pos.y), vz = trunc2i(pos.z);
    for (uint32_t iter = 0u; iter < kMaxSteps; iter++) {
        const uint32_t sub = ((((uint32_t)vz >> 2) & 1u) << 2) | ((((uint32_t)vy >> 2) & 1u) << 1) | (((uint32_t)vx >> 2) & 1u);
        uint32_t off;
        if (DIRECT) {
            off = mad_i24(vz >> 3, slab128, mad_i24(vy >> 3, row128, ((uint32_t)(vx >> 3) << 7) + (sub << 4)));
        } else {   // (a position outside the world finds the border's zero, block 0: cells of zeros)
            const uint32_t block = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(db, mad_i24(vz >> 5, dslab, mad_i24(vy >> 5, drow, (uint32_t)(vx >> 5) << 2)), 0, 0) << 13;
            const uint32_t line = ((((((uint32_t)vz >> 3) & 3u) << 2) | (((uint32_t)vy >> 3) & 3u)) << 2) | (((uint32_t)vx >> 3) & 3u);
            off = block + (((line << 3) | sub) << 4);
        }
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        const u32x4 cell = __builtin_amdgcn_raw_buffer_load_b128(mb, off, 0, 0);   // the step's one load
        const uint32_t u = ((uint32_t)vx & 3u) | (((uint32_t)vy & 3u) << 2) | (((uint32_t)vz & 3u) << 4);
        const unsigned long long passes = ((unsigned long long)cell.w << 32) | cell.z;
        if (!((passes >> u) & 1ull)) return cell.x != 0u;   // a solid voxel — or, the entry 0, a position outside the world
        // the leaf's size - 1: a leaf cell's lo, or the size-2 bit of a split cell's voxel (vrt_path_cells.h: take_step)
        const uint32_t sel = kAirLeaf | (cell.x & 31u) | ((cell.y >> ((u >> 1) & 31u)) & 1u);
        const float tx = (__uint_as_float(bfi(sel, mxm, (uint32_t)vx)) + cx) - pos.x;
        const float ty = (__uint_as_float(bfi(sel, mym, (uint32_t)vy)) + cy) - pos.y;
        const float tz = (__uint_as_float(bfi(sel, mzm, (uint32_t)vz)) + cz) - pos.z;
        const float adx = abs_mul(tx, ux), ady = abs_mul(ty, uy), adz = abs_mul(tz, uz);
        float step = min3_f32(adx, ady, adz);
        if (__ballot(!(step > 0.0f)) != 0ull)
            step = __uint_as_float(min3_u32(__float_as_uint(adx) - 1u, __float_as_uint(ady) - 1u, __float_as_uint(adz) - 1u) + 1u);
        const float sp = step + 0.001f;
        pos.x += dir.x * (step == adx ? sp : step);
        pos.y += dir.y * (step == ady ? sp : step);
        pos.z += dir.z * (step == adz ? sp : step);
        vx = flr2i(pos.x);
        vy = flr2i(pos.y);
        vz = flr2i(pos.z);
    }
    return true;   // out of lookups: stopped
}

// a record of the sun buffer, read back by the lane that marches it
struct SunRecord {
    uint32_t slot;
    V3 so, sd, term;
};
__device__ __forceinline__ SunRecord load_sun_record(const SunLaunch &S, uint32_t i) {
    const uint4 a = S.recs[i], b = S.recs[S.cap + i], c = S.recs[2u * S.cap + i];
    return SunRecord{a.x, V3{__uint_as_float(a.y), __uint_as_float(a.z), __uint_as_float(a.w)},
                     V3{__uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z)},
                     V3{__uint_as_float(c.x), __uint_as_float(c.y), __uint_as_float(c.z)}};
}

// The sun launch of a plain frame over the march cells: lane = one record of the trace launch in front of it.
template <bool DIRECT>
__global__ void __launch_bounds__(256) path_sun_cells_kernel(FrameParams P, SunLaunch S) {
    const uint32_t seg = blockIdx.x % kHitSegments, part = blockIdx.x / kHitSegments;
    const uint32_t count = min(S.counts[seg * kSegStride], S.seg_cap);
    const uint32_t j = part * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const SunRecord r = load_sun_record(S, seg * S.seg_cap + j);
    if (!sun_occluded_cells<DIRECT>(P, r.so, r.sd)) add_light(P.out, r.slot, r.term);
}

// ... of every other frame (stats, the literal march, worlds without march cells): the records marched by march<> — which also
// counts: a stats frame's steps and node visits include the sun marches, its secondary rays the sun rays.  vrt_read_steps'
// per-pixel counts stay the path segments'.
template <int MARCH, bool LDS_ROOTS, bool STATS>
__global__ void __launch_bounds__(256) path_sun_kernel(FrameParams P, SunLaunch S) {
    const PathLds s = path_lds<STATS>();
    stage_lds(P, s.roots, s.liquid, LDS_ROOTS);
    const uint32_t seg = blockIdx.x % kHitSegments, part = blockIdx.x / kHitSegments;
    const uint32_t count = min(S.counts[seg * kSegStride], S.seg_cap);
    const uint32_t j = part * blockDim.x + threadIdx.x;
    const bool active = j < count;
    if (!STATS && part * blockDim.x >= count) return;
    MarchResult R;
    R.iters = 0; R.visits = 0; R.hit = false;
    if (active) {
        const SunRecord r = load_sun_record(S, seg * S.seg_cap + j);
        R = march<MARCH, LDS_ROOTS, STATS>(P, s.roots, s.liquid, r.so, r.sd);
        if (!R.hit) add_light(P.out, r.slot, r.term);
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

// vrt_path_common.h — what the path trace's kernels share (vrt_path.hip: the primary launch, the lane = path bounce kernels
// and the pool kernel over the march cells; vrt_kernels.hip's self-test of the exact math): the RNG of path_tracer.wgsl:56-72, log and cos spelled out in + - * / (host and device agree to the bit), and what follows a
// segment's march (path_tracer.wgsl:155-192).  DESIGN.md, path trace.
#pragma once

#include "vrt_march.h"

namespace vrt {

// rng_next, path_tracer.wgsl:56-61
__device__ __forceinline__ float rng_next(uint32_t &state) {
    state = state * 747796405u + 2891336453u;
    uint32_t r = ((state >> ((state >> 28u) + 4u)) ^ state) * 277803737u;
    r = (r >> 22u) ^ r;
    return (float)r / 4294967295.0f;
}

// ln(x), x normal > 0: x = m * 2^e with m in (sqrt(1/2), sqrt(2)], ln m = 2 atanh((m-1)/(m+1))
// BANDED: the one division without the general sequence's scaffolding (vrt_march.h: rcp_refined / div_in_band).  Its operands are
// always inside what that needs: m + 1 in [1.70, 2.42]; m - 1 is zero — +0 / d is +0 from either form — or of magnitude >= 2^-24
// (m is a binary32 in (0.707, 1.4143]).  So there is no choice to make per wave: 8 instructions for 11, 25 issue cycles for 40.
// vrt_selftest_exact_math runs both forms over every mantissa.
template <bool BANDED>
__device__ __forceinline__ float vlog_t(float x) {
    const uint32_t b = __float_as_uint(x);
    int e = (int)(b >> 23) - 127;
    float m = __uint_as_float((b & 0x007FFFFFu) | 0x3F800000u);
    if (m > 1.41421354f) { m = m * 0.5f; e += 1; }
    const float num = m - 1.0f, den = m + 1.0f;
    const float s = BANDED ? div_in_band(num, den, rcp_refined(den)) : num / den;
    const float z = s * s;
    const float p = z * (0.333333343f + z * (0.2f + z * (0.142857149f + z * (0.111111112f + z * 0.0909090936f))));
    return (float)e * 0.693147182f + (s + s * p) * 2.0f;
}
__device__ __forceinline__ float vlog(float x) { return vlog_t<true>(x); }

// cos(2*pi*u), u in [0,1]
__device__ __forceinline__ float vcos2pi(float u) {
    const float t = u * 4.0f;
    const float q = floorf(t);
    const float a = (t - q) * 1.57079637f;
    const float a2 = a * a;
    const float sn = a * (1.0f + a2 * (-0.166666672f + a2 * (0.00833333377f + a2 * (-0.000198412701f + a2 * (2.75573188e-06f + a2 * -2.50521079e-08f)))));
    const float cs = 1.0f + a2 * (-0.5f + a2 * (0.0416666679f + a2 * (-0.00138888892f + a2 * (2.48015876e-05f + a2 * (-2.75573199e-07f + a2 * 2.08767559e-09f)))));
    const int qi = (int)q & 3;
    return qi == 0 ? cs : (qi == 1 ? -sn : (qi == 2 ? -cs : sn));
}

// rng_next_norm / rng_next_dir, path_tracer.wgsl:62-72: three normal deviates rho * cos(2 pi u1), rho = sqrt(-2 ln u2), drawn in
// the shader's order (u1, u2 of x, then of y, then of z), and their direction.  The three square roots take vrt_march.h's banded
// form — v_sqrt_f32 and one ulp either way — when every lane's three arguments are in its range (one ballot for the three): an
// argument is -0 when u2 rounds to 1 (a draw in 2^25), else >= 1.19e-7.  Same operations on the same values as the texts below.
__device__ __forceinline__ float rng_next_u2(uint32_t &state) {
    const float u2 = rng_next(state);
    return u2 < 1.0e-10f ? 1.0e-10f : u2;
}
// what a wave's square-root arguments must all reach to take sqrt_banded (its range is [2^-96, inf); !(x >= this) also sends
// -0 and NaN to sqrtf): rng_next_dir below and lens_sqrt_of
constexpr float kSqrtBandLo = 1.0e-28f;
__device__ __forceinline__ V3 rng_next_dir(uint32_t &state) {
    const float u1x = rng_next(state), tx = -2.0f * vlog(rng_next_u2(state));
    const float u1y = rng_next(state), ty = -2.0f * vlog(rng_next_u2(state));
    const float u1z = rng_next(state), tz = -2.0f * vlog(rng_next_u2(state));
    float rx, ry, rz;   // (the arguments are <= 46.1)
    if (__ballot(!(min3_f32(tx, ty, tz) >= kSqrtBandLo)) == 0ull) {
        rx = sqrt_banded(tx); ry = sqrt_banded(ty); rz = sqrt_banded(tz);
    } else {
        rx = sqrtf(tx); ry = sqrtf(ty); rz = sqrtf(tz);
    }
    return normalize_wave(V3{rx * vcos2pi(u1x), ry * vcos2pi(u1y), rz * vcos2pi(u1z)});
}

// The IEEE divide and square root of a lens sample's ray (vrt_path_lens.h: lens_ray hands them to both/lens_math.h) in vrt_march.h's
// refined forms when every lane's operands are in their range — a ballot each; a zero numerator is: +-0 / d is +-0 from either form
// (div_refined's fix-up: vrt_march.h).
// Named, not lambdas of lens_ray, so that vrt_selftest_math_values calls the same text.
__device__ __forceinline__ float lens_div(float n, float d) {
    if (__ballot(!((n == 0.0f || in_band(n)) && in_band(d))) == 0ull) return div_refined(n, d, rcp_refined(d));
    return n / d;
}
__device__ __forceinline__ float lens_sqrt_of(float x) {
    if (__ballot(!(x >= kSqrtBandLo)) == 0ull) return sqrt_banded(x);
    return sqrtf(x);
}

// The material colour of a hit after face shading (ray_tracer.wgsl:296-314) — shade()'s first half.
__device__ __forceinline__ V3 hit_color(const FrameParams &P, const MarchResult &R) {
    const vrt_material *m = &P.mats[min(R.voxel, 255u)];
    V3 mc{m->color[0], m->color[1], m->color[2]};
    if (R.norm.x != 0.0f) { mc.x *= 0.5f; mc.y *= 0.5f; mc.z *= 0.5f; }
    if (R.norm.z != 0.0f) { mc.x *= 0.7f; mc.y *= 0.7f; mc.z *= 0.7f; }
    if (R.norm.y == -1.0f) { mc.x *= 0.2f; mc.y *= 0.2f; mc.z *= 0.2f; }
    if (P.settings.show_step_count == 1u) {
        const float f = vclamp((float)R.iters / 500.0f, 0.0f, 1.0f);
        mc = V3{f, f, f};
    }
    return mc;
}

struct PathState {
    uint32_t slot;
    V3 origin, dir, thr;
    uint32_t rng;
};

// The light a hit gives off (path_tracer.wgsl:183-184, vrt_write_emission): (mc * e) * thr per channel, thr the throughput
// before the hit, e the voxel's entry of the emission table.  false (and `light` untouched) when e is 0: nothing is added.
__device__ __forceinline__ bool path_emission(const FrameParams &P, const MarchResult &R, const V3 &mc, const V3 &thr, V3 &light) {
    const float e = emission_table(P.mats)[min(R.voxel, 255u)];
    if (e == 0.0f) return false;
    light = V3{(mc.x * e) * thr.x, (mc.y * e) * thr.y, (mc.z * e) * thr.z};
    return true;
}

// A hit of a translucent frame (vrt_write_translucency, include/vrt.h: steps 3 to 6 there; the TRANSLUCENT builds of the
// path kernels).  ut is drawn on every hit, ahead of everything else; a lane whose ut is below its entry's chance passes: it keeps
// dir, crosses the unit voxel that holds the hit position, multiplies thr by the entry's colour and draws nothing more.  Every
// other lane runs the body of path_after_march below — the coat's draw under the word behind the tables (the same for every
// lane: a scalar branch), so that this family exists once, polished or not.  The RNG state, origin, dir and tint are selected per
// lane; the bounce's draws (three logs, three square roots, three cosines) are branched around only where the whole wave passes.
__device__ __forceinline__ void path_translucent_hit(const FrameParams &P, PathState &st, const MarchResult &R, const V3 &mc) {
    const uint32_t entry = min(R.voxel, 255u);
    const float4 tc = *reinterpret_cast<const float4 *>(&translucency_table(P.mats)[entry]);   // color + chance: one load
    const float ut = rng_next(st.rng);
    const bool passes = ut < tc.w;
    uint32_t rng = st.rng;
    V3 origin = R.pos, dir = st.dir, tint{tc.x, tc.y, tc.z};
    if (__ballot(!passes) != 0ull) {
        const bool coat = __builtin_amdgcn_readfirstlane(*coat_word(P.mats)) != 0u;
        const float d = vdot(R.norm, st.dir);
        const V3 spec{st.dir.x - 2.0f * R.norm.x * d, st.dir.y - 2.0f * R.norm.y * d, st.dir.z - 2.0f * R.norm.z * d};
        float u = 0.0f;
        if (coat) u = rng_next(rng);
        const V3 rd = rng_next_dir(rng);
        const V3 sc = normalize_wave(V3{R.norm.x + rd.x, R.norm.y + rd.y, R.norm.z + rd.z});
        const vrt_polish *e = &polish_table(P.mats)[entry];
        const float4 cc = *reinterpret_cast<const float4 *>(e);
        const bool polished = coat && u < cc.w;
        const float scatter = polished ? e->scatter : P.mats[entry].scatter;
        const V3 nd = normalize_wave(V3{vmix(spec.x, sc.x, scatter), vmix(spec.y, sc.y, scatter), vmix(spec.z, sc.z, scatter)});
        if (!passes) {
            tint = V3{polished ? cc.x : mc.x, polished ? cc.y : mc.y, polished ? cc.z : mc.z};
            origin = V3{R.pos.x + R.norm.x * kShadowBias, R.pos.y + R.norm.y * kShadowBias, R.pos.z + R.norm.z * kShadowBias};
            dir = nd;
            st.rng = rng;
        }
    }
    // the pass: across the unit voxel of the hit position, in the form the march advances across an air node (compares and selects)
    const float inf = __builtin_inff();
    const float cx = floorf(R.pos.x), cy = floorf(R.pos.y), cz = floorf(R.pos.z);
    const float tx = st.dir.x != 0.0f ? ((st.dir.x > 0.0f ? cx + 1.0f : cx) - R.pos.x) / st.dir.x : inf;
    const float ty = st.dir.y != 0.0f ? ((st.dir.y > 0.0f ? cy + 1.0f : cy) - R.pos.y) / st.dir.y : inf;
    const float tz = st.dir.z != 0.0f ? ((st.dir.z > 0.0f ? cz + 1.0f : cz) - R.pos.z) / st.dir.z : inf;
    float t = tx;
    if (ty < t) t = ty;
    if (tz < t) t = tz;
    const float ts = t + 0.001f;
    if (passes) origin = V3{R.pos.x + st.dir.x * ts, R.pos.y + st.dir.y * ts, R.pos.z + st.dir.z * ts};
    st.thr = V3{st.thr.x * tint.x, st.thr.y * tint.y, st.thr.z * tint.z};
    st.origin = origin;
    st.dir = dir;
}

// What follows a segment's march (the rest of the body of ray_color's loop, path_tracer.wgsl:155-192).  Returns true if the
// path goes on (st updated to the next segment); a miss puts the sky's light, weighted, into `light`, and so does — EMIT — a
// hit on an emissive voxel its own.  lit: `light` holds a term for the sample's texel.
// POLISH (vrt_write_polish; :175, :180, :185): every hit draws u ahead of the direction's six draws, and where u is below the
// chance of the voxel's entry of the polish table, the entry's scatter and colour take the place of the material's scatter and mc.
// TRANSLUCENT (vrt_write_translucency; :167-173): path_translucent_hit above in the place of everything behind the emission term;
// POLISH is then not read (the coat's draw is under the word behind the tables).
// SKY_NO_DISC (vrt_set_sun_light, vrt_path_sun.h): a miss takes the sky without the sun's disc — a later segment of a sun-lit path.
template <bool EMIT = false, bool POLISH = false, bool TRANSLUCENT = false, bool SKY_NO_DISC = false>
__device__ __forceinline__ bool path_after_march(const FrameParams &P, PathState &st, const MarchResult &R, V3 &light, bool &lit) {
    lit = !R.hit;
    if (!R.hit) {
        const V3 sky = ray_sky<false, SKY_NO_DISC>(P, st.origin, st.dir);
        light = V3{sky.x * st.thr.x, sky.y * st.thr.y, sky.z * st.thr.z};
        return false;
    }
    const V3 mc = hit_color(P, R);
    if (EMIT) lit = path_emission(P, R, mc, st.thr, light);   // (before thr *= mc: :183-186)
    if (TRANSLUCENT) {
        path_translucent_hit(P, st, R, mc);
        return true;
    }
    const float d = vdot(R.norm, st.dir);
    const V3 spec{st.dir.x - 2.0f * R.norm.x * d, st.dir.y - 2.0f * R.norm.y * d, st.dir.z - 2.0f * R.norm.z * d};
    float u = 0.0f;
    if (POLISH) u = rng_next(st.rng);
    const V3 rd = rng_next_dir(st.rng);
    const V3 sc = normalize_wave(V3{R.norm.x + rd.x, R.norm.y + rd.y, R.norm.z + rd.z});
    float scatter = P.mats[min(R.voxel, 255u)].scatter;
    V3 tint = mc;
    if (POLISH) {   // (selects, behind the draws: only u is kept across them)
        const vrt_polish *e = &polish_table(P.mats)[min(R.voxel, 255u)];
        const float4 cc = *reinterpret_cast<const float4 *>(e);   // color + chance: one load
        const bool polished = u < cc.w;
        scatter = polished ? e->scatter : scatter;
        tint = V3{polished ? cc.x : mc.x, polished ? cc.y : mc.y, polished ? cc.z : mc.z};
    }
    const V3 nd = normalize_wave(V3{vmix(spec.x, sc.x, scatter), vmix(spec.y, sc.y, scatter), vmix(spec.z, sc.z, scatter)});
    st.thr = V3{st.thr.x * tint.x, st.thr.y * tint.y, st.thr.z * tint.z};
    st.origin = V3{R.pos.x + R.norm.x * kShadowBias, R.pos.y + R.norm.y * kShadowBias, R.pos.z + R.norm.z * kShadowBias};
    st.dir = nd;
    return true;
}

// path_after_march of a frame whose kernels read coat and pass-through from the launch (`lobes`: kSunLobePolish | kSunLobeTranslucent,
// the same for every lane — a scalar branch; one kernel, not one per combination), the emission term always carried: a table of
// zeros adds nothing and marks nothing lit
template <bool SKY_NO_DISC = false>
__device__ __forceinline__ bool path_after_march_lobes(const FrameParams &P, uint32_t lobes, PathState &st, const MarchResult &R, V3 &light, bool &lit) {
    if (lobes & kSunLobeTranslucent) return path_after_march<true, false, true, SKY_NO_DISC>(P, st, R, light, lit);
    if (lobes & kSunLobePolish) return path_after_march<true, true, false, SKY_NO_DISC>(P, st, R, light, lit);
    return path_after_march<true, false, false, SKY_NO_DISC>(P, st, R, light, lit);
}

// the nudge off a voxel face at the start of a march (ray_tracer.wgsl:204-207)
__device__ __forceinline__ V3 nudged(V3 pos, V3 dir) {
    if (pos.x - floorf(pos.x) < 0.001f || pos.y - floorf(pos.y) < 0.001f || pos.z - floorf(pos.z) < 0.001f) {
        pos.x += 0.001f * dir.x;
        pos.y += 0.001f * dir.y;
        pos.z += 0.001f * dir.z;
    }
    return pos;
}

// how many lanes of the mask are below this one (two instructions over the mask's halves; no per-lane mask to keep)
__device__ __forceinline__ uint32_t lanes_below(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// Append the wave's surviving paths to this workgroup's segment of the out buffer (one atomic per wave).  direct: what the
// record's spare word — the third plane's .w — carries, 1 or 0 (a lamp-lit frame: whether the path is still direct, vrt_path_lamp.h).
__device__ __forceinline__ void append_paths(const FrameParams &P, bool alive, const PathState &st, uint32_t lane, bool direct = false) {
    const unsigned long long ballot = __ballot(alive);
    const uint32_t n = (uint32_t)__popcll(ballot);
    if (!n) return;
    const uint32_t seg = blockIdx.x % kHitSegments;
    const int leader = __ffsll((long long)ballot) - 1;
    uint32_t base = 0;
    if ((int)lane == leader) base = atomicAdd(&P.seg_counts[seg * kSegStride], n);
    base = __shfl(base, leader, 64) + seg * P.hit_seg_cap;
    if (alive) {
        const uint32_t i = base + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
        P.path_out[i] = make_uint4(st.slot, __float_as_uint(st.origin.x), __float_as_uint(st.origin.y), __float_as_uint(st.origin.z));
        P.path_out[P.path_cap + i] = make_uint4(__float_as_uint(st.dir.x), __float_as_uint(st.dir.y), __float_as_uint(st.dir.z), st.rng);
        P.path_out[2u * P.path_cap + i] = make_uint4(__float_as_uint(st.thr.x), __float_as_uint(st.thr.y), __float_as_uint(st.thr.z), direct ? 1u : 0u);
    }
}

// A path record of the in buffer (append_paths wrote it), read back by the lane that marches it; its spare word, for the kernels
// that read it (the third plane is loaded once: the compiler merges the two reads)
__device__ __forceinline__ PathState load_path(const FrameParams &P, uint32_t i) {
    const uint4 a = P.path_in[i], b = P.path_in[P.path_cap + i], c = P.path_in[2u * P.path_cap + i];
    PathState st;
    st.slot = a.x;
    st.origin = V3{__uint_as_float(a.y), __uint_as_float(a.z), __uint_as_float(a.w)};
    st.dir = V3{__uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z)};
    st.rng = b.w;
    st.thr = V3{__uint_as_float(c.x), __uint_as_float(c.y), __uint_as_float(c.z)};
    return st;
}
__device__ __forceinline__ uint32_t path_spare_word(const FrameParams &P, uint32_t i) { return P.path_in[2u * P.path_cap + i].w; }

// Append the wave's rays towards a light to this workgroup's segment of that light's buffer (append_paths' ballot compaction; B: the
// SunLaunch or the LampLaunch, whose recs / counts / cap / seg_cap it is).  w1, w2: the spare words of the direction's and the term's plane.
template <class B>
__device__ __forceinline__ void append_light_rays(const B &buf, bool wants, uint32_t slot, const V3 &so, const V3 &dir, const V3 &term, uint32_t w1,
                                                  uint32_t w2, uint32_t lane) {
    const unsigned long long ballot = __ballot(wants);
    const uint32_t n = (uint32_t)__popcll(ballot);
    if (!n) return;
    const uint32_t seg = blockIdx.x % kHitSegments;
    const int leader = __ffsll((long long)ballot) - 1;
    uint32_t base = 0;
    if ((int)lane == leader) base = atomicAdd(&buf.counts[seg * kSegStride], n);
    base = __shfl(base, leader, 64);
    if (wants) {
        const uint32_t j = base + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
        // (never false: a workgroup appends at most 256 records in a launch, and a segment has seg_cap / 256 producers)
        if (j < buf.seg_cap) {
            const uint32_t i = seg * buf.seg_cap + j;
            buf.recs[i] = make_uint4(slot, __float_as_uint(so.x), __float_as_uint(so.y), __float_as_uint(so.z));
            buf.recs[buf.cap + i] = make_uint4(__float_as_uint(dir.x), __float_as_uint(dir.y), __float_as_uint(dir.z), w1);
            buf.recs[2u * buf.cap + i] = make_uint4(__float_as_uint(term.x), __float_as_uint(term.y), __float_as_uint(term.z), w2);
        }
    }
}

// ---- what the kernels of the lane = path families open and close with ----

// The LDS of a launch (lds_bytes_path, vrt_path.hip): the liquid set, the stats frame's block sums (zeroed here), the root table
// where it fits.  The tables are staged by the kernel itself, behind this: stage_lds(P, s.roots, s.liquid, LDS_ROOTS)
struct PathLds {
    uint32_t *liquid, *roots;
    unsigned long long *acc;
};
template <bool STATS>
__device__ __forceinline__ PathLds path_lds() {
    extern __shared__ uint32_t smem[];
    const PathLds s{smem, smem + 24, reinterpret_cast<unsigned long long *>(smem + 8)};
    if (STATS && threadIdx.x < 8) s.acc[threadIdx.x] = 0ull;
    return s;
}

// the id word of a march result, composed as shade() does
__device__ __forceinline__ uint32_t id_word(const MarchResult R) {
    uint32_t id = R.voxel & VRT_ID_VOXEL_MASK;
    if (R.hit) id |= VRT_ID_HIT;
    if (R.norm.x != 0.0f) id |= VRT_ID_NX;
    if (R.norm.y != 0.0f) id |= VRT_ID_NY;
    if (R.norm.z != 0.0f) id |= VRT_ID_NZ;
    if (R.water_dist != 0.0f) id |= VRT_ID_WATER;
    return id;
}

// A sample's seed: path_tracer.wgsl:328 (y*W + x) + the per-sample stride and frame seed of SURVEY §8d; an accumulating frame's
// samples continue the accumulation's (P.sample_base: 0 otherwise)
__device__ __forceinline__ uint32_t sample_seed(const FrameParams &P, uint32_t px, uint32_t py, uint32_t sample) {
    return py * P.width + px + (P.sample_base + sample) * (P.width * P.height) + P.seed * 0x9E3779B9u;
}

// a light term into its texel: a plain read-modify-write (one owner lane per slot and launch)
__device__ __forceinline__ void add_light(Texel *out, uint32_t slot, const V3 light) {
    uint4 t = out[slot];
    t.x = __float_as_uint(__uint_as_float(t.x) + light.x);
    t.y = __float_as_uint(__uint_as_float(t.y) + light.y);
    t.z = __float_as_uint(__uint_as_float(t.z) + light.z);
    out[slot] = t;
}

// What a stats frame's bounce kernels close with: the block's steps, node visits and marched paths into the frame's counters (the
// secondary rays).  The two light-ray kernels (path_sun_kernel, path_lamp_rays_kernel) keep this text written out: called from
// them, the load of P.counters moves in their compiled code (profiles/path_templates_isa_diff.txt).
__device__ __forceinline__ void secondary_stats(const FrameParams &P, unsigned long long *acc, bool active, const MarchResult &R) {
    block_add(acc, 0, active ? R.iters : 0u);
    block_add(acc, 1, active ? R.visits : 0u);
    block_add(acc, 2, active ? 1ull : 0ull);
    __syncthreads();
    if (threadIdx.x == 0 && acc[2]) {
        atomicAdd(&P.counters[kCtrSteps], acc[0]);
        atomicAdd(&P.counters[kCtrVisits], acc[1]);
        atomicAdd(&P.counters[kCtrSecondary], acc[2]);
    }
}

// A wave's pool of rays (the bounce launches below): K batches of 64 paths, 4 words each in the wave's own LDS — unit[3]
// (phase A -> the hand-out), then pos[3] + the packed end state (the march -> phase C): 4 KiB per wave
constexpr uint32_t kPoolBatches = 4;                     // K
constexpr uint32_t kPoolEntries = kPoolBatches * 64u;
constexpr uint32_t kPoolWords = 4u * kPoolEntries;
constexpr uint32_t kPoolRefillAt = 16u;                  // idle lanes (of 64) that send the wave back to the pool

constexpr uint32_t kCellsPoolBytesPerWave = kPoolWords * 4u + kPoolEntries * 2u;   // the pool + a u16 order per entry

// what a launch of path_bounce_cells_kernel is given (one argument: the kernel reads it again for every segment)
struct CellsLaunch {
    FrameParams P;
    uint32_t refill_at;   // a wave takes rays from its pool when this many of its lanes are idle
    uint32_t segments;    // bounce segments in this launch: all that the frame's paths have left
};

}  // namespace vrt

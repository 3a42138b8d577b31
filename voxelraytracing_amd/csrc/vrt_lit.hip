// vrt_lit.hip — the sun marks of a table set (docs/NUMERICS.md "Lit stops"): the lit bits on the cell grid's air leaves
// (vrt_device.h kAirUnlit) and the shadow pool of lit voxels (kLitVoxel), which let a shadow ray of the one-launch frame stop where
// nothing can lie between it and the sun.  Everything about them is here:
//   the kernels      accel_lit_kernel (the cell marks, a launch per slab), accel_lit_voxels_kernel and its undo (the voxel marks),
//                    accel_floor_masks_kernel and accel_dark_kernel (the dark marks: kAirDark, "Dark stops"), accel_dark_voxels_kernel
//                    (the dark marks of the shadow pool: kDarkVoxel)
//   the plan         whether this world and sun get marks and which (lit_plan), the slab depth and the voxel layers by grid size
//   the frame hook   sun_marks_for_frame: vrt_render calls it for a one-launch shadow frame whose table set is up to date on its
//                    stream; it makes the marks there once they are due (ensure_sun_marks) and hands the frame its stops
//   the read-backs   vrt_get_sun_marks, vrt_read_lit_voxels, vrt_get_dark_marks, vrt_read_dark_voxels
// The state is vrt_ctx::Tables::SunMarks (vrt_ctx.h).  vrt_accel.hip builds the grid with every mark set, vrt_uploads.hip asks the
// record what a copy of a set takes along; nothing else touches the marks.
#include "vrt_ctx.h"

namespace vrt {

namespace {

// The lit pass: the sun marks of the cell grid's air leaves (vrt_device.h kAirUnlit; docs/NUMERICS.md "Lit stops").
//
// A cell is LIT when a shadow ray whose position is anywhere in it meets nothing from there to the world's face.  The host has
// picked the axis `a` on which the sun lies beyond the world (on the side `up`), and made sure that on the two other axes no ray
// towards the sun moves more than 0.99 voxels per voxel of `a` (LitPass; lit_plan below).  A ray with a position in
// cell C has the direction of a line to the sun through a point of C widened by one voxel (its positions stray from its line by
// the nudges, less than 500 * 0.001, and their roundings), so on each other axis `b` its slope (sun_b - q_b) / (sun_a - q_a) lies
// between the smallest and the largest one over the widened cell.  Layers are counted from C towards the sun; while the ray is in
// layer c_a + k it has risen between max(0, 4k - 5) and 4k + 5 voxels on `a` since it was in C, so its `b` lies in
//     [4 c_b + rise * slope_min - allow_k,  4 c_b + 4 + rise * slope_max + allow_k]      (each end with the rise that widens it)
// (and never beyond C's own cell on a side no ray of C points to: a ray's coordinates are monotone)
// where allow_k covers the nudges and roundings of the steps in between (0.015 per layer, never more than a ray's 500 steps can
// add up to: 1) and this kernel's own binary32 arithmetic (0.01).  The cells overlapping that interval on both axes are
// REACH_k(C): what a ray of C can be in while in layer c_a + k — a corridor along the rays, not a pyramid that widens by a cell
// per layer.  For a slab of `depth` layers whose sun-side end is m layers from C's layer (m = 1 .. depth):
//     lit(C)  <=>  for k = 0 .. m - 1 every cell of REACH_k(C) inside the world is an air leaf of at least `min_lo + 1` voxels, and
//                  every cell a ray of C can be in when it enters layer c_a + m is lit (or outside the world).
// The slabs are swept from the sun's side, so the marks behind a slab are final when it reads them, and all cells of a slab are
// independent: G / depth dependent launches.  depth = G is the whole corridor in one launch; depth = 1 has the reach of a sweep
// layer by layer.  Every air leaf of the grid gets its bit written, set or clear: nothing of an earlier sun or an earlier world
// survives a pass.  (A cell's bit is written while neighbours test its entry: they ask `>= kAirLeaf` and `& 31`, which the bit
// leaves alone.)
struct LitPass {
    uint32_t G;          // cells per axis
    uint32_t axis;       // 0, 1, 2: x, y, z
    uint32_t up;         // 1: the sun is beyond the world's high face of `axis`
    uint32_t min_lo;     // leaves below min_lo + 1 voxels are never lit (the step budget: docs/NUMERICS.md)
    float sun[3];        // settings.sun_pos - f32(world.min), as the shadow ray subtracts from it
};

// The cells of axis `b` a ray of cell c_b can be in after a rise of r_lo .. r_hi voxels, as [lo, hi] clamped to the world;
// false: all of them lie outside it.  s_min / s_max: the slopes over the widened cell.
__device__ inline bool lit_reach(float c4, float s_min, float s_max, float r_lo, float r_hi, float allow, uint32_t G, uint32_t *lo, uint32_t *hi) {
    const float b_lo = c4 + (s_min < 0.0f ? r_hi : r_lo) * s_min - allow;
    const float b_hi = c4 + 4.0f + (s_max > 0.0f ? r_hi : r_lo) * s_max + allow;
    int l = (int)floorf(b_lo * 0.25f), h = (int)floorf(b_hi * 0.25f);
    // a coordinate is monotone along a ray (a step adds a rounded product of the direction's sign): where no ray of the cell points
    // to lower `b` none gets below the cell it is in, whatever the allowance says, and likewise above
    const int own = (int)(c4 * 0.25f);
    if (!(s_min < 0.0f)) l = max(l, own);
    if (!(s_max > 0.0f)) h = min(h, own);
    if (h < 0 || l >= (int)G) return false;
    *lo = (uint32_t)max(l, 0);
    *hi = (uint32_t)min(h, (int)G - 1);
    return true;
}

// Smallest and largest slope on `b` of a line to the sun through the widened cell: sun_b - q_b in [n_lo, n_hi], sun_a - q_a in
// [d_lo, d_hi] (d_lo > 0: the sun lies beyond the widened world).
__device__ inline void lit_slopes(float n_lo, float n_hi, float d_lo, float d_hi, float *s_min, float *s_max) {
    *s_min = n_lo / (n_lo < 0.0f ? d_lo : d_hi);
    *s_max = n_hi / (n_hi > 0.0f ? d_lo : d_hi);
}

// One slab: layers first .. first + count - 1, counted from the sun's side; a thread per cell.
__global__ void __launch_bounds__(256) accel_lit_kernel(uint32_t *grid, LitPass lp, uint32_t first, uint32_t count) {
    const uint32_t G = lp.G, G1 = G + 1u;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count * G * G) return;
    const uint32_t a = lp.axis, u = a == 0u ? 1u : 0u, v = a == 2u ? 1u : 2u;   // the two other axes, the lower one fastest
    const size_t row = G1, slab = (size_t)G1 * G1;
    const size_t sa = a == 0u ? 1u : a == 1u ? row : slab, su = u == 0u ? 1u : row, sv = v == 1u ? row : slab;   // strides of [z][y][x]
    const uint32_t cu = t % G, cv = (t / G) % G, j = t / (G * G);
    const uint32_t ca = lp.up ? G - 1u - (first + j) : first + j;
    const size_t at = ca * sa + cu * su + cv * sv;
    const uint32_t e = grid[at];
    if (e < kAirLeaf) return;   // not an air leaf: no mark
    // the sweep's own frame: `a` mirrored when the sun is below, so that it grows towards the sun; i: the cell's layer there
    const float W = (float)(G * 4u);
    const float sun_a = lp.up ? lp.sun[a] : W - lp.sun[a], sun_u = lp.sun[u], sun_v = lp.sun[v];
    const float a4 = (float)((G - 1u - (first + j)) * 4u), u4 = (float)(cu * 4u), v4 = (float)(cv * 4u);
    const float d_lo = sun_a - (a4 + 5.0f), d_hi = sun_a - (a4 - 1.0f);
    float us_min, us_max, vs_min, vs_max;
    lit_slopes(sun_u - (u4 + 5.0f), sun_u - (u4 - 1.0f), d_lo, d_hi, &us_min, &us_max);
    lit_slopes(sun_v - (v4 + 5.0f), sun_v - (v4 - 1.0f), d_lo, d_hi, &vs_min, &vs_max);
    const size_t step = lp.up ? sa : (size_t)0 - sa;   // one layer towards the sun
    bool lit = true;
    size_t layer = ca * sa;
    for (uint32_t k = 0; k <= j && lit; k++, layer += step) {
        const float r_lo = k >= 2u ? (float)(4u * k - 5u) : 0.0f, r_hi = (float)(4u * k + 5u);
        const float allow = fminf(0.015f * (float)(k + 1u), 1.0f) + 0.01f;
        uint32_t ul, uh, vl, vh;
        if (!lit_reach(u4, us_min, us_max, r_lo, r_hi, allow, G, &ul, &uh) || !lit_reach(v4, vs_min, vs_max, r_lo, r_hi, allow, G, &vl, &vh)) continue;
        for (uint32_t nv = vl; nv <= vh; nv++)
            for (uint32_t nu = ul; nu <= uh; nu++) {
                const uint32_t own = grid[layer + nu * su + nv * sv];
                lit = lit && own >= kAirLeaf && (own & 31u) >= lp.min_lo;
            }
    }
    if (lit && first > 0u) {   // the layer behind the slab: its marks are final
        const uint32_t m = j + 1u;
        const float r_lo = m >= 2u ? (float)(4u * m - 5u) : 0.0f, r_hi = (float)(4u * m + 1u) + 0.01f;
        const float allow = fminf(0.015f * (float)(m + 1u), 1.0f) + 0.01f;
        uint32_t ul, uh, vl, vh;
        if (lit_reach(u4, us_min, us_max, r_lo, r_hi, allow, G, &ul, &uh) && lit_reach(v4, vs_min, vs_max, r_lo, r_hi, allow, G, &vl, &vh))
            for (uint32_t nv = vl; nv <= vh; nv++)
                for (uint32_t nu = ul; nu <= uh; nu++) {
                    const uint32_t nx = grid[layer + nu * su + nv * sv];
                    lit = lit && nx >= kAirLeaf && !(nx & kAirUnlit);
                }
    }
    // (a new pass re-arms the dark mark with the lit one: the dark pass behind this one sets it again where it holds)
    grid[at] = lit ? (e & ~(kAirUnlit | kAirDark)) : ((e & ~kAirDark) | kAirUnlit);
}

// The voxel marks: the lit rule carried down to the air voxels of SPLIT cells (docs/NUMERICS.md "Lit stops", the voxels of split
// cells; tests/lit_voxel_ref.py states it in numpy).  A shadow ray starts a hair above a surface voxel, so inside a split cell, where
// the cell marks say nothing; it walks that cell's and its neighbours' bricks voxel by voxel until it reaches an air leaf.  This
// pass writes the table set's SHADOW POOL: the brick pool entry for entry, except that an air voxel from which every shadow ray
// reaches lit cells through air holds kLitVoxel (its lo kept) — which the march loop of a shadow ray takes for a solid voxel, at no
// instruction of its own (vrt_march.h (u)).  The rule is the cell rule with a cell of one voxel: slopes over the voxel widened by a
// voxel, a rise of max(0, k - 2) .. k + 2 voxels to voxel layer k, the cell rule's allowance, one-sided intervals; layer 0 is the
// voxel's own.  Layer by layer towards the sun every voxel of the reach must be air (an air-leaf cell is air throughout); the walk
// ends LIT at the first layer whose whole reach lies in cells with the cell mark — a ray with a point of its path in a lit cell is a
// ray of that cell, and the cell's proof takes over — and UNLIT at a voxel that is not air, at the world's border, or after
// `layers` layers.  Runs behind accel_lit_kernel on its stream: the cell marks it reads are final.
// A wave takes 16 cells of the grid — cell w, w + waves, w + 2 waves ... of the G^3 numbered with y slowest: at 16 heights, because
// the split cells of a terrain lie together in a few layers, and a wave that met a whole row of them walked them one after the
// other while the others had left (64 cells in a row: 640 us more than the cell marks' pass for 64^3 cells; 16 cells a slab apart: 204;
// this: profiles/lit_voxels_ab.txt) — finds the split ones among them
// with one ballot, and gives each a trip with a lane per voxel.  Only bricks a cell of the grid points to are written; nothing else of the pool is ever read.
// A brick entry that holds kLitVoxel as the world's own voxel sets *clash: accel_lit_voxels_undo_kernel then makes the pool a plain copy.
constexpr uint32_t kLitVoxelCellsPerWave = 16u;
struct LitVoxelPass {
    uint32_t G;          // cells per axis
    uint32_t axis, up;   // as LitPass
    uint32_t layers;     // K: voxel layers beyond the voxel's own
    uint32_t entries;    // 16-bit entries of either pool
    float sun_a, sun_u, sun_v;   // the sun on the pass's axes: on `a` mirrored with the world when the sun is below
};

// The voxels of axis `b` a ray of voxel i can be in after a rise of r_lo .. r_hi voxels, as [lo, hi]; false: some lie beyond the world.
__device__ inline bool lit_voxel_reach(float i, float s_min, float s_max, float r_lo, float r_hi, float allow, int W, int *lo, int *hi) {
    const float b_lo = i + (s_min < 0.0f ? r_hi : r_lo) * s_min - allow;
    const float b_hi = i + 1.0f + (s_max > 0.0f ? r_hi : r_lo) * s_max + allow;
    int l = (int)floorf(b_lo), h = (int)floorf(b_hi);
    const int own = (int)i;
    if (!(s_min < 0.0f)) l = max(l, own);   // (monotone coordinates, as lit_reach)
    if (!(s_max > 0.0f)) h = min(h, own);
    *lo = l;
    *hi = h;
    return l >= 0 && h < W;
}

// The walk of one air voxel, in the pass's own frame: `a` the sun's axis (mirrored when the sun is below, so that it grows towards
// the sun), u and v the two others; ca / cu / cv: the strides of a cell in the bordered grid, ha / hu / hv: the shifts of a voxel's
// two low bits in a brick's index.  One exit: the loops carry flags, not returns.
__device__ inline bool lit_voxel_walk(const uint32_t *grid, const uint16_t *bricks, const LitVoxelPass &lp, int ia, int iu, int iv, uint32_t ca,
                                      uint32_t cu, uint32_t cv, uint32_t ha, uint32_t hu, uint32_t hv) {
    const int W = (int)(lp.G * 4u);
    const float fa = (float)ia, fu = (float)iu, fv = (float)iv;
    const float d_lo = lp.sun_a - (fa + 2.0f), d_hi = lp.sun_a - (fa - 1.0f);
    float us_min, us_max, vs_min, vs_max;
    lit_slopes(lp.sun_u - (fu + 2.0f), lp.sun_u - (fu - 1.0f), d_lo, d_hi, &us_min, &us_max);
    lit_slopes(lp.sun_v - (fv + 2.0f), lp.sun_v - (fv - 1.0f), d_lo, d_hi, &vs_min, &vs_max);
    bool open = true, lit = false;
    for (uint32_t k = 0; k <= lp.layers && open; k++) {
        const int la = ia + (int)k;
        const float r_lo = k >= 2u ? (float)(k - 2u) : 0.0f, r_hi = (float)(k + 2u);
        const float allow = fminf(0.015f * (float)(k + 1u), 1.0f) + 0.01f;
        int ul, uh, vl, vh;
        const bool in_u = lit_voxel_reach(fu, us_min, us_max, r_lo, r_hi, allow, W, &ul, &uh);
        const bool in_v = lit_voxel_reach(fv, vs_min, vs_max, r_lo, r_hi, allow, W, &vl, &vh);
        if (!in_u || !in_v || la >= W) break;   // the world's border: unlit
        const uint32_t qa = (uint32_t)(lp.up ? la : W - 1 - la);
        const uint32_t cell_a = (qa >> 2) * ca, bit_a = (qa & 3u) << ha;
        bool all_air = true, all_lit = true;
        for (int nv = vl; nv <= vh; nv++)
            for (int nu = ul; nu <= uh; nu++) {
                // (every coordinate is inside the world here: the cell is one of the grid's G^3)
                const uint32_t e = grid[cell_a + ((uint32_t)nu >> 2) * cu + ((uint32_t)nv >> 2) * cv];
                const bool split = is_split_entry(e);
                const uint32_t at = (e & 0x7FFFFFC0u) + (bit_a | (((uint32_t)nu & 3u) << hu) | (((uint32_t)nv & 3u) << hv));
                uint32_t voxel = 1u;   // (a brick beyond the pool: not air)
                if (split && at < lp.entries) voxel = (uint32_t)bricks[at] >> 1;
                all_air = all_air && (e >= kAirLeaf || (split && voxel == 0u));   // (an air-leaf cell is air throughout)
                all_lit = all_lit && e >= kAirLeaf && !(e & (kAirUnlit | kAirDark));   // (a dark leaf has bit 22 clear too.  None is here today: accel_lit_kernel has just cleared bit 21 and the dark pass runs behind this one; the test holds should the passes be reordered)
            }
        open = all_air && !all_lit;
        lit = all_air && all_lit;
    }
    return lit;
}

__global__ void __launch_bounds__(256) accel_lit_voxels_kernel(const uint32_t *grid, const uint16_t *bricks, uint16_t *lit_bricks, LitVoxelPass lp,
                                                               uint32_t *clash) {
    const uint32_t G = lp.G, G1 = G + 1u, lane = threadIdx.x & 63u;
    const uint32_t cells = G * G * G, waves = (cells + kLitVoxelCellsPerWave - 1u) / kLitVoxelCellsPerWave;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (wave >= waves) return;   // (wave-uniform)
    const uint32_t mine = wave + lane * waves;   // (below 2^32: lane < kLitVoxelCellsPerWave where it is used)
    uint32_t e_mine = 0u;
    // (the cells are numbered with y slowest — x = n % G, z = n / G % G, y = n / G^2 — so that a wave's cells lie at 16 heights)
    if (lane < kLitVoxelCellsPerWave && mine < cells) e_mine = grid[(((mine / G) % G) * G1 + mine / (G * G)) * G1 + mine % G];   // (below 2^32: grid_dim <= 800)
    const uint32_t a = lp.axis, u = a == 0u ? 1u : 0u, v = a == 2u ? 1u : 2u;   // the two other axes, as accel_lit_kernel
    const uint32_t cs[3] = {1u, G1, G1 * G1};
    const uint32_t ca = cs[a], cu = cs[u], cv = cs[v], ha = 2u * a, hu = 2u * u, hv = 2u * v;
    const int W = (int)(G * 4u);
    unsigned long long todo = __ballot(is_split_entry(e_mine));
    while (todo) {
        const uint32_t i = (uint32_t)__ffsll((long long)todo) - 1u;
        todo &= todo - 1ull;
        const uint32_t e = (uint32_t)__shfl((int)e_mine, (int)i, 64), cell = wave + i * waves;
        if ((e & 0x7FFFFFC0u) + 64u > lp.entries) continue;   // (wave-uniform: a brick beyond the pool is never read by the march either)
        const uint32_t at = (e & 0x7FFFFFC0u) + lane;
        const int px = (int)((cell % G) * 4u + (lane & 3u)), py = (int)((cell / (G * G)) * 4u + ((lane >> 2) & 3u)), pz = (int)(((cell / G) % G) * 4u + (lane >> 4));
        const int pa = a == 0u ? px : a == 1u ? py : pz, pu = u == 0u ? px : py, pv = v == 1u ? py : pz;
        uint32_t b = bricks[at];
        if ((b >> 1) == kLitVoxel) atomicOr(clash, 1u);
        if ((b >> 1) == 0u && lit_voxel_walk(grid, bricks, lp, lp.up ? pa : W - 1 - pa, pu, pv, ca, cu, cv, ha, hu, hv)) b |= kLitVoxel << 1;
        lit_bricks[at] = (uint16_t)b;
    }
}

// ... and where the world itself holds kLitVoxel in a brick: the shadow pool becomes the plain one without any mark — entry for
// entry, but for the world's own voxels of that id, which are written as the id below it: as solid and as little a liquid to a
// shadow ray, of which the frame reads `hit` alone (the host builds no marks where the liquid table could tell the two apart)
__global__ void __launch_bounds__(256) accel_lit_voxels_undo_kernel(const uint32_t *clash, const uint32_t *bricks, uint32_t *lit_bricks, uint32_t words) {
    if (*clash == 0u) return;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < words; i += gridDim.x * blockDim.x) {
        uint32_t w = bricks[i];
        if (((w >> 1) & 0x7FFFu) == kLitVoxel) w &= ~2u;          // (0x7FFF -> 0x7FFE: the voxel's lowest bit is the entry's bit 1)
        if ((w >> 17) == kLitVoxel) w &= ~(2u << 16);
        lit_bricks[i] = w;
    }
}

// The voxel marks of a table set, on `st` behind launch_accel_lit: `lit_bricks` becomes the shadow pool of `bricks` (both of
// `entries` 16-bit entries, a multiple of 64); *clash (device) is cleared, and set if the world holds kLitVoxel in a brick.
void launch_accel_lit_voxels(const uint32_t *grid, const uint16_t *bricks, uint16_t *lit_bricks, uint32_t entries, uint32_t G, uint32_t axis, bool up,
                             const float sun[3], uint32_t layers, uint32_t *clash, hipStream_t st) {
    const uint32_t u = axis == 0u ? 1u : 0u, v = axis == 2u ? 1u : 2u;
    const LitVoxelPass lp{G, axis, up ? 1u : 0u, layers, entries, up ? sun[axis] : (float)(G * 4u) - sun[axis], sun[u], sun[v]};
    if (hipMemsetAsync(clash, 0, sizeof(uint32_t), st) != hipSuccess) return;   // (the caller asks hipGetLastError)
    const uint32_t waves = (G * G * G + kLitVoxelCellsPerWave - 1u) / kLitVoxelCellsPerWave;
    hipLaunchKernelGGL(accel_lit_voxels_kernel, dim3((waves + 3u) / 4u), dim3(256), 0, st, grid, bricks, lit_bricks, lp, clash);
    const uint32_t words = entries / 2u, blocks = (words + 255u) / 256u;
    hipLaunchKernelGGL(accel_lit_voxels_undo_kernel, dim3(blocks < 1024u ? (blocks ? blocks : 1u) : 1024u), dim3(256), 0, st, clash,
                       reinterpret_cast<const uint32_t *>(bricks), reinterpret_cast<uint32_t *>(lit_bricks), words);
}

// The lit pass over the whole grid, on `st`: a launch per slab of `depth` layers, from the sun's side (the last one may be short).
void launch_accel_lit(uint32_t *grid, uint32_t G, uint32_t axis, bool up, uint32_t min_lo, const float sun[3], uint32_t depth, hipStream_t st) {
    const LitPass lp{G, axis, up ? 1u : 0u, min_lo, {sun[0], sun[1], sun[2]}};
    if (depth < 1u) depth = 1u;
    for (uint32_t first = 0; first < G; first += depth) {
        const uint32_t count = G - first < depth ? G - first : depth;
        hipLaunchKernelGGL(accel_lit_kernel, dim3((count * G * G + 255u) / 256u), dim3(256), 0, st, grid, lp, first, count);
    }
}

// The dark pass: the dark marks of the cell grid's air leaves (vrt_device.h kAirDark; docs/NUMERICS.md "Dark stops";
// tests/dark_cell_ref.py states the rule in numpy).  An all-air cell C of layer c_a is DARK when for some k >= 1 (c_a + k inside the
// world, k <= depth) REACH_j(C) lies wholly inside the world for every j = 0 .. k — no ray of C can have left it sideways — and the
// cells of REACH_k(C) share a closed voxel layer: one of the four voxel layers across `a` in which every one of them holds 16 solid
// voxels that are no liquid.  A ray of C rises monotonely through adjacent leaves, so unless it ends before (a hit, or its lookups
// spent, which the reference reports as a hit) it looks up a voxel of that layer in one of those cells.  REACH is the lit rule's,
// but computed in binary64 in the order tests/dark_cell_ref.py computes it: the marks are the reference's cell for cell.
// Two launches behind the lit passes: the floor masks (a byte per cell, bit j: voxel layer j across `a` is closed), then a thread per
// cell, which walks its corridor until the rule holds or the corridor touches the world's side.  Only air leaves that are not lit are
// walked, and each gets its two bits written: dark, or unlit.
struct DarkPass {
    uint32_t G, axis, up, depth;
    float sun[3];
    uint32_t liquid[8];   // bit v: material v is a liquid (ids above 255 are material 255)
};

__global__ void __launch_bounds__(256) accel_floor_masks_kernel(const uint32_t *grid, const uint16_t *bricks, uint32_t entries, uint8_t *floors, DarkPass dp) {
    const uint32_t G = dp.G, G1 = G + 1u;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= G * G * G) return;
    const size_t at = ((size_t)(t / (G * G)) * G1 + (t / G) % G) * G1 + t % G;
    const uint32_t e = grid[at];
    auto blocks = [&](uint32_t voxel) {
        const uint32_t id = voxel < 255u ? voxel : 255u;
        return voxel != 0u && !((dp.liquid[id >> 5] >> (id & 31u)) & 1u);
    };
    uint32_t m = 0u;
    if (is_split_entry(e)) {
        const uint32_t base = e & 0x7FFFFFC0u, sh = 2u * dp.axis;
        if (base + 64u <= entries) {   // (a brick beyond the pool is never read by the march either)
            m = 15u;
            for (uint32_t i = 0; i < 64u; i++)
                if (!blocks((uint32_t)bricks[base + i] >> 1)) m &= ~(1u << ((i >> sh) & 3u));
        }
    } else if (e < kAirLeaf && e != 0u) {
        m = blocks(e >> 16) ? 15u : 0u;
    }
    floors[at] = (uint8_t)m;
}

// The cells of axis `b` of REACH, as [lo, hi]; false: some lie beyond the world (tests/dark_cell_ref.py: _reach)
__device__ inline bool dark_reach(double c4, double s_min, double s_max, double r_lo, double r_hi, double allow, int G, int *lo, int *hi) {
    const double b_lo = c4 + (s_min < 0.0 ? r_hi : r_lo) * s_min - allow;
    const double b_hi = c4 + 4.0 + (s_max > 0.0 ? r_hi : r_lo) * s_max + allow;
    int l = (int)floor(b_lo / 4.0), h = (int)floor(b_hi / 4.0);
    const int own = (int)(c4 / 4.0);
    if (!(s_min < 0.0)) l = max(l, own);   // (monotone coordinates, as lit_reach)
    if (!(s_max > 0.0)) h = min(h, own);
    *lo = l;
    *hi = h;
    return l >= 0 && h < G;
}

__device__ inline void dark_slopes(double n_lo, double n_hi, double d_lo, double d_hi, double *s_min, double *s_max) {
    *s_min = n_lo / (n_lo < 0.0 ? d_lo : d_hi);
    *s_max = n_hi / (n_hi > 0.0 ? d_lo : d_hi);
}

__global__ void __launch_bounds__(256) accel_dark_kernel(uint32_t *grid, const uint8_t *floors, DarkPass dp) {
    const uint32_t G = dp.G, G1 = G + 1u;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= G * G * G) return;
    const uint32_t a = dp.axis, u = a == 0u ? 1u : 0u, v = a == 2u ? 1u : 2u;   // as accel_lit_kernel
    const size_t row = G1, slab = (size_t)G1 * G1;
    const size_t sa = a == 0u ? 1u : a == 1u ? row : slab, su = u == 0u ? 1u : row, sv = v == 1u ? row : slab;
    const uint32_t cu = t % G, cv = (t / G) % G, i = t / (G * G);   // i: the cell's layer in the pass's frame, which grows towards the sun
    const uint32_t ca = dp.up ? i : G - 1u - i;
    const size_t at = ca * sa + cu * su + cv * sv;
    const uint32_t e = grid[at];
    if (e < kAirLeaf || !(e & (kAirUnlit | kAirDark))) return;   // not an air leaf, or a lit one
    const double W = (double)(G * 4u);
    const double sun_a = dp.up ? (double)dp.sun[a] : W - (double)dp.sun[a], sun_u = (double)dp.sun[u], sun_v = (double)dp.sun[v];
    const double a4 = 4.0 * (double)i, u4 = 4.0 * (double)cu, v4 = 4.0 * (double)cv;
    const double d_lo = sun_a - (a4 + 5.0), d_hi = sun_a - (a4 - 1.0);
    double us_min, us_max, vs_min, vs_max;
    dark_slopes(sun_u - (u4 + 5.0), sun_u - (u4 - 1.0), d_lo, d_hi, &us_min, &us_max);
    dark_slopes(sun_v - (v4 + 5.0), sun_v - (v4 - 1.0), d_lo, d_hi, &vs_min, &vs_max);
    const size_t step = dp.up ? sa : (size_t)0 - sa;   // one layer towards the sun
    const uint32_t k_max = min(dp.depth, G - 1u - i);
    bool dark = false;
    size_t layer = ca * sa;
    for (uint32_t k = 0; k <= k_max; k++, layer += step) {
        const double r_lo = k >= 2u ? 4.0 * (double)k - 5.0 : 0.0, r_hi = 4.0 * (double)k + 5.0;
        const double allow = fmin(0.015 * (double)(k + 1u), 1.0) + 0.01;
        int ul, uh, vl, vh;
        if (!dark_reach(u4, us_min, us_max, r_lo, r_hi, allow, (int)G, &ul, &uh) || !dark_reach(v4, vs_min, vs_max, r_lo, r_hi, allow, (int)G, &vl, &vh))
            break;   // a ray of C may leave the world sideways from here on
        if (k == 0u) continue;
        uint32_t m = 15u;
        for (int nv = vl; nv <= vh; nv++)
            for (int nu = ul; nu <= uh; nu++) m &= floors[layer + (size_t)nu * su + (size_t)nv * sv];
        if (m) { dark = true; break; }
    }
    grid[at] = dark ? ((e & ~kAirUnlit) | kAirDark) : ((e & ~kAirDark) | kAirUnlit);
}

// The dark pass of a table set, on `st` behind the lit passes: `floors` (a byte per entry of the bordered grid) is its scratch.
void launch_accel_dark(uint32_t *grid, const uint16_t *bricks, uint32_t entries, uint8_t *floors, uint32_t G, uint32_t axis, bool up, const float sun[3],
                       uint32_t depth, const uint32_t liquid[8], hipStream_t st) {
    DarkPass dp{G, axis, up ? 1u : 0u, depth, {sun[0], sun[1], sun[2]}, {}};
    for (int i = 0; i < 8; i++) dp.liquid[i] = liquid[i];
    const uint32_t blocks = (G * G * G + 255u) / 256u;
    hipLaunchKernelGGL(accel_floor_masks_kernel, dim3(blocks), dim3(256), 0, st, grid, bricks, entries, floors, dp);
    hipLaunchKernelGGL(accel_dark_kernel, dim3(blocks), dim3(256), 0, st, grid, floors, dp);
}

// The dark voxel marks: the dark rule carried down to the air voxels of SPLIT cells (docs/NUMERICS.md "Dark stops", the voxels of
// split cells; tests/dark_voxel_ref.py states it in numpy).  An occluded shadow ray starts a hair above a surface voxel, inside a
// split cell, and walks bricks voxel by voxel until it hits or reaches a dark cell.  An air voxel of a split cell that holds no lit
// mark is DARK when for some k, 1 <= k <= layers, REACH_j lies wholly inside the world for every j = 0 .. k, voxel layer i_a + k with
// it, and every voxel of REACH_k is CLOSED: a solid voxel that is no liquid (a solid leaf cell is solid throughout), or a voxel of a
// cell with the dark cell mark.  REACH is the lit voxel rule's — the voxel widened by a voxel, a rise of max(0, k - 2) .. k + 2, the
// cell rule's allowance, one-sided intervals — but computed in binary64 in the order tests/dark_voxel_ref.py computes it: the marks
// are the reference's voxel for voxel.  A ray with a point in the voxel rises monotonely, so it looks up a voxel of REACH_k unless it
// ends before, and every way to end before is a hit (a solid voxel, or its lookups spent): no step budget.  The pass writes
// kDarkVoxel (the entry's lo kept) into the shadow pool, which the march takes for the solid voxel it is.
// Runs behind accel_dark_kernel (the cell marks it reads are final; where that pass is off no leaf carries kAirDark and solid voxels
// alone close a corridor) and behind accel_lit_voxels_undo_kernel, whose *clash it reads: a
// pool that was made a plain copy gets no mark.  The work distribution is accel_lit_voxels_kernel's; only the wave's own pool
// entries are written, and only the grid and the plain bricks are read beside them.
struct DarkVoxelPass {
    uint32_t G, axis, up;
    uint32_t layers;     // K_d: voxel layers beyond the voxel's own
    uint32_t entries;    // 16-bit entries of either pool
    float sun[3];
    uint32_t liquid[8];  // as DarkPass
};

// The voxels of axis `b` of REACH, as [lo, hi]; false: some lie beyond the world (tests/lit_voxel_ref.py: _reach)
__device__ inline bool dark_voxel_reach(double i, double s_min, double s_max, double r_lo, double r_hi, double allow, int W, int *lo, int *hi) {
    const double b_lo = i + (s_min < 0.0 ? r_hi : r_lo) * s_min - allow;
    const double b_hi = i + 1.0 + (s_max > 0.0 ? r_hi : r_lo) * s_max + allow;
    int l = (int)floor(b_lo), h = (int)floor(b_hi);
    const int own = (int)i;
    if (!(s_min < 0.0)) l = max(l, own);   // (monotone coordinates, as lit_reach)
    if (!(s_max > 0.0)) h = min(h, own);
    *lo = l;
    *hi = h;
    return l >= 0 && h < W;
}

// The walk of one air voxel, in the pass's own frame (as lit_voxel_walk).  One exit: the loops carry flags, not returns.
__device__ inline bool dark_voxel_walk(const uint32_t *grid, const uint16_t *bricks, const DarkVoxelPass &dp, int ia, int iu, int iv, uint32_t ca,
                                       uint32_t cu, uint32_t cv, uint32_t ha, uint32_t hu, uint32_t hv) {
    const int W = (int)(dp.G * 4u);
    const uint32_t a = dp.axis, u = a == 0u ? 1u : 0u, v = a == 2u ? 1u : 2u;
    const double fa = (double)ia, fu = (double)iu, fv = (double)iv;
    const double sun_a = dp.up ? (double)dp.sun[a] : (double)W - (double)dp.sun[a], sun_u = (double)dp.sun[u], sun_v = (double)dp.sun[v];
    const double d_lo = sun_a - (fa + 2.0), d_hi = sun_a - (fa - 1.0);
    double us_min, us_max, vs_min, vs_max;
    dark_slopes(sun_u - (fu + 2.0), sun_u - (fu - 1.0), d_lo, d_hi, &us_min, &us_max);
    dark_slopes(sun_v - (fv + 2.0), sun_v - (fv - 1.0), d_lo, d_hi, &vs_min, &vs_max);
    auto blocks = [&](uint32_t voxel) {
        const uint32_t id = voxel < 255u ? voxel : 255u;
        return voxel != 0u && !((dp.liquid[id >> 5] >> (id & 31u)) & 1u);
    };
    bool inside = true, dark = false;
    for (uint32_t k = 0; k <= dp.layers && inside && !dark; k++) {
        const int la = ia + (int)k;
        const double r_lo = k >= 2u ? (double)k - 2.0 : 0.0, r_hi = (double)k + 2.0;
        const double allow = fmin(0.015 * (double)(k + 1u), 1.0) + 0.01;
        int ul, uh, vl, vh;
        const bool in_u = dark_voxel_reach(fu, us_min, us_max, r_lo, r_hi, allow, W, &ul, &uh);
        const bool in_v = dark_voxel_reach(fv, vs_min, vs_max, r_lo, r_hi, allow, W, &vl, &vh);
        inside = in_u && in_v && la < W;   // false: a ray of the voxel may leave the world from here on
        if (!inside || k == 0u) continue;
        const uint32_t qa = (uint32_t)(dp.up ? la : W - 1 - la);
        const uint32_t cell_a = (qa >> 2) * ca, bit_a = (qa & 3u) << ha;
        bool shut = true;
        for (int nv = vl; nv <= vh && shut; nv++)
            for (int nu = ul; nu <= uh && shut; nu++) {
                // (every coordinate is inside the world here: the cell is one of the grid's G^3)
                const uint32_t e = grid[cell_a + ((uint32_t)nu >> 2) * cu + ((uint32_t)nv >> 2) * cv];
                if (e >= kAirLeaf) {
                    shut = (e & kAirDark) != 0u;   // an air leaf: closed where every ray of the cell hits
                } else if (is_split_entry(e)) {
                    const uint32_t at = (e & 0x7FFFFFC0u) + (bit_a | (((uint32_t)nu & 3u) << hu) | (((uint32_t)nv & 3u) << hv));
                    shut = at < dp.entries && blocks((uint32_t)bricks[at] >> 1);   // (a brick beyond the pool: not closed)
                } else {
                    shut = e != 0u && blocks(e >> 16);
                }
            }
        dark = shut;
    }
    return dark;
}

__global__ void __launch_bounds__(256) accel_dark_voxels_kernel(const uint32_t *grid, const uint16_t *bricks, uint16_t *lit_bricks, DarkVoxelPass dp,
                                                                const uint32_t *clash) {
    if (*clash != 0u) return;   // the world holds kLitVoxel in a brick: the pool is a plain copy, and stays one
    const uint32_t G = dp.G, G1 = G + 1u, lane = threadIdx.x & 63u;
    const uint32_t cells = G * G * G, waves = (cells + kLitVoxelCellsPerWave - 1u) / kLitVoxelCellsPerWave;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (wave >= waves) return;   // (wave-uniform)
    const uint32_t mine = wave + lane * waves;   // (as accel_lit_voxels_kernel: the cells at 16 heights, numbered with y slowest)
    uint32_t e_mine = 0u;
    if (lane < kLitVoxelCellsPerWave && mine < cells) e_mine = grid[(((mine / G) % G) * G1 + mine / (G * G)) * G1 + mine % G];
    const uint32_t a = dp.axis, u = a == 0u ? 1u : 0u, v = a == 2u ? 1u : 2u;
    const uint32_t cs[3] = {1u, G1, G1 * G1};
    const uint32_t ca = cs[a], cu = cs[u], cv = cs[v], ha = 2u * a, hu = 2u * u, hv = 2u * v;
    const int W = (int)(G * 4u);
    unsigned long long todo = __ballot(is_split_entry(e_mine));
    while (todo) {
        const uint32_t i = (uint32_t)__ffsll((long long)todo) - 1u;
        todo &= todo - 1ull;
        const uint32_t e = (uint32_t)__shfl((int)e_mine, (int)i, 64), cell = wave + i * waves;
        if ((e & 0x7FFFFFC0u) + 64u > dp.entries) continue;   // (wave-uniform: the lit voxel pass wrote no such brick either)
        const uint32_t at = (e & 0x7FFFFFC0u) + lane;
        const int px = (int)((cell % G) * 4u + (lane & 3u)), py = (int)((cell / (G * G)) * 4u + ((lane >> 2) & 3u)), pz = (int)(((cell / G) % G) * 4u + (lane >> 4));
        const int pa = a == 0u ? px : a == 1u ? py : pz, pu = u == 0u ? px : py, pv = v == 1u ? py : pz;
        const uint32_t b = bricks[at];
        // an air voxel of the world that the lit voxel pass, which wrote this entry of the pool, left without its mark
        if ((b >> 1) == 0u && ((uint32_t)lit_bricks[at] >> 1) != kLitVoxel &&
            dark_voxel_walk(grid, bricks, dp, dp.up ? pa : W - 1 - pa, pu, pv, ca, cu, cv, ha, hu, hv))
            lit_bricks[at] = (uint16_t)((kDarkVoxel << 1) | (b & 1u));
    }
}

// The dark voxel marks of a table set, on `st` behind launch_accel_lit_voxels and launch_accel_dark.
void launch_accel_dark_voxels(const uint32_t *grid, const uint16_t *bricks, uint16_t *lit_bricks, uint32_t entries, uint32_t G, uint32_t axis, bool up,
                              const float sun[3], uint32_t layers, const uint32_t liquid[8], const uint32_t *clash, hipStream_t st) {
    DarkVoxelPass dp{G, axis, up ? 1u : 0u, layers, entries, {sun[0], sun[1], sun[2]}, {}};
    for (int i = 0; i < 8; i++) dp.liquid[i] = liquid[i];
    const uint32_t waves = (G * G * G + kLitVoxelCellsPerWave - 1u) / kLitVoxelCellsPerWave;
    hipLaunchKernelGGL(accel_dark_voxels_kernel, dim3((waves + 3u) / 4u), dim3(256), 0, st, grid, bricks, lit_bricks, dp, clash);
}

}  // namespace

}  // namespace vrt

namespace {

using Tables = vrt_ctx::Tables;
using SunMarks = Tables::SunMarks;

// Whether this world and this sun get marks, and which: the axis on which the sun lies beyond the world, the smallest leaf that is
// marked, and the wave trip count up to which a mark may stop a shadow ray.
struct LitPlan { uint32_t axis; bool up; uint32_t min_lo, trips; };
constexpr uint32_t kLitSettleFrames = 4;
bool lit_plan(uint32_t world_size, const float sun[3], LitPlan *lp) {
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(sun[k])) return false;
    // every ray's line passes within one voxel of the cells it is in: the directions are those from the box widened by a voxel
    const float lo = -1.0f, hi = (float)world_size + 1.0f;
    float best = 0.0f;
    for (uint32_t a = 0; a < 3; a++)
        for (int up = 0; up < 2; up++) {
            const float clear = up ? sun[a] - hi : lo - sun[a];   // the sun's distance beyond the face, along the axis
            if (clear > best) { best = clear; lp->axis = a; lp->up = up != 0; }
        }
    if (!(best > 0.0f)) return false;   // the sun is inside the world (or within a voxel of it on every axis)
    for (uint32_t b = 0; b < 3; b++) {
        if (b == lp->axis) continue;
        const float lateral = std::max(std::fabs(sun[b] - lo), std::fabs(sun[b] - hi));
        if (!(lateral <= 0.99f * best)) return false;   // some ray could cross more than a cell sideways per layer
    }
    // The step budget: through air leaves of at least L voxels a ray takes at most B = 6 (W / L + 1) + 2 steps to the world's face
    // (docs/NUMERICS.md); a lit entry stops a lane only while the wave's trip count leaves the reference's ray B + 1 of its 500
    for (uint32_t L = 4u; L <= 32u; L *= 2u) {
        const uint32_t B = 6u * (world_size / L + 1u) + 2u;
        if (B + 2u <= vrt::kMaxSteps) { lp->min_lo = L - 1u; lp->trips = vrt::kMaxSteps - B - 1u; return true; }
    }
    return false;
}

// How many layers a launch of the lit pass tests a cell's corridor over before it relies on the marks behind (accel_lit_kernel): the
// largest depth whose pass pays for itself within 100 frames of the world it is built for, measured per grid size
// (profiles/lit_corridor_ab.txt).  Up to 64 cells a side the whole corridor: one launch, 97 us where the sweep layer by layer took
// 305, and 5.7 us off every frame.  Larger grids gain no frame time at any depth (their marks sit on leaves of 8 or 16 voxels, high
// over the terrain), so a depth qualifies while its pass is no dearer than the layer-by-layer sweep's, for a sun on any axis:
// 32 up to 128 cells a side (312 us against 494; the whole corridor: 769), 8 above (313 us against 696 for 240 cells; 16 is dearer
// than the sweep for a sun on x).  VRT_LIT_SLAB overrides: the A/B, and the tests' comparison of the rules inside one build
// (1: the reach of a sweep layer by layer).
uint32_t lit_slab_depth(const vrt_ctx *c, uint32_t G) {
    const uint32_t depth = c->lit_slab ? c->lit_slab : G <= 64u ? G : G <= 128u ? 32u : 8u;
    return depth < G ? depth : G;
}

// The voxel marks (accel_lit_voxels_kernel): how many voxel layers K a voxel's walk may take before it gives up, per
// grid size, by the slab depth's rule — the largest K whose pass pays for itself within 100 frames (profiles/lit_voxels_ab.txt);
// 0: no voxel marks at that size.  Up to 64 cells a side 8 layers: 99 us on the pass for 2.1 us off every frame (4: 59 us for 1.2; 12: 134
// us for the same 2.1).  128 cells a side: the frames gain 2.0 us at 8 layers, but the pass costs 376 us more: 185 frames, so none; 240: the
// frames get slower with the second pool, none.  VRT_LIT_VOXEL_LAYERS overrides.  And what K costs the step budget (docs/NUMERICS.md "Lit
// stops"): from a lit voxel to the first lit cell a ray crosses at most K + 1 voxel planes of the sun's axis and, its slopes below
// one over a rise of at most K + 2, K + 3 of each other axis with the widened voxel's — 3 K + 6 in all, allowed for in full —
// and one re-step per plane.
uint32_t lit_voxel_layers(const vrt_ctx *c, uint32_t G) {
    if (!c->lit_voxels) return 0u;
    if (c->lit_voxel_layers >= 0) return (uint32_t)c->lit_voxel_layers;
    return G <= 64u ? 8u : 0u;
}
uint32_t lit_voxel_budget(uint32_t layers) { return 2u * (3u * layers + 6u); }

// The dark marks (accel_dark_kernel): how many layers a cell's corridor is walked over before the cell is left unmarked, per grid
// size, by the slab depth's rule — the largest depth whose pass pays for itself within 100 frames, each step up paying for its own
// extra (profiles/dark_marks_ab.txt); 0: no dark marks at that size.  Up to 64 cells a side 32 layers: 60 us on the pass for 5.7 us off
// every frame of the standing view (16: 40 us for 4.3; 64: 76 us for the same 5.8, the same 179 cells).  128 cells a side: 130 us for
// 0.3 us, inside the spread: none; larger grids were not measured: none.  VRT_DARK_DEPTH overrides, VRT_DARK_MARKS=0 switches them off.
uint32_t dark_depth(const vrt_ctx *c, uint32_t G) {
    if (!c->dark_marks) return 0u;
    const uint32_t depth = c->dark_depth >= 0 ? (uint32_t)c->dark_depth : G <= 64u ? 32u : 0u;
    return depth < G ? depth : G;
}

// The dark voxel marks (accel_dark_voxels_kernel): how many voxel layers K_d a voxel's walk may take, per grid size, by the same rule —
// the largest K_d whose pass pays for itself within 100 frames, each step up paying for its own extra (profiles/dark_voxels_ab.txt);
// 0: no dark voxel marks.  Up to 64 cells a side 16 layers: 97 us on the pass for 1.2 to 1.4 us off every frame of the standing view
// (two / one in flight), 70 to 82 frames (8: 53 us for 0.24 to 0.35, 150 to 220 frames, but the step from 8 to 16 buys 1.0 us for
// 44 us; 32: 185 us for 1.95 to 2.21, whose 88 us over 16 buy 0.8 us: 107 to 114 frames, so not 32).  Above 64 cells a side the lit voxel marks are off and there is no shadow pool to mark: none; not measured.
// VRT_DARK_VOXEL_LAYERS overrides; 0 switches the marks off: the frames then run as they did before these marks.
uint32_t dark_voxel_layers(const vrt_ctx *c, uint32_t G) {
    if (c->dark_voxel_layers >= 0) return (uint32_t)c->dark_voxel_layers;
    return G <= 64u ? 16u : 0u;
}

// Marks are worth a pass (0.4 ms for 64^3 cells, 0.9 ms for the client's 240^3: profiles/sun_marks_edit_cost.txt) once what
// they are made from stands still: while edits arrive or the sun moves from frame to frame, the frames run without marks,
// as they always did, and the pass follows kLitSettleFrames frames after the last change.  True: this frame is that one.
bool settled(SunMarks &L, const SunMarks::Key &now) {
    if (!(L.want_frames && L.want.same(now))) { L.want = now; L.want_frames = 0u; }
    if (++L.want_frames < kLitSettleFrames) return false;
    L.want_frames = 0u;
    return true;
}

// Ordered like the chunk updates of update_tables, which it follows on the frame's stream `st`: the pass is one launch per slab (ceil(G / depth): 1, 4 or 30 for the bench's worlds)
// on `st`, behind the set's chunk update and before the frame; nothing waits for it on the host.  Whoever else reads the set:
//   - frames of the set's own frame set run on `st` too: stream order;
//   - a split set (edits arriving: every frame set its own tables) has no other readers;
//   - the shared set tabs[0], read from several streams: frames of OTHER frame sets still in flight are waited for as update_tables
//     waits for them before it rewrites a shared set (quiesce: the one host wait, of at most the frames in flight, and only when the
//     sun moved or the world was built — an edit splits the sets first); what the context's own stream holds is waited for by an event;
//     and every later frame on another stream waits for the pass by the event behind it (SunMarks::ev), as it waits for ev_updated.
int order_pass(vrt_ctx *c, SunMarks &L, uint32_t k, hipStream_t st, bool shares) {
    if (k == 0u && (shares || c->shared_readers_in_flight)) {
        VRT_TRY(quiesce_before_frame(c));
        if (st != c->stream) {
            HIP_TRY(c, L.ev_guard.ensure());
            HIP_TRY(c, hipEventRecord(L.ev_guard, c->stream));
            HIP_TRY(c, hipStreamWaitEvent(st, L.ev_guard, 0));
        }
    }
    if (L.pending && L.stream != st) HIP_TRY(c, hipStreamWaitEvent(st, L.ev, 0));   // (a pass behind a pass)
    return VRT_OK;
}

// The cell pass, the voxel pass where it applies, and the event behind both; the marks are `now`'s from here on.
int launch_passes(vrt_ctx *c, Tables &T, const LitPlan &lp, const SunMarks::Key &now, hipStream_t st) {
    SunMarks &L = T.lit;
    const uint32_t G = c->accel_S * 8u;
    L.valid = L.voxels_valid = false;
    vrt::launch_accel_lit(T.d_grid, G, lp.axis, lp.up, lp.min_lo, now.sun, lit_slab_depth(c, G), st);
    HIP_TRY(c, hipGetLastError());
    // the voxel marks, behind the cell marks they hand over to: not where the reserved id could be a liquid (a liquid table that is
    // not a range below 255 covers it: ids above 255 are material 255), and not where their step budget leaves the marks no trips
    const uint32_t layers = lit_voxel_layers(c, G);
    L.clash_pending = false;
    if (layers && c->liquid_is_range && lit_voxel_budget(layers) < lp.trips && T.d_bricks.cap() >= 64u && L.clash_gen != T.gen) {
        HIP_TRY(c, L.d_pool.exactly(T.d_bricks.cap()));
        HIP_TRY(c, L.d_clash.once(1));
        HIP_TRY(c, L.h_clash.ensure((size_t)64));
        vrt::launch_accel_lit_voxels(T.d_grid, T.d_bricks, L.d_pool, (uint32_t)T.d_bricks.cap(), G, lp.axis, lp.up, now.sun, layers, L.d_clash, st);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(L.h_clash, L.d_clash, sizeof(uint32_t), hipMemcpyDeviceToHost, st));   // (pinned: nothing waits; ev is behind it)
        L.clash_pending = true;
        L.pool_gen = T.gen;
        L.voxels_valid = true;
        L.voxel_layers = layers;
        c->lit_voxel_passes += 1u;
    }
    const bool pool_made = L.voxels_valid;
    // the dark marks, behind the lit ones: on every air leaf the passes above left unlit, whatever the plan's smallest leaf is
    L.dark_valid = false;
    if (const uint32_t depth = dark_depth(c, G)) {
        HIP_TRY(c, L.d_floors.exactly(T.d_grid.cap()));
        vrt::launch_accel_dark(T.d_grid, T.d_bricks, (uint32_t)T.d_bricks.cap(), L.d_floors, G, lp.axis, lp.up, now.sun, depth, now.liquid, st);
        HIP_TRY(c, hipGetLastError());
        L.dark_valid = true;
        c->dark_passes += 1u;
    }
    // the dark voxel marks, into the pool this pass has just made, behind the dark cell marks they lean on: under the conditions of the
    // lit voxel pass (the liquids a range: kDarkVoxel is material 255, no liquid).  Where the dark pass did not run no leaf carries
    // kAirDark (accel_lit_kernel has cleared it): solid voxels alone close a corridor then, which is the rule with no dark cell
    L.dark_voxel_layers = 0u;
    if (const uint32_t layers = pool_made ? dark_voxel_layers(c, G) : 0u) {
        vrt::launch_accel_dark_voxels(T.d_grid, T.d_bricks, L.d_pool, (uint32_t)T.d_bricks.cap(), G, lp.axis, lp.up, now.sun, layers, c->liquid_mask, L.d_clash, st);
        HIP_TRY(c, hipGetLastError());
        L.dark_voxel_layers = layers;
        c->dark_voxel_passes += 1u;
    }
    HIP_TRY(c, L.ev.ensure());
    HIP_TRY(c, hipEventRecord(L.ev, st));
    L.pending = true;
    L.stream = st;
    L.valid = true;
    L.made = now;
    c->lit_passes += 1u;
    return VRT_OK;
}

// The held marks to the frame on `st`: its stops, and what the read-backs report of it (c->lit_last_*).
int hand_out(vrt_ctx *c, Tables &T, const LitPlan &lp, hipStream_t st, vrt::FrameParams &P) {
    SunMarks &L = T.lit;
    if (L.pending && L.stream != st) {   // the marks this frame reads were made on another stream
        if (hipEventQuery(L.ev) == hipSuccess) L.pending = false;
        else HIP_TRY(c, hipStreamWaitEvent(st, L.ev, 0));
    }
    P.shadow_below = vrt::kLitBelow;
    P.lit_trips = lp.trips;
    c->lit_last_min_leaf = lp.min_lo + 1u;
    c->lit_last_trips = lp.trips;
    c->dark_last_used = L.dark_valid;   // (the frame's threshold is kLitBelow: a dark leaf stops its shadow rays as a lit one does)
    if (L.clash_pending && hipEventQuery(L.ev) == hipSuccess) {   // the pass is over: did it meet the reserved id in a brick of the world?
        L.clash_pending = false;
        if (*reinterpret_cast<volatile uint32_t *>(L.h_clash.get())) { L.voxels_valid = false; L.clash_gen = T.gen; }   // the plain bricks from here on
    }
    if (L.voxels_valid && L.pool_fits(T.d_bricks.cap()) && lit_voxel_budget(L.voxel_layers) < lp.trips) {
        P.shadow_bricks = L.d_pool;
        P.lit_voxel_trips = lp.trips - lit_voxel_budget(L.voxel_layers);
        c->lit_last_voxel_layers = L.voxel_layers;
        c->lit_last_voxel_trips = P.lit_voxel_trips;
        c->dark_last_voxel_layers = L.dark_voxel_layers;
    }
    return VRT_OK;
}

// The sun marks of table set k for the sun at P.sun_local, made on `st` if the set does not hold them and what they are made from
// has stood still; the frame's stops are left as they are (none) when this world and sun get no marks, or none yet.
int ensure_sun_marks(vrt_ctx *c, uint32_t k, hipStream_t st, bool shares, vrt::FrameParams &P) {
    Tables &T = c->tabs[k];
    LitPlan lp{};
    if (!c->accel_ok || !T.live || !T.d_grid || !lit_plan(c->world.size, P.sun_local, &lp)) return VRT_OK;
    SunMarks::Key now{T.gen, {P.sun_local[0], P.sun_local[1], P.sun_local[2]}, lp.min_lo, {}};
    // (the dark marks' blockers, the cells' and the voxels', are solid voxels that are no liquid: another liquid set, other marks)
    if (dark_depth(c, c->accel_S * 8u) || (lit_voxel_layers(c, c->accel_S * 8u) && dark_voxel_layers(c, c->accel_S * 8u)))
        memcpy(now.liquid, c->liquid_mask, sizeof now.liquid);
    if (T.lit.valid && T.lit.made.same(now)) {
        T.lit.want_frames = 0u;   // (a sun that swings between two places must not collect its four frames one at a time)
    } else {
        if (!settled(T.lit, now)) return VRT_OK;
        VRT_TRY(order_pass(c, T.lit, k, st, shares));
        VRT_TRY(launch_passes(c, T, lp, now, st));
    }
    return hand_out(c, T, lp, st, P);
}

// What the two read-backs share once their arguments are checked: the table set the last frame used (c->last.tab), with the frames
// in flight and a pending pass waited for, and the G^3 cells of its grid.
int marks_of_last_frame(vrt_ctx *c, const char *who, std::vector<uint32_t> &cells) {
    if (!c->accel_ok || c->accel_dirty || !c->tabs[c->last.tab].live)
        return fail(c, VRT_ERR_STATE, "%s: the tables are not up to date (render a frame first)", who);
    HIP_TRY(c, hipSetDevice(c->device));
    QUIESCE(c);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    Tables &T = c->tabs[c->last.tab];   // the table set the last frame used
    if (T.lit.pending) { HIP_TRY(c, hipEventSynchronize(T.lit.ev)); T.lit.pending = false; }
    cells.resize((size_t)c->accel_S * c->accel_S * c->accel_S * 512u);
    return read_grid_cells(c, T.d_grid, cells.data());
}

}  // namespace

int sun_marks_for_frame(vrt_ctx *c, uint32_t tab, hipStream_t st, bool shares, vrt::FrameParams &P) {
    c->lit_last_min_leaf = c->lit_last_trips = c->lit_last_voxel_layers = c->lit_last_voxel_trips = 0u;
    c->dark_last_used = false;
    c->dark_last_voxel_layers = 0u;
    return c->sun_marks ? ensure_sun_marks(c, tab, st, shares, P) : VRT_OK;
}

extern "C" {

int vrt_get_sun_marks(vrt_ctx *c, uint32_t *passes, uint32_t *min_leaf, uint32_t *lit_trips, uint8_t *lit) {
    GRP_ROOT(c, vrt_get_sun_marks(d, passes, min_leaf, lit_trips, lit));
    if (!c) return VRT_ERR_INVALID_ARG;
    if (passes) *passes = c->lit_passes;
    if (min_leaf) *min_leaf = c->lit_last_min_leaf;
    if (lit_trips) *lit_trips = c->lit_last_trips;
    if (!lit) return VRT_OK;
    std::vector<uint32_t> cells;
    VRT_TRY(marks_of_last_frame(c, "vrt_get_sun_marks", cells));
    const bool held = c->tabs[c->last.tab].lit.holds(c->tabs[c->last.tab].gen);
    for (size_t i = 0; i < cells.size(); i++) lit[i] = (held && cells[i] >= vrt::kAirLeaf && !(cells[i] & (vrt::kAirUnlit | vrt::kAirDark))) ? 1u : 0u;
    return VRT_OK;
}

int vrt_get_dark_marks(vrt_ctx *c, uint32_t *passes, uint32_t *count, uint32_t *used, uint8_t *dark) {
    GRP_ROOT(c, vrt_get_dark_marks(d, passes, count, used, dark));
    if (!c) return VRT_ERR_INVALID_ARG;
    if (passes) *passes = c->dark_passes;
    if (used) *used = c->dark_last_used ? 1u : 0u;
    if (!count && !dark) return VRT_OK;
    std::vector<uint32_t> cells;
    VRT_TRY(marks_of_last_frame(c, "vrt_get_dark_marks", cells));
    const Tables &T = c->tabs[c->last.tab];
    const bool held = T.lit.holds(T.gen) && T.lit.dark_valid;
    uint32_t n = 0;
    for (size_t i = 0; i < cells.size(); i++) {
        const bool d = held && cells[i] >= vrt::kAirLeaf && (cells[i] & vrt::kAirDark);
        n += d ? 1u : 0u;
        if (dark) dark[i] = d ? 1u : 0u;
    }
    if (count) *count = n;
    return VRT_OK;
}

int vrt_read_lit_voxels(vrt_ctx *c, uint32_t *passes, uint32_t *layers, uint32_t *lit_trips, uint8_t *lit) {
    GRP_ROOT(c, vrt_read_lit_voxels(d, passes, layers, lit_trips, lit));
    if (!c) return VRT_ERR_INVALID_ARG;
    if (passes) *passes = c->lit_voxel_passes;
    if (layers) *layers = c->lit_last_voxel_layers;
    if (lit_trips) *lit_trips = c->lit_last_voxel_trips;
    if (!lit) return VRT_OK;
    std::vector<uint32_t> cells;
    VRT_TRY(marks_of_last_frame(c, "vrt_read_lit_voxels", cells));
    const Tables &T = c->tabs[c->last.tab];
    const size_t G = (size_t)c->accel_S * 8u, W = G * 4u;
    memset(lit, 0, W * W * W);
    // (the pool as the last pass left it, in use or not: where the world holds the reserved id in a brick it is a copy without a mark)
    if (!T.lit.pool_is_of(T.gen, T.d_bricks.cap())) return VRT_OK;
    std::vector<uint16_t> pool(T.lit.d_pool.cap());
    HIP_TRY(c, hipMemcpy(pool.data(), T.lit.d_pool, pool.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
    for (size_t z = 0; z < G; z++)
        for (size_t y = 0; y < G; y++)
            for (size_t x = 0; x < G; x++) {
                const uint32_t e = cells[(z * G + y) * G + x];
                const size_t at = e & 0x7FFFFFC0u;
                if (!vrt::is_split_entry(e) || at + 64u > pool.size()) continue;
                for (size_t u = 0; u < 64u; u++)
                    if ((uint32_t)(pool[at + u] >> 1) == vrt::kLitVoxel)
                        lit[((z * 4u + (u >> 4)) * W + (y * 4u + ((u >> 2) & 3u))) * W + (x * 4u + (u & 3u))] = 1u;
            }
    return VRT_OK;
}

int vrt_read_dark_voxels(vrt_ctx *c, uint32_t *passes, uint32_t *layers, uint8_t *dark) {
    GRP_ROOT(c, vrt_read_dark_voxels(d, passes, layers, dark));
    if (!c) return VRT_ERR_INVALID_ARG;
    if (passes) *passes = c->dark_voxel_passes;
    if (layers) *layers = c->dark_last_voxel_layers;
    if (!dark) return VRT_OK;
    std::vector<uint32_t> cells;
    VRT_TRY(marks_of_last_frame(c, "vrt_read_dark_voxels", cells));
    const Tables &T = c->tabs[c->last.tab];
    const size_t G = (size_t)c->accel_S * 8u, W = G * 4u;
    memset(dark, 0, W * W * W);
    if (!T.lit.pool_is_of(T.gen, T.d_bricks.cap())) return VRT_OK;
    // (a mark is kDarkVoxel in the pool where the world's own brick holds air: a world that holds the id itself has no mark there)
    std::vector<uint16_t> pool(T.lit.d_pool.cap()), plain(T.d_bricks.cap());
    HIP_TRY(c, hipMemcpy(pool.data(), T.lit.d_pool, pool.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(plain.data(), T.d_bricks, plain.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
    for (size_t z = 0; z < G; z++)
        for (size_t y = 0; y < G; y++)
            for (size_t x = 0; x < G; x++) {
                const uint32_t e = cells[(z * G + y) * G + x];
                const size_t at = e & 0x7FFFFFC0u;
                if (!vrt::is_split_entry(e) || at + 64u > pool.size()) continue;
                for (size_t u = 0; u < 64u; u++)
                    if ((uint32_t)(pool[at + u] >> 1) == vrt::kDarkVoxel && (plain[at + u] >> 1) == 0u)
                        dark[((z * 4u + (u >> 4)) * W + (y * 4u + ((u >> 2) & 3u))) * W + (x * 4u + (u & 3u))] = 1u;
            }
    return VRT_OK;
}

}  // extern "C"

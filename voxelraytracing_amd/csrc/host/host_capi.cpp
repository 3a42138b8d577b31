// host_capi.cpp — include/vrt_host.h over the C++ host mirror (world.hpp, graphics.hpp, worldgen.hpp, collide.hpp) and the
// arithmetic it shares with the kernels (../both/).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <atomic>
#include <system_error>
#include <thread>

#include "../../../include/vrt_host.h"
#include "../both/cast_dda.h"
#include "../both/column_top.h"
#include "../both/denoise_math.h"
#include "../both/lens_math.h"
#include "../both/haze_math.h"
#include "../both/refract_math.h"
#include "../both/shape_math.h"
#include "../both/tone_math.h"
#include "../both/water_math.h"
#include "collide.hpp"
#include "edit_check.hpp"
#include "graphics.hpp"
#include "materials.hpp"
#include "netmsg.hpp"
#include "regionfile.hpp"
#include "worldgen.hpp"

using namespace vrt;

struct vrth_world {
    ClientWorld w;
    vrth_world(ChunkPos c, uint32_t max_nodes, uint32_t size) : w(c, max_nodes, size) {}
};

static ChunkPos cp3(const int32_t p[3]) { return {p[0], p[1], p[2]}; }

// fn(i0, i1) over [0, n) in blocks of `block`, handed out to `threads` workers (<= 0: one per hardware thread, at most
// cap_threads), this thread among them; fn returns false to end its worker.
template <class Fn>
static void parallel_blocks(size_t n, size_t block, int threads, unsigned cap_threads, Fn fn) {
    unsigned nt = threads > 0 ? (unsigned)threads : std::min(cap_threads, std::max(1u, std::thread::hardware_concurrency()));
    nt = (unsigned)std::min<size_t>(nt, (n + block - 1) / block);
    std::atomic<size_t> next{0};
    auto work = [&]() {
        for (;;) {
            const size_t i0 = next.fetch_add(block);
            if (i0 >= n || !fn(i0, std::min(i0 + block, n))) return;
        }
    };
    std::vector<std::thread> pool;
    try {
        for (unsigned t = 1; t < nt; t++) pool.emplace_back(work);
    } catch (const std::system_error &) {
        // no more threads to be had: the ones that started (and this one) do the work
    }
    work();
    for (auto &t : pool) t.join();
}

extern "C" {

vrth_world *vrth_world_new(const int32_t center_chunk[3], uint32_t max_nodes, uint32_t size_in_chunks) {
    if (!center_chunk || max_nodes < 2 || size_in_chunks == 0) return nullptr;
    try {
        return new vrth_world(cp3(center_chunk), max_nodes, size_in_chunks);
    } catch (...) {
        return nullptr;
    }
}

void vrth_world_free(vrth_world *w) { delete w; }

int vrth_world_create_chunk(vrth_world *w, const int32_t chunk_pos[3], const uint16_t *nodes, uint32_t n, uint32_t *root_out) {
    SetVoxelErr err;
    const NodeAddr root = w->w.create_chunk(cp3(chunk_pos), reinterpret_cast<const Node *>(nodes), n, err);
    if (root_out) *root_out = root;
    return (int)err;
}

int vrth_world_set_voxel(vrth_world *w, const int32_t p[3], uint16_t voxel, uint32_t *range_start, uint32_t *range_len) {
    // GameState::set_voxel (client/src/lib.rs:67-76): NoChange short-circuit, then ClientWorld::set_voxel
    Voxel cur;
    if (auto e = w->w.get_voxel(cp3(p), cur); e != SetVoxelErr::Ok) return (int)e;
    if (cur == Voxel(voxel)) return (int)SetVoxelErr::NoChange;
    const Chunk *c = nullptr;
    const SetVoxelErr e = w->w.set_voxel(cp3(p), Voxel(voxel), &c);
    if ((e == SetVoxelErr::Ok || e == SetVoxelErr::OutOfMemory) && c) {  // OutOfMemory: the partial split is in the pool
        if (range_start) *range_start = c->range.start;
        if (range_len) *range_len = c->range.len();
    }
    return (int)e;
}

int vrth_world_get_voxel(const vrth_world *w, const int32_t p[3], uint16_t *voxel_out) {
    Voxel v;
    const SetVoxelErr e = w->w.get_voxel(cp3(p), v);
    if (e == SetVoxelErr::Ok && voxel_out) *voxel_out = v.as_data();
    return (int)e;
}

// common::math::cast_ray from ../both/cast_dda.h's parts (the text the GPU's cast compiles too) with the client's collides
// (clientdesktop/src/main.rs:320-325).  This file is built with -ffp-contract=off (Makefile).
int vrth_world_cast_ray(const vrth_world *w, const float start[3], const float dir[3], float max_dist, vrt_ray_hit *out) {
    vrt_ray_hit r;
    memset(&r, 0, sizeof r);
    if (cast_rejected(start, max_dist)) {
        r.status = VRT_RAY_REJECTED;
    } else {
        const VoxelPos lo = w->w.min_voxel();
        const int32_t lo3[3] = {lo.x, lo.y, lo.z};
        CastDda d = cast_setup(start, dir);
        float dist = 0.0f;
        while (dist < max_dist) {
            const int32_t px = d.mx, py = d.my, pz = d.mz;
            dist = cast_step(d);
            Voxel v;
            const bool in_world = w->w.get_voxel(VoxelPos{d.mx, d.my, d.mz}, v) == SetVoxelErr::Ok;
            if (in_world && !v.is_empty()) {
                cast_hit(r, d, px, py, pz, dist);
                r.status = VRT_RAY_HIT;
                break;
            }
            if (!in_world && cast_gone(d, lo3, w->w.size_in_voxels())) break;   // (an Err is also a missing chunk: cast_gone says no inside)
        }
    }
    if (out) *out = r;
    return (int)r.status;
}

void vrth_world_cast_rays(const vrth_world *w, const vrt_ray_query *q, uint32_t n, vrt_ray_hit *out, int threads) {
    if (!w || !q || !out || !n) return;
    parallel_blocks(n, 1024, threads, ~0u, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) vrth_world_cast_ray(w, q[i].start, q[i].dir, q[i].max_dist, &out[i]);
        return true;
    });
}

uint32_t vrth_world_center_chunks(vrth_world *w, const int32_t anchor_chunk[3]) {
    std::vector<std::pair<ChunkPos, Chunk>> removed;
    w->w.center_chunks(cp3(anchor_chunk), removed);
    for (auto &rc : removed) w->w.free_chunk(rc.second);
    return (uint32_t)removed.size();
}

void vrth_world_resize(vrth_world *w, uint32_t size_in_chunks) { w->w.resize(size_in_chunks); }

const uint16_t *vrth_world_nodes(const vrth_world *w) { return reinterpret_cast<const uint16_t *>(w->w.nodes()); }
uint32_t vrth_world_max_nodes(const vrth_world *w) { return w->w.max_nodes(); }

uint32_t vrth_world_chunk_roots(const vrth_world *w, uint32_t *out, uint32_t cap) {
    if (!out) return (uint32_t)w->w.chunk_count();
    const std::vector<NodeAddr> &r = w->w.chunk_roots();
    std::copy_n(r.begin(), std::min<size_t>(cap, r.size()), out);
    return (uint32_t)r.size();
}

const uint32_t *vrth_world_chunk_roots_ptr(const vrth_world *w) { return w->w.chunk_roots().data(); }
uint64_t vrth_world_chunk_roots_generation(const vrth_world *w) { return w->w.roots_generation(); }

void vrth_world_info(const vrth_world *w, int32_t min_voxel[3], uint32_t *size_in_voxels, uint32_t *size_in_chunks, uint32_t *populated) {
    const VoxelPos m = w->w.min_voxel();
    if (min_voxel) { min_voxel[0] = m.x; min_voxel[1] = m.y; min_voxel[2] = m.z; }
    if (size_in_voxels) *size_in_voxels = w->w.size_in_voxels();
    if (size_in_chunks) *size_in_chunks = w->w.size_in_chunks();
    if (populated) *populated = (uint32_t)w->w.populated_count();
}

void vrth_world_alloc_status(const vrth_world *w, uint32_t *free_nodes, uint32_t *max_nodes) {
    const auto s = w->w.chunk_alloc_status();
    if (free_nodes) *free_nodes = s.first;
    if (max_nodes) *max_nodes = s.second;
}

int vrth_world_chunk_state(const vrth_world *w, const int32_t chunk_pos[3], uint32_t *range_start, uint32_t *range_end,
                           uint32_t *last_used_addr, uint32_t *spans, uint32_t cap_spans) {
    const Chunk *c = w->w.get_chunk(cp3(chunk_pos));
    if (!c) return -1;
    if (range_start) *range_start = c->range.start;
    if (range_end) *range_end = c->range.end;
    if (last_used_addr) *last_used_addr = c->alloc.last_used_addr;
    const auto &fm = c->alloc.free_mem;
    for (size_t i = 0; i < fm.size() && i < cap_spans; i++) {
        spans[2 * i] = fm[i].start;
        spans[2 * i + 1] = fm[i].end;
    }
    return (int)fm.size();
}

// ---- collisions (collide.hpp) ----
int vrth_world_get_collisions(const vrth_world *w, const float from[3], const float to[3], const vrt_material *mats256, int32_t *out_xyz,
                              uint32_t cap, uint32_t *n) {
    if (n) *n = 0;
    if (!w || !from || !to || !mats256) return -1;
    for (int a = 0; a < 3; a++)
        if (!clip_in_range(from[a]) || !clip_in_range(to[a])) return -1;
    const Aabb bb{{from[0], from[1], from[2]}, {to[0], to[1], to[2]}};
    if (collisions_over_cap(bb)) return -1;
    const std::vector<VoxelPos> v = get_collisions_w(w->w, bb, mats256);
    for (size_t i = 0; i < v.size() && i < cap && out_xyz; i++) {
        out_xyz[3 * i] = v[i].x; out_xyz[3 * i + 1] = v[i].y; out_xyz[3 * i + 2] = v[i].z;
    }
    if (n) *n = (uint32_t)v.size();
    return 0;
}

int vrth_world_clip_move(const vrth_world *w, const vrt_material *mats256, const vrt_box_query *q, vrt_box_move *out) {
    vrt_box_move r;
    clip_aabb_movement(w->w, mats256, *q, r);
    if (out) *out = r;
    return (int)r.status;
}

void vrth_world_clip_moves(const vrth_world *w, const vrt_material *mats256, const vrt_box_query *q, uint32_t n, vrt_box_move *out, int threads) {
    if (!w || !mats256 || !q || !out || !n) return;
    parallel_blocks(n, 1024, threads, ~0u, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) clip_aabb_movement(w->w, mats256, q[i], out[i]);
        return true;
    });
}

int vrth_world_highest_vox_at(const vrth_world *w, int32_t x, int32_t z, int32_t *y_out) {
    const auto y = w->w.highest_vox_at({x, 0, z});
    if (!y) return 0;
    if (y_out) *y_out = *y;
    return 1;
}

// ---- column tops (../both/column_top.h): highest_vox_at's loop, every voxel of the column through get_voxel ----
// One column against a solid set made once (solid_set); the x / z test is include/vrt.h's box, not check_bounds' (whose far
// faces lie 31 voxels further out, where get_voxel then finds no chunk)
static void column_top(const ClientWorld &w, const uint32_t solid[8], const vrt_column_query &q, vrt_column_top &r) {
    const VoxelPos lo = w.min_voxel();
    const uint32_t W = w.size_in_voxels();
    const uint32_t ux = (uint32_t)q.x - (uint32_t)lo.x, uz = (uint32_t)q.z - (uint32_t)lo.z;
    if (!(ux < W && uz < W)) {
        column_outside(r);
        return;
    }
    uint32_t uy;
    if (column_start(q.flags, q.from_y, lo.y, W, uy)) {
        for (;; uy--) {
            Voxel v;   // get_voxel(pos) or Voxel::EMPTY
            if (w.get_voxel(VoxelPos{q.x, (int32_t)((uint32_t)lo.y + uy), q.z}, v) != SetVoxelErr::Ok) v = Voxel();
            if (column_counts(v.as_data(), q.flags, solid)) {
                column_found(r, lo.y, uy, v.as_data());
                return;
            }
            if (uy == 0u) break;
        }
    }
    column_none(r, lo.y);
}

// get_voxel as vrt_get_voxels records it: include/vrt.h's box first (see above), then ClientWorld::get_voxel's own answer
void vrth_world_get_voxels(const vrth_world *w, const int32_t *pos, uint32_t n, vrt_voxel_at *out, int threads) {
    if (!w || !pos || !out || !n) return;
    const VoxelPos lo = w->w.min_voxel();
    const uint32_t W = w->w.size_in_voxels();
    parallel_blocks(n, 4096, threads, ~0u, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) {
            const int32_t *p = pos + 3 * i;
            vrt_voxel_at r{0, (uint16_t)VRT_VOXEL_OUT_OF_BOUNDS};
            if ((uint32_t)p[0] - (uint32_t)lo.x < W && (uint32_t)p[1] - (uint32_t)lo.y < W && (uint32_t)p[2] - (uint32_t)lo.z < W) {
                Voxel v;
                r.status = (uint16_t)w->w.get_voxel(VoxelPos{p[0], p[1], p[2]}, v);
                r.voxel = r.status == VRT_VOXEL_OK ? v.as_data() : (uint16_t)0;
            }
            out[i] = r;
        }
        return true;
    });
}

int vrth_world_column_top(const vrth_world *w, const vrt_material *mats256, const vrt_column_query *q, vrt_column_top *out) {
    if (!w || !q || !out) return -1;
    uint32_t solid[8];
    solid_set(mats256, solid);
    column_top(w->w, solid, *q, *out);
    return (int)out->status;
}

void vrth_world_column_tops(const vrth_world *w, const vrt_material *mats256, const vrt_column_query *q, uint32_t n, vrt_column_top *out,
                            int threads) {
    if (!w || !q || !out || !n) return;
    uint32_t solid[8];
    solid_set(mats256, solid);
    parallel_blocks(n, 1024, threads, ~0u, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) column_top(w->w, solid, q[i], out[i]);
        return true;
    });
}

int vrth_world_top_map(const vrth_world *w, const vrt_material *mats256, uint32_t flags, vrt_top_entry *map, int threads) {
    if (!w || !map || (flags & ~VRT_COLUMN_SOLID)) return -1;
    uint32_t solid[8];
    solid_set(mats256, solid);
    const VoxelPos lo = w->w.min_voxel();
    const size_t W = w->w.size_in_voxels();
    parallel_blocks(W * W, 256, threads, ~0u, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) {
            const vrt_column_query q{(int32_t)((uint32_t)lo.x + (uint32_t)(i % W)), (int32_t)((uint32_t)lo.z + (uint32_t)(i / W)), 0, flags};
            vrt_column_top r;
            column_top(w->w, solid, q, r);
            map[i].y = r.y;
            map[i].voxel = r.voxel;
        }
        return true;
    });
    return 0;
}

void vrth_world_data_from(const vrth_world *w, vrt_world_data *out) { *out = WorldData::from(w->w); }

void vrth_cam_data_create(const float rot_deg[3], const float eye[3], float fov_deg, const float proj_size[2], vrt_cam_data *out) {
    *out = CamData::create({rot_deg[0], rot_deg[1], rot_deg[2]}, {eye[0], eye[1], eye[2]}, fov_deg, {proj_size[0], proj_size[1]});
}

void vrth_axis_rot_to_ray(const float rot_rad[3], float out[3]) {
    const float r = std::cos(rot_rad[0]);
    out[0] = r * -std::sin(rot_rad[1]);
    out[2] = r * -std::cos(rot_rad[1]);
    out[1] = -std::sin(rot_rad[0]);
}

void vrth_std_materials(vrt_material *out256) {
    std::memset(out256, 0, 256 * sizeof(vrt_material));  // Material::ZERO for unnamed slots
    for (int i = 0; i < kStdVoxelCount; i++) {
        out256[i].color[0] = kStdVoxels[i].r;
        out256[i].color[1] = kStdVoxels[i].g;
        out256[i].color[2] = kStdVoxels[i].b;
        out256[i].is_empty = kStdVoxels[i].is_empty;
        out256[i].is_liquid = kStdVoxels[i].is_liquid;
        out256[i].scatter = 0.0f;
    }
}

const char *vrth_std_voxel_name(uint32_t id) { return id < (uint32_t)kStdVoxelCount ? kStdVoxels[id].name : nullptr; }

uint32_t vrth_svo_build_by_set_node(const uint16_t *dense, uint16_t *nodes, uint32_t cap) {
    return build_svo_by_set_node(dense, reinterpret_cast<Node *>(nodes), cap);
}

uint32_t vrth_svo_build_bottom_up(const uint16_t *dense, uint16_t *nodes, uint32_t cap) {
    std::vector<Node> out;
    if (!build_svo_bottom_up(dense, out) || out.size() > cap) return 0;
    std::memcpy(nodes, out.data(), out.size() * sizeof(Node));
    return (uint32_t)out.size();
}

void vrth_svo_to_dense(const uint16_t *nodes, uint16_t *dense) {
    const Node *n = reinterpret_cast<const Node *>(nodes);
    const Svo svo{0, CHUNK_SIZE};
    for (uint32_t z = 0; z < 32; z++)
        for (uint32_t y = 0; y < 32; y++)
            for (uint32_t x = 0; x < 32; x++) dense[x + 32 * (y + 32 * z)] = n[svo.find_node(n, {x, y, z}, CHUNK_DEPTH).idx].voxel().as_data();
}

int32_t vrth_gen_height(uint32_t seed, int32_t x, int32_t z) {
    WorldGen g;
    g.seed = seed;
    return g.height(x, z);
}

int vrth_gen_dense(uint32_t seed, const int32_t chunk_pos[3], uint16_t *dense) {
    WorldGen g;
    g.seed = seed;
    return g.fill_dense(cp3(chunk_pos), dense) ? 1 : 0;
}

void vrth_gen_dense_superflat(const int32_t chunk_pos[3], uint16_t *dense) { fill_dense_superflat(cp3(chunk_pos), dense); }

// Shared by vrth_world_generate (every cell of the grid) and vrth_world_generate_missing (the empty cells only: what the
// server sends back for request_missing_chunks, client/src/lib.rs:80-108, after the grid moved).  `ranges`: (root, count)
// of every chunk created, in grid order — the ranges GameState::process_cmd hands to NodeBuffer::write (main.rs:289-295).
static int generate_impl(vrth_world *w, uint32_t kind, uint32_t seed, int threads, bool only_missing, uint32_t *ranges, uint32_t cap,
                         uint32_t *n_ranges) {
    const uint32_t S = w->w.size_in_chunks();
    const size_t total = (size_t)S * S * S;
    std::vector<std::vector<Node>> built(total);
    std::vector<uint8_t> skip(total, 0);
    if (only_missing) {
        const ChunkPos mn0 = w->w.min_chunk();
        for (size_t i = 0; i < total; i++) {
            const ChunkPos cp{mn0.x + (int32_t)(i % S), mn0.y + (int32_t)((i / S) % S), mn0.z + (int32_t)(i / ((size_t)S * S))};
            skip[i] = w->w.get_chunk(cp) != nullptr;
        }
    }
    std::atomic<int> failed{0};
    WorldGen g;
    g.seed = seed;
    const ChunkPos mn = w->w.min_chunk();
    // (at most 16 workers unless asked for more: a chunk is ~0.1 ms of work, and a host with hundreds of hardware threads —
    // or a limit on tasks per process — gains nothing from one thread per core here)
    parallel_blocks(total, 1, threads, 16u, [&](size_t i, size_t) {
        thread_local std::vector<uint16_t> dense(32768);   // one pair of buffers per worker, not per chunk
        thread_local std::vector<Node> scratch(NODES_PER_CHUNK + 64);
        if (skip[i]) return true;
        const ChunkPos cp{mn.x + (int32_t)(i % S), mn.y + (int32_t)((i / S) % S), mn.z + (int32_t)(i / ((size_t)S * S))};
        if (kind == 1) {
            fill_dense_superflat(cp, dense.data());
            // C1 is built the reference's way (set_node, x -> z -> y), holes and all
            const uint32_t used = build_svo_by_set_node(dense.data(), scratch.data(), (uint32_t)scratch.size());
            if (!used) { failed = (int)SetVoxelErr::OutOfMemory; return false; }
            built[i].assign(scratch.begin(), scratch.begin() + used);
        } else {
            const bool uniform = g.fill_dense(cp, dense.data());
            if (uniform) built[i].assign(1, Node::make(Voxel(dense[0])));
            else if (!build_svo_bottom_up(dense.data(), built[i])) { failed = (int)SetVoxelErr::OutOfMemory; return false; }
        }
        return true;
    });
    if (failed) return failed;
    // create_chunk in grid order (x fastest), so pool layout is deterministic regardless of threads
    uint32_t count = 0;
    for (size_t i = 0; i < total; i++) {
        const ChunkPos cp{mn.x + (int32_t)(i % S), mn.y + (int32_t)((i / S) % S), mn.z + (int32_t)(i / ((size_t)S * S))};
        // an all-air chunk needs no storage: leaving the cell empty resolves to pool[0] (world.rs:154-159)
        if (skip[i] || (built[i].size() == 1 && built[i][0].w == 0)) continue;
        SetVoxelErr err;
        const NodeAddr root = w->w.create_chunk(cp, built[i].data(), (uint32_t)built[i].size(), err);
        if (err != SetVoxelErr::Ok) return (int)err;
        if (ranges && count < cap) { ranges[2 * count] = root; ranges[2 * count + 1] = (uint32_t)built[i].size(); }
        count++;
    }
    if (n_ranges) *n_ranges = count;
    return 0;
}

int vrth_world_generate(vrth_world *w, uint32_t kind, uint32_t seed, int threads) {
    return generate_impl(w, kind, seed, threads, false, nullptr, 0, nullptr);
}

int vrth_world_generate_missing(vrth_world *w, uint32_t kind, uint32_t seed, int threads, uint32_t *ranges, uint32_t cap, uint32_t *n_ranges) {
    return generate_impl(w, kind, seed, threads, true, ranges, cap, n_ranges);
}

// The other half of generate_impl, for nodes built elsewhere (vrt_generate_chunks): create_chunk in the order given, all-air
// chunks skipped, ranges as above.  A refused chunk (an empty range) fails the whole call first, as generate_impl's builder does.
int vrth_world_create_chunks(vrth_world *w, const int32_t *chunk_pos, uint32_t n, const uint16_t *nodes, const uint64_t *offsets,
                             uint32_t *ranges, uint32_t cap, uint32_t *n_ranges) {
    if (n_ranges) *n_ranges = 0;
    if (n == 0) return 0;
    for (uint32_t i = 0; i < n; i++)
        if (offsets[i + 1] <= offsets[i]) return (int)SetVoxelErr::OutOfMemory;
    const Node *src = reinterpret_cast<const Node *>(nodes);
    uint32_t count = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t cnt = offsets[i + 1] - offsets[i];
        const Node *c = src + offsets[i];
        if (cnt == 1 && c[0].w == 0) continue;
        if (cnt > 0xFFFFFFFFull) return (int)SetVoxelErr::BadChunkData;
        SetVoxelErr err;
        const NodeAddr root = w->w.create_chunk(cp3(chunk_pos + 3ull * i), c, (uint32_t)cnt, err);
        if (err != SetVoxelErr::Ok) return (int)err;
        if (ranges && count < cap) { ranges[2 * count] = root; ranges[2 * count + 1] = (uint32_t)cnt; }
        count++;
    }
    if (n_ranges) *n_ranges = count;
    return 0;
}


// ---- feature shapes (include/vrt.h vrt_edit_chunks): the specification of vrt_edit.hip's kernels ----

// One shape onto the block of the chunk whose first voxel is (x0, y0, z0): BuiltFeature's placements (gen.rs:312-354) that lie
// in the chunk, from ../both/shape_math.h's parts
static void apply_shape(uint16_t *dense, int32_t x0, int32_t y0, int32_t z0, const vrt_shape &s) {
    const uint16_t v = (uint16_t)s.voxel;
    auto put = [&](int32_t x, int32_t y, int32_t z) {
        const uint32_t lx = (uint32_t)(x - x0), ly = (uint32_t)(y - y0), lz = (uint32_t)(z - z0);
        if (lx < 32u && ly < 32u && lz < 32u) dense[lx + 32u * (ly + 32u * lz)] = v;
    };
    if (s.kind == kShapePoint) {
        put(s.a[0], s.a[1], s.a[2]);
    } else if (s.kind == kShapeLine) {
        LineWalk w = line_begin(s);
        do put(w.x, w.y, w.z);
        while (line_next(w));
    } else {
        ShapeBox bx = shape_box(s);
        if (!shape_box_clip(bx, x0, y0, z0)) return;
        const float r2 = s.r * s.r;
        for (int32_t z = bx.lo[2]; z <= bx.hi[2]; z++)
            for (int32_t y = bx.lo[1]; y <= bx.hi[1]; y++)
                for (int32_t x = bx.lo[0]; x <= bx.hi[0]; x++)
                    if (shape_within(s.a[0], s.a[1], s.a[2], r2, x, y, z)) put(x, y, z);
    }
}

static int edit_status(EditFault f) { return f == EditFault::None ? VRT_OK : edit_fault_is_range(f) ? VRT_ERR_OUT_OF_RANGE : VRT_ERR_INVALID_ARG; }

int vrth_apply_shapes(uint16_t *dense, const int32_t chunk_pos[3], const vrt_shape *shapes, uint32_t m) {
    if (!dense || !chunk_pos) return VRT_ERR_INVALID_ARG;
    // (the checks of a call with this one chunk, as an all-air tree)
    const uint16_t air = 0;
    const uint64_t offs[2] = {0, 1};
    uint64_t out_offs[2] = {0, 0}, index;
    uint8_t changed = 0;
    EditBins bins;
    if (const EditFault f = edit_check(chunk_pos, 1, &air, offs, shapes, m, nullptr, 0, out_offs, &changed, bins, &index); f != EditFault::None)
        return edit_status(f);
    for (uint16_t j : bins.list) apply_shape(dense, chunk_pos[0] * 32, chunk_pos[1] * 32, chunk_pos[2] * 32, shapes[j]);
    return VRT_OK;
}

int vrth_edit_chunks(const int32_t *chunk_pos, uint32_t n, const uint16_t *nodes_in, const uint64_t *offsets_in, const vrt_shape *shapes,
                     uint32_t m, uint16_t *nodes_out, uint64_t cap_nodes, uint64_t *offsets_out, uint8_t *changed, int threads) {
    EditBins bins;
    uint64_t index;
    if (const EditFault f = edit_check(chunk_pos, n, nodes_in, offsets_in, shapes, m, nodes_out, cap_nodes, offsets_out, changed, bins, &index);
        f != EditFault::None)
        return edit_status(f);
    offsets_out[0] = 0;
    if (n == 0) return VRT_OK;
    std::vector<std::vector<Node>> built(n);
    parallel_blocks(n, 1, threads, 16u, [&](size_t i, size_t) {
        thread_local std::vector<uint16_t> before(32768), dense(32768);
        vrth_svo_to_dense(nodes_in + offsets_in[i], before.data());
        dense = before;
        const int32_t *p = chunk_pos + 3 * i;
        for (uint32_t k = bins.start[i]; k < bins.start[i + 1]; k++) apply_shape(dense.data(), p[0] * 32, p[1] * 32, p[2] * 32, shapes[bins.list[k]]);
        changed[i] = dense != before;
        if (!build_svo_bottom_up(dense.data(), built[i])) built[i].clear();   // refused: an empty range
        return true;
    });
    // the outputs, as vrt_build_chunks leaves them
    uint32_t refused = 0;
    for (uint32_t i = 0; i < n; i++) {
        offsets_out[i + 1] = offsets_out[i] + built[i].size();
        refused += built[i].empty();
    }
    if (offsets_out[n] > cap_nodes) return VRT_ERR_OOM;
    for (uint32_t i = 0; i < n; i++)
        if (!built[i].empty()) std::memcpy(nodes_out + offsets_out[i], built[i].data(), built[i].size() * sizeof(Node));
    return refused ? VRT_ERR_OUT_OF_RANGE : VRT_OK;
}

// ---- region files (servercli/src/main.rs:25-73) ----

int vrth_region_load_into_world(vrth_world *w, const uint8_t *bytes, uint64_t n, const int32_t region_pos[3], uint32_t *chunks_loaded) {
    auto rf = RegionFile::from_file(bytes, (size_t)n);
    if (!rf) return -1;
    uint32_t loaded = 0;
    for (auto &kv : rf->chunks) {
        uint32_t cn = 0;
        const Node *nodes = rf->read_chunk_data(kv.first, cn);
        if (!nodes) return -1;
        const ChunkPos cp{region_pos[0] * (int32_t)REGION_SIZE + (int32_t)kv.first[0], region_pos[1] * (int32_t)REGION_SIZE + (int32_t)kv.first[1],
                          region_pos[2] * (int32_t)REGION_SIZE + (int32_t)kv.first[2]};
        SetVoxelErr err;
        w->w.create_chunk(cp, nodes, cn, err);
        if (err == SetVoxelErr::PosOutOfBounds) continue;  // outside the client's grid, like received_oob_chunks (lib.rs:116)
        if (err != SetVoxelErr::Ok) return (int)err;
        loaded++;
    }
    if (chunks_loaded) *chunks_loaded = loaded;
    return 0;
}

uint64_t vrth_region_save_from_world(const vrth_world *w, const int32_t region_pos[3], uint8_t *out, uint64_t cap) {
    RegionFile rf;
    const int32_t r = (int32_t)REGION_SIZE;
    for (int32_t z = 0; z < r; z++)
        for (int32_t y = 0; y < r; y++)
            for (int32_t x = 0; x < r; x++) {
                const ChunkPos cp{region_pos[0] * r + x, region_pos[1] * r + y, region_pos[2] * r + z};
                const Chunk *c = w->w.get_chunk(cp);
                if (!c) continue;
                // what the server stores per chunk is its used node prefix (ServerChunk::used_nodes, server/src/world/mod.rs:109-112)
                rf.append_chunk({(uint32_t)x, (uint32_t)y, (uint32_t)z}, w->w.nodes() + c->range.start, c->alloc.last_used_addr + 1);
            }
    const std::vector<uint8_t> bytes = rf.to_file();
    if (out && bytes.size() <= cap) std::memcpy(out, bytes.data(), bytes.size());
    return bytes.size();
}

void vrth_region_of_chunk(const int32_t chunk_pos[3], int32_t region_pos[3], uint32_t pos_in_region[3]) {
    const auto rp = chunk_region(cp3(chunk_pos));
    region_pos[0] = rp.first.x; region_pos[1] = rp.first.y; region_pos[2] = rp.first.z;
    for (int i = 0; i < 3; i++) pos_in_region[i] = rp.second[i];
}

uint32_t vrth_region_file_name(const int32_t region_pos[3], char *out, uint32_t cap) {
    const std::string s = region_file_name(cp3(region_pos));
    if (out && cap > s.size()) std::memcpy(out, s.c_str(), s.size() + 1);
    return (uint32_t)s.size();
}

int vrth_chunk_msg_ingest(vrth_world *w, const uint8_t *bytes, uint64_t n, uint64_t *consumed, int32_t chunk_pos[3], uint32_t *root,
                          uint32_t *node_count) {
    GiveChunkData m;
    size_t used = 0;
    switch (GiveChunkData::decode(bytes, (size_t)n, m, used)) {
        case GiveChunkData::Status::NeedMore: return -2;
        case GiveChunkData::Status::NotChunkData: return -3;
        case GiveChunkData::Status::Malformed: return -1;
        case GiveChunkData::Status::Ok: break;
    }
    if (consumed) *consumed = used;
    if (chunk_pos) { chunk_pos[0] = m.pos.x; chunk_pos[1] = m.pos.y; chunk_pos[2] = m.pos.z; }
    // GameState::process_cmd, client/src/lib.rs:112-118
    SetVoxelErr err;
    const NodeAddr addr = w->w.create_chunk(m.pos, m.nodes.data(), (uint32_t)m.nodes.size(), err);
    if (root) *root = addr;
    if (node_count) *node_count = (uint32_t)m.nodes.size();
    return (int)err;
}

uint64_t vrth_chunk_msg_encode(const vrth_world *w, const int32_t chunk_pos[3], uint8_t *out, uint64_t cap) {
    const Chunk *c = w->w.get_chunk(cp3(chunk_pos));
    if (!c) return 0;
    // server/src/lib.rs:229-233, 292-296: GiveChunkData(pos, Cow::Borrowed(chunk.used_nodes()), NodeAlloc::new(0..1, 1..2))
    // — the allocator field is a placeholder on the wire; the client rebuilds its own (world.rs:323)
    GiveChunkData m;
    m.pos = cp3(chunk_pos);
    const uint32_t used = c->alloc.last_used_addr + 1;
    m.nodes.assign(w->w.nodes() + c->range.start, w->w.nodes() + c->range.start + used);
    m.range = {0, 2};
    m.free_mem = {NodeRange{1, 2}};
    m.last_used_addr = 0;
    const std::vector<uint8_t> bytes = m.encode();
    if (out && bytes.size() <= cap) std::memcpy(out, bytes.data(), bytes.size());
    return bytes.size();
}

// vrt_set_denoise's filter over host arrays: csrc/both/denoise_math.h's pixel, pass after pass between two copies of the frame
int vrth_denoise(const float *rgb, const uint32_t *ids, const uint32_t *guide, uint32_t w, uint32_t h, const vrt_denoise_opts *opts, float *out) {
    if (!rgb || !ids || !guide || !out) return -1;
    const uint32_t passes = opts ? opts->passes : 0u;
    const float sigma = opts ? opts->sigma_color : 0.0f;
    if (opts && (passes > vrt::kDnMaxPasses || !(sigma >= 0.0f) || std::isinf(sigma) || opts->flags || opts->_reserved)) return -1;
    const size_t n = (size_t)w * h;
    std::vector<float> a(rgb, rgb + n * 3), b(a);
    const int wt = (int)(w & ~7u), ht = (int)(h & ~7u);
    for (uint32_t i = 0; i < passes; i++) {
        const int s = 1 << i;
        const bool stop = sigma != 0.0f;
        const float sg2 = vrt::denoise_sigma2(sigma, i);
        for (int y = 0; y < ht; y++)
            for (int x = 0; x < wt; x++) {
                const size_t p = (size_t)y * w + x;
                if (!vrt::denoise_filterable(ids[p])) continue;   // (copied)
                const uint32_t key = vrt::denoise_key(ids[p]), g = guide[p];
                auto fetch = [&](int qx, int qy, vrt::DnColor &c) {
                    if (qx < 0 || qy < 0 || qx >= wt || qy >= ht) return false;
                    const size_t q = (size_t)qy * w + qx;
                    if (vrt::denoise_key(ids[q]) != key || guide[q] != g) return false;
                    c = vrt::DnColor{a[q * 3], a[q * 3 + 1], a[q * 3 + 2]};
                    return true;
                };
                const vrt::DnColor o = vrt::denoise_pixel(fetch, x, y, s, vrt::DnColor{a[p * 3], a[p * 3 + 1], a[p * 3 + 2]}, stop, sg2);
                b[p * 3] = o.r; b[p * 3 + 1] = o.g; b[p * 3 + 2] = o.b;
            }
        a.swap(b);   // (the pixels a pass copies never change: both copies hold them from the start)
    }
    std::memcpy(out, a.data(), n * 3 * sizeof(float));
    return 0;
}

// vrt_set_camera_sampling's primary ray of one sample: csrc/both/lens_math.h's two halves with the plain operators, and the
// normalisation between them as orc_normalize / vnormalize write it
int vrth_lens_ray(const vrt_cam_data *cam, const int32_t world_min[3], const vrt_camera_sampling *opts, uint32_t px, uint32_t py, const float u[4],
                  float out[9]) {
    if (!cam || !world_min || !opts || !u || !out) return -1;
    auto div = [](float n, float d) { return n / d; };
    auto sqrt_of = [](float x) { return sqrtf(x); };
    const vrt::LensV3 w = vrt::lens_pixel_dir(px, py, u[0], u[1], opts->pixel_spread, cam->proj_size, cam->inv_proj_mat, cam->inv_view_mat, div);
    const vrt::LensV3 origin{cam->pos[0] - (float)world_min[0], cam->pos[1] - (float)world_min[1], cam->pos[2] - (float)world_min[2]};
    vrt::LensV3 o = origin, v = w;
    if (opts->aperture != 0.0f) {
        const float len = sqrtf(w.x * w.x + w.y * w.y + w.z * w.z);
        const vrt::LensV3 d{w.x / len, w.y / len, w.z / len};
        vrt::lens_thin(origin, d, u[2], u[3], opts->aperture, opts->focus_distance, cam->inv_view_mat, sqrt_of, o, v);
    }
    const float r[9] = {w.x, w.y, w.z, o.x, o.y, o.z, v.x, v.y, v.z};
    std::memcpy(out, r, sizeof r);
    return 0;
}

// vrt_set_tone_map's metering over a host frame: csrc/both/tone_math.h's bin per pixel of the traced area, then its one-thread
// step over the bins' prefix sums, found here in a plain loop
int vrth_tone_meter(const float *rgb, uint32_t w, uint32_t h, const vrt_tone_map *opts, int has_prev, float prev_exposure, vrt_tone_info *info,
                    uint32_t bins[256]) {
    if (!rgb || !opts) return -1;
    vrt_tone_map o = *opts;
    if (!vrt::tone_setting_ok(o)) return -1;
    o.flags |= vrt::kToneAuto;   // (what is metered is held to the metering's ranges)
    if (o.curve == vrt::kToneOff) o.curve = vrt::kToneLinear;
    if (!vrt::tone_setting_ok(o)) return -1;
    uint32_t count[vrt::kToneBins] = {};
    const uint32_t wt = w & ~7u, ht = h & ~7u;
    for (uint32_t y = 0; y < ht; y++)
        for (uint32_t x = 0; x < wt; x++) {
            const float *p = rgb + ((size_t)y * w + x) * 3;
            const int b = vrt::tone_bin(vrt::tone_luminance(p[0], p[1], p[2]));
            if (b >= 0) count[b] += 1u;
        }
    uint64_t n = 0;
    for (uint32_t v : count) n += v;
    uint64_t rank = 0, before = 0;
    uint32_t b = 0;
    if (n) {
        rank = vrt::tone_rank(n, o.percentile);
        while (before + count[b] <= rank) before += count[b++];
    }
    const vrt::ToneMeter m{o.exposure, o.key, o.adapt, o.min_auto, o.max_auto, o.percentile};
    const vrt::ToneMetered r = vrt::tone_finish(m, n, rank, b, before, count[b], has_prev != 0, prev_exposure);
    if (info) {
        std::memset(info, 0, sizeof *info);
        info->exposure = r.exposure;
        info->target = r.target;
        info->luminance = r.luminance;
        info->bin = r.bin;
        info->counted = n;
        info->skipped = (uint64_t)wt * ht - n;
    }
    if (bins) std::memcpy(bins, count, sizeof count);
    return 0;
}

int vrth_tone_map(const float *rgb_in, uint64_t n, const vrt_tone_map *opts, float exposure, float *rgb_out) {
    if (!rgb_in || !rgb_out || !opts || !vrt::tone_setting_ok(*opts)) return -1;
    if (opts->curve == vrt::kToneOff) {
        if (rgb_out != rgb_in) std::memmove(rgb_out, rgb_in, n * sizeof(float));
        return 0;
    }
    const vrt::ToneCurve t = vrt::tone_curve_of(opts->curve, opts->flags, opts->white);
    for (uint64_t i = 0; i < n; i++) rgb_out[i] = vrt::tone_map_channel(t, exposure, rgb_in[i]);
    return 0;
}

}  // extern "C"

// vrt_set_water_optics' transmittance of n segments: csrc/both/water_math.h's vexp_neg of the binary32 product absorb * dist, the
// text and the product the water kernels compile
int vrth_water_transmittance(const float *absorb, const float *dist, uint64_t n, float *out) {
    if (!absorb || !dist || !out) return -1;
    for (uint64_t i = 0; i < n; i++) out[i] = vrt::vexp_neg(absorb[i] * dist[i]);
    return 0;
}

// vrt_set_water_refraction's bends (csrc/both/refract_math.h, the text the refracting kernels compile): A for leaving == 0, C otherwise
int vrth_water_refract(float ior, float reflectance, const float d[3], const float normal[3], float u, int leaving, float d_out[3]) {
    if (!d || !normal || !d_out || !(ior >= 1.0f && ior <= 4.0f)) return -1;
    if (leaving) return vrt::refract_leave(ior, reflectance, d, normal, u, d_out);
    vrt::refract_enter(1.0f / ior, d, normal, d_out);   // (eta as the context forms it)
    return VRTH_REFRACT_ENTERED;
}

// vrt_set_haze's distance draw and box exit: csrc/both/haze_math.h, the text the haze kernels compile
int vrth_haze_distance(const float *u, uint64_t n, float inv, float *out) {
    if (!u || !out) return -1;
    for (uint64_t i = 0; i < n; i++) out[i] = vrt::haze_distance(u[i], inv);
    return 0;
}

int vrth_haze_exit(const float o[3], const float d[3], float world_max, float *out) {
    if (!o || !d || !out) return -1;
    *out = vrt::haze_exit(o, d, world_max);
    return 0;
}

// ... and vrt_set_water_refraction's span walk over a host world: the voxel as vrth_world_get_voxels records it (0 outside the box, 0 without a chunk)
int vrth_world_water_span(const vrth_world *w, const vrt_material *mats256, const float o[3], const float d[3], uint32_t max_span, vrth_water_span *out) {
    if (!w || !mats256 || !o || !d || !out || max_span > vrt::kRefractSpanMax) return -1;
    const VoxelPos lo = w->w.min_voxel();
    const uint32_t W = w->w.size_in_voxels();
    const vrt::WaterSpan s = vrt::water_span(
        o, d, max_span ? max_span : vrt::kRefractSpanDefault,
        [&](int32_t x, int32_t y, int32_t z) -> uint32_t {
            if (!((uint32_t)x < W && (uint32_t)y < W && (uint32_t)z < W)) return 0u;
            Voxel v;
            return w->w.get_voxel(VoxelPos{lo.x + x, lo.y + y, lo.z + z}, v) == SetVoxelErr::Ok ? (uint32_t)v.as_data() : 0u;
        },
        [&](uint32_t v) { return mats256[v < 255u ? v : 255u].is_liquid == 1u; });
    memset(out, 0, sizeof *out);
    out->dist = s.dist;
    for (int k = 0; k < 3; k++) { out->prev[k] = s.prev[k]; out->m[k] = s.m[k]; }
    out->v = s.v;
    out->event = s.event ? 1u : 0u;
    out->steps = s.steps;
    return 0;
}

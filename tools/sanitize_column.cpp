// tools/sanitize_column.cpp — vrth_world_get_voxels / vrth_world_column_tops / vrth_world_top_map (the host twins of
// vrt_get_voxels, vrt_column_tops and vrt_read_top_map) under AddressSanitizer + UBSan, as a program of its own: a 3^3-chunk world
// with min (-32, -32, -32), missing chunks, a chunk of water and a lone voxel; every combination of INT32_MIN, INT32_MAX, the faces of
// the world box and a few inner values as x, z, y and from_y, every flag (and bits without a meaning), with and without a
// material table; the map with both flags.  Without flags every answer is checked against vrth_world_highest_vox_at.
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
//       -ffp-contract=off -o /tmp/sanitize_column tools/sanitize_column.cpp && /tmp/sanitize_column
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../voxelraytracing_amd/csrc/host/host_capi.cpp"

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); std::exit(1); } } while (0)

int main() {
    const int32_t centre[3] = {0, 0, 0};
    vrth_world *w = vrth_world_new(centre, 1 << 17, 3);
    CHECK(w);
    const uint16_t stone = 1, air = 0, water = 9;
    const int32_t chunks[4][3] = {{-1, -1, -1}, {0, 0, 0}, {1, 1, 1}, {0, 1, 0}};
    const uint16_t *fill[4] = {&stone, &air, &air, &water};
    for (int i = 0; i < 4; i++) CHECK(vrth_world_create_chunk(w, chunks[i], fill[i], 1, nullptr) == 0);
    const int32_t lone[3] = {5, 7, 9};
    CHECK(vrth_world_set_voxel(w, lone, 2, nullptr, nullptr) == 0);
    std::vector<vrt_material> mats(256);   // every id solid but air and the water
    std::memset(mats.data(), 0, 256 * sizeof(vrt_material));
    mats[0].is_empty = 1u;
    mats[water].is_liquid = 1u;

    const int32_t vals[] = {INT_MIN, INT_MAX, -33, -32, 0, 5, 63, 64, 94, 95, 96};
    std::vector<vrt_column_query> q;
    std::vector<int32_t> pos;
    for (int32_t x : vals)
        for (int32_t z : vals)
            for (int32_t y : vals)
                for (uint32_t f = 0; f < 4; f++) {
                    q.push_back({x, z, y, f | 0xFFFFFFF0u});
                    pos.insert(pos.end(), {x, y, z});
                }
    std::vector<vrt_column_top> with(q.size()), without(q.size());
    vrth_world_column_tops(w, mats.data(), q.data(), (uint32_t)q.size(), with.data(), 4);
    vrth_world_column_tops(w, nullptr, q.data(), (uint32_t)q.size(), without.data(), 1);
    unsigned found = 0, outside = 0;
    for (size_t i = 0; i < q.size(); i++) {
        vrt_column_top one;
        CHECK(vrth_world_column_top(w, mats.data(), &q[i], &one) == (int)with[i].status && one.y == with[i].y && one.voxel == with[i].voxel);
        found += with[i].status == VRT_COLUMN_FOUND;
        outside += with[i].status == VRT_COLUMN_OUTSIDE;
        if ((q[i].flags & 3u) == 0u && with[i].status != VRT_COLUMN_OUTSIDE) {   // highest_vox_at itself
            int32_t y = 0;
            const int has = vrth_world_highest_vox_at(w, q[i].x, q[i].z, &y);
            CHECK(has == (int)with[i].status && (!has || y == with[i].y) && (has || with[i].y == -33));
            CHECK(without[i].y == with[i].y && without[i].voxel == with[i].voxel);
        }
        if (q[i].flags & VRT_COLUMN_SOLID) CHECK(without[i].status != VRT_COLUMN_FOUND);   // no table: nothing is solid
    }
    CHECK(found > 0 && outside > 0);

    std::vector<vrt_voxel_at> vox(pos.size() / 3);
    vrth_world_get_voxels(w, pos.data(), (uint32_t)vox.size(), vox.data(), 4);
    unsigned by_status[4] = {0, 0, 0, 0};
    for (const vrt_voxel_at &v : vox) {
        CHECK(v.status <= 3 && v.status != 2 && (v.status == VRT_VOXEL_OK || v.voxel == 0));
        by_status[v.status]++;
    }
    CHECK(by_status[0] && by_status[1] && by_status[3]);

    std::vector<vrt_top_entry> map(96 * 96), solid(96 * 96);
    CHECK(vrth_world_top_map(w, nullptr, 0, map.data(), 4) == 0 && vrth_world_top_map(w, mats.data(), VRT_COLUMN_SOLID, solid.data(), 1) == 0);
    CHECK(vrth_world_top_map(w, nullptr, VRT_COLUMN_FROM_Y, map.data(), 1) == -1 && vrth_world_top_map(nullptr, nullptr, 0, map.data(), 1) == -1);
    CHECK(map[0].y == -1 && map[0].voxel == 1);                                       // the stone chunk at the world's corner
    CHECK(map[(9 + 32) * 96 + 5 + 32].y == 63 && map[(9 + 32) * 96 + 5 + 32].voxel == 9);   // water on top ...
    CHECK(solid[(9 + 32) * 96 + 5 + 32].y == 7 && solid[(9 + 32) * 96 + 5 + 32].voxel == 2);  // ... and the lone voxel under it
    CHECK(map[95 * 96 + 95].y == -33 && map[95 * 96 + 95].voxel == 0);                // an air chunk alone
    vrth_world_free(w);
    std::printf("sanitize_column: %zu queries (%u found, %u outside), %zu positions, two maps: ok\n", q.size(), found, outside, vox.size());
    return 0;
}

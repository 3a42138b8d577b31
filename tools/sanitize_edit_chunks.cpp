// tools/sanitize_edit_chunks.cpp — vrth_apply_shapes / vrth_edit_chunks (the host mirror of vrt_edit_chunks) under
// AddressSanitizer + UBSan, as a program of its own: the inputs of tests/test_edit_chunks_ref.py (generated chunks with a
// tree and a lake on their common corner, lines in every mode and of dist 4096, spheres and discs across chunk faces at negative
// coordinates, a refused tree, a short buffer, a set_node-built tree, every refused call), each answer checked against
// to_dense -> apply -> bottom_up done by hand.
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
//       -ffp-contract=off -o /tmp/sanitize_edit_chunks tools/sanitize_edit_chunks.cpp && /tmp/sanitize_edit_chunks
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../voxelraytracing_amd/csrc/host/host_capi.cpp"

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); std::exit(1); } } while (0)

static vrt_shape shape(uint32_t kind, uint32_t voxel, int ax, int ay, int az, int bx, int by, int bz, float r, uint32_t h) {
    vrt_shape s;
    s.kind = kind; s.voxel = voxel;
    s.a[0] = ax; s.a[1] = ay; s.a[2] = az;
    s.b[0] = bx; s.b[1] = by; s.b[2] = bz;
    s.r = r; s.height = h;
    return s;
}

struct Batch {
    std::vector<int32_t> pos;
    std::vector<uint16_t> nodes;
    std::vector<uint64_t> offs{0};
    void add(int x, int y, int z, const std::vector<uint16_t> &tree) {
        pos.insert(pos.end(), {x, y, z});
        nodes.insert(nodes.end(), tree.begin(), tree.end());
        offs.push_back(nodes.size());
    }
    uint32_t n() const { return (uint32_t)(offs.size() - 1); }
};

static std::vector<uint16_t> bottom_up(const uint16_t *dense) {
    std::vector<uint16_t> t(32768);
    t.resize(vrth_svo_build_bottom_up(dense, t.data(), 32768));
    return t;
}

// The call, and each chunk against to_dense -> vrth_apply_shapes -> bottom_up; returns the status
static int run(const Batch &b, const std::vector<vrt_shape> &shapes, int threads) {
    std::vector<uint64_t> offs(b.n() + 1, 77);
    std::vector<uint8_t> changed(b.n(), 9);
    int rc = vrth_edit_chunks(b.pos.data(), b.n(), b.nodes.data(), b.offs.data(), shapes.data(), (uint32_t)shapes.size(), nullptr, 0, offs.data(),
                              changed.data(), threads);
    CHECK(rc == VRT_ERR_OOM || (rc == VRT_OK && offs[b.n()] == 0) || rc == VRT_ERR_OUT_OF_RANGE);
    std::vector<uint16_t> out(offs[b.n()] + 1, 0xABCD);
    rc = vrth_edit_chunks(b.pos.data(), b.n(), b.nodes.data(), b.offs.data(), shapes.data(), (uint32_t)shapes.size(), out.data(), offs[b.n()],
                          offs.data(), changed.data(), threads);
    CHECK(rc == VRT_OK || rc == VRT_ERR_OUT_OF_RANGE);
    CHECK(out.back() == 0xABCD);
    for (uint32_t i = 0; i < b.n(); i++) {
        std::vector<uint16_t> before(32768), dense;
        vrth_svo_to_dense(b.nodes.data() + b.offs[i], before.data());
        dense = before;
        CHECK(vrth_apply_shapes(dense.data(), b.pos.data() + 3 * i, shapes.data(), (uint32_t)shapes.size()) == VRT_OK);
        const std::vector<uint16_t> want = bottom_up(dense.data());
        CHECK(offs[i + 1] - offs[i] == want.size());
        CHECK(std::equal(want.begin(), want.end(), out.begin() + offs[i]));
        CHECK(changed[i] == (dense != before));
    }
    return rc;
}

int main() {
    const uint32_t SEED = 1, WOOD = 53, LEAVES = 62, WATER = 3, STONE = 5;
    std::vector<uint16_t> dense(32768);
    // the 2 x 2 x 2 generated chunks around voxel (64, 96, 96), a tree beside the corner and a lake on it
    Batch blk;
    for (int z = 2; z <= 3; z++)
        for (int y = 2; y <= 3; y++)
            for (int x = 1; x <= 2; x++) {
                const int32_t p[3] = {x, y, z};
                vrth_gen_dense(SEED, p, dense.data());
                blk.add(x, y, z, bottom_up(dense.data()));
            }
    std::vector<vrt_shape> feature = {shape(VRT_SHAPE_SPHERE, LEAVES, 70, 108, 96, 0, 0, 0, 5.0f, 0), shape(VRT_SHAPE_SPHERE, LEAVES, 73, 106, 91, 0, 0, 0, 3.0f, 0),
                                      shape(VRT_SHAPE_LINE, WOOD, 70, 103, 96, 73, 106, 91, 0, 0), shape(VRT_SHAPE_LINE, WOOD, 70, 96, 96, 70, 108, 96, 0, 0)};
    for (int y = 0; y < 4; y++) feature.push_back(shape(VRT_SHAPE_DISC, WATER, 64, 96 - y - 3, 96, 0, 0, 0, 3.9f - 0.5f * (float)y, 1));
    for (int y = -2; y < 3; y++) feature.push_back(shape(VRT_SHAPE_DISC, 0, 64, 96 - y, 96, 0, 0, 0, 3.9f, 1));
    CHECK(run(blk, feature, 4) == VRT_OK);
    CHECK(run(blk, feature, 1) == VRT_OK);
    CHECK(run(blk, {}, 2) == VRT_OK);

    // lines in every mode and direction, ties, equal axes, dist 4096; spheres and discs over faces and at negative coordinates
    Batch around;
    for (int z = -2; z <= 1; z++)
        for (int y = -1; y <= 1; y++)
            for (int x = -2; x <= 1; x++) around.add(x, y, z, {(uint16_t)((x + y + z) & 1 ? 4 : 0)});
    std::vector<vrt_shape> mix;
    const int ends[][6] = {{5, 6, 7, 5, 6, 7}, {1, 2, 3, 40, 9, 20}, {40, 9, 20, 1, 2, 3}, {1, 2, 3, 9, 50, 20}, {9, 50, 20, 1, 2, 3}, {1, 2, 3, 9, 20, 61},
                           {9, 20, 61, 1, 2, 3}, {4, 2, 3, 4, 30, 11}, {4, 2, 3, 33, 2, -11}, {4, 2, 3, -20, 17, 3}, {0, 0, 0, 20, -20, 7},
                           {0, 0, 0, 3, 25, -25}, {-3, -3, -3, 14, 14, -20}, {-2048, 3, 5, 2048, 900, -700}};
    for (const auto &e : ends) mix.push_back(shape(VRT_SHAPE_LINE, WOOD, e[0], e[1], e[2], e[3], e[4], e[5], 0, 0));
    for (float r : {0.0f, 0.4f, 1.0f, 3.0f, 5.0f, 4.9f, 9.9f}) mix.push_back(shape(VRT_SHAPE_SPHERE, LEAVES, -1, 31, -33, 0, 0, 0, r, 0));
    for (uint32_t h : {0u, 1u, 3u})
        for (int w = 1; w <= 6; w++) mix.push_back(shape(VRT_SHAPE_DISC, STONE, 30, 30, 1, 0, 0, 0, (float)w * 0.5f - 0.1f, h));
    mix.push_back(shape(VRT_SHAPE_POINT, STONE, -1, -1, -1, 0, 0, 0, 0, 0));
    mix.push_back(shape(VRT_SHAPE_SPHERE, 0, 0, 0, 0, 0, 0, 0, 9.9f, 0));
    mix.push_back(shape(VRT_SHAPE_DISC, WATER, 0, -3, 0, 0, 0, 0, 32767.5f, 32768));
    CHECK(run(around, mix, 4) == VRT_OK);

    // a refused tree beside an ordinary chunk; a set_node-built input
    std::vector<vrt_shape> pts;
    for (int k = 0; k < 16; k++)
        for (int j = 0; j < 16; j++)
            for (int i = 0; i < 16; i++) pts.push_back(shape(VRT_SHAPE_POINT, STONE, 2 * i, 2 * j, 2 * k, 0, 0, 0, 0, 0));
    Batch two;
    two.add(0, 0, 0, {0});
    const int32_t p121[3] = {1, 2, 1};
    vrth_gen_dense(SEED, p121, dense.data());
    std::vector<uint16_t> loose(37449 + 64);
    loose.resize(vrth_svo_build_by_set_node(dense.data(), loose.data(), (uint32_t)loose.size()));
    CHECK(!loose.empty() && loose.size() <= 32761);
    two.add(1, 2, 1, loose);
    CHECK(run(two, pts, 2) == VRT_ERR_OUT_OF_RANGE);

    // refused calls: status only, outputs untouched
    uint64_t o[3] = {5, 5, 5};
    uint8_t ch[2] = {7, 7};
    uint16_t buf[64];
    const int32_t origin[6] = {0, 0, 0, 1, 0, 0};
    const uint16_t air[2] = {0, 0};
    const uint64_t offs1[2] = {0, 1};
    auto refused = [&](const vrt_shape &s, int want) {
        CHECK(vrth_edit_chunks(origin, 1, air, offs1, &s, 1, buf, 64, o, ch, 1) == want);
        CHECK(o[0] == 5 && o[1] == 5 && ch[0] == 7);
    };
    refused(shape(4, STONE, 0, 0, 0, 0, 0, 0, 1.0f, 1), VRT_ERR_INVALID_ARG);
    refused(shape(VRT_SHAPE_POINT, 0x8000, 0, 0, 0, 0, 0, 0, 0, 0), VRT_ERR_INVALID_ARG);
    refused(shape(VRT_SHAPE_SPHERE, STONE, 0, 0, 0, 0, 0, 0, -0.1f, 0), VRT_ERR_INVALID_ARG);
    refused(shape(VRT_SHAPE_DISC, STONE, 0, 0, 0, 0, 0, 0, NAN, 1), VRT_ERR_INVALID_ARG);
    refused(shape(VRT_SHAPE_SPHERE, STONE, 0, 0, 0, 0, 0, 0, 32768.0f, 0), VRT_ERR_INVALID_ARG);
    refused(shape(VRT_SHAPE_DISC, STONE, 0, 0, 0, 0, 0, 0, 1.0f, 32769), VRT_ERR_INVALID_ARG);
    refused(shape(VRT_SHAPE_POINT, STONE, 0, 1 << 22, 0, 0, 0, 0, 0, 0), VRT_ERR_INVALID_ARG);
    refused(shape(VRT_SHAPE_LINE, STONE, (1 << 22) - 5, 0, 0, 1 << 22, 0, 0, 0, 0), VRT_ERR_INVALID_ARG);
    refused(shape(VRT_SHAPE_LINE, STONE, 0, 0, 0, 5, -4097, 0, 0, 0), VRT_ERR_INVALID_ARG);
    refused(shape(VRT_SHAPE_LINE, STONE, -(1 << 22) + 1, 0, 0, (1 << 22) - 1, 0, 0, 0, 0), VRT_ERR_INVALID_ARG);   // (b - a: no overflow)
    const vrt_shape ok = shape(VRT_SHAPE_POINT, STONE, 1, 1, 1, 0, 0, 0, 0, 0);
    const uint16_t bad_child[8] = {0x8001, 0, 0, 0, 0, 0, 0, 0};
    const uint64_t offs8[2] = {0, 8};
    CHECK(vrth_edit_chunks(origin, 1, bad_child, offs8, &ok, 1, buf, 64, o, ch, 1) == VRT_ERR_INVALID_ARG);
    uint16_t deep[49] = {0};
    for (int d = 0; d < 6; d++) deep[d == 0 ? 0 : 1 + 8 * (d - 1)] = (uint16_t)(0x8000 | (1 + 8 * d));
    const uint64_t offs49[2] = {0, 49};
    CHECK(vrth_edit_chunks(origin, 1, deep, offs49, &ok, 1, buf, 64, o, ch, 1) == VRT_ERR_INVALID_ARG);
    const uint64_t down[3] = {1, 2, 1}, empty[3] = {0, 0, 1};
    CHECK(vrth_edit_chunks(origin, 2, air, down, &ok, 1, buf, 64, o, ch, 1) == VRT_ERR_INVALID_ARG);
    CHECK(vrth_edit_chunks(origin, 2, air, empty, &ok, 1, buf, 64, o, ch, 1) == VRT_ERR_INVALID_ARG);
    const int32_t far_chunk[3] = {0, 1 << 17, 0};
    CHECK(vrth_edit_chunks(far_chunk, 1, air, offs1, &ok, 1, buf, 64, o, ch, 1) == VRT_ERR_INVALID_ARG);
    CHECK(vrth_edit_chunks(origin, 1, air, offs1, nullptr, 1, buf, 64, o, ch, 1) == VRT_ERR_INVALID_ARG);
    CHECK(vrth_edit_chunks(origin, 1, air, offs1, &ok, 1, buf, 64, nullptr, ch, 1) == VRT_ERR_INVALID_ARG);
    std::vector<vrt_shape> many(65536, ok);
    CHECK(vrth_edit_chunks(origin, 1, air, offs1, many.data(), 65536, buf, 64, o, ch, 1) == VRT_ERR_OUT_OF_RANGE);
    CHECK(o[0] == 5 && o[1] == 5 && o[2] == 5 && ch[0] == 7 && ch[1] == 7);
    CHECK(vrth_edit_chunks(nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, 0, o, nullptr, 1) == VRT_OK && o[0] == 0);
    std::puts("sanitize_edit_chunks: ok");
    return 0;
}

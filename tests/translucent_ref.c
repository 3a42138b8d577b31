/* tests/translucent_ref.c — the path trace with the per-material emission, polish and translucency tables (include/vrt.h:
 * vrt_write_emission, vrt_write_polish, vrt_write_translucency), for the tests.  TEST INFRASTRUCTURE ONLY: compiled by
 * tests/translucent_ref.py with oracle/Makefile's CFLAGS into a temporary directory.
 *
 * tests/polish_ref.c's loop with steps 3 to 5 of vrt_write_translucency's contract: when the frame is translucent — some
 * entry's chance is not 0 — every hit after which the path may go on draws ut ahead of the coat's draw and the direction's six,
 * and where ut < the chance of the voxel's entry the path passes: no further draw, thr *= the entry's colour as written, dir
 * unchanged, and the origin moved across the one unit voxel that holds the hit position, in the form the march advances
 * across an air node.  With no chance that is not 0 nothing is drawn and the loop is polish_ref.c's.  The march, the sky and
 * the RNG are the oracle's own functions (this file includes it); the file is compiled without contraction, so the exit
 * arithmetic below is binary32 operation for operation. */
#include "../oracle/vrt_oracle.c"

typedef struct {   /* include/vrt.h: vrt_polish */
    float color[3];
    float chance;
    float scatter;
    uint32_t _reserved[3];
} ref_polish;

typedef struct {   /* include/vrt.h: vrt_translucency */
    float color[3];
    float chance;
} ref_translucency;

/* step 5's exit: how far along dir the unit voxel of pos ends on one axis */
static float exit_t(float pos, float dir) {
    const float c = floorf(pos);
    const float far = dir > 0.0f ? c + 1.0f : c;
    return dir != 0.0f ? (far - pos) / dir : INFINITY;
}

static v3 trace_path_translucent(const orc_scene *s, const float *emission, const ref_polish *polish, const ref_translucency *tr,
                                 int polished_frame, int translucent_frame, uint32_t px, uint32_t py, uint32_t rng, uint32_t *id,
                                 uint64_t *n_passes) {
    v3 light = V3(0.0f, 0.0f, 0.0f);
    v3 origin, dir;
    create_ray_from_screen(s, (int32_t)px, (int32_t)py, &origin, &dir);
    v3 thr = V3(1.0f, 1.0f, 1.0f);
    for (uint32_t bounce = 0; bounce < s->settings.max_ray_bounces; bounce++) {
        hit_result rs = ray_world(s, origin, dir);
        if (bounce == 0) *id = id_word(&rs);
        if (!rs.hit) {
            v3 sky = ray_sky(s, origin, dir);
            light.x += sky.x * thr.x;
            light.y += sky.y * thr.y;
            light.z += sky.z * thr.z;
            break;
        }
        const uint32_t entry = rs.voxel > 255u ? 255u : rs.voxel;
        const float e = emission[entry];
        if (e != 0.0f) {
            light.x += (rs.color.x * e) * thr.x;
            light.y += (rs.color.y * e) * thr.y;
            light.z += (rs.color.z * e) * thr.z;
        }
        if (bounce + 1 == s->settings.max_ray_bounces) break;   /* the last allowed segment: what follows is observed by nothing */
        if (translucent_frame && orc_rng_next(&rng) < tr[entry].chance) {   /* ut: ahead of u and of the direction */
            const float tx = exit_t(rs.pos.x, dir.x), ty = exit_t(rs.pos.y, dir.y), tz = exit_t(rs.pos.z, dir.z);
            float t = tx;
            if (ty < t) t = ty;
            if (tz < t) t = tz;
            const float ts = t + 0.001f;
            thr.x *= tr[entry].color[0]; thr.y *= tr[entry].color[1]; thr.z *= tr[entry].color[2];
            origin = V3(rs.pos.x + dir.x * ts, rs.pos.y + dir.y * ts, rs.pos.z + dir.z * ts);
            *n_passes += 1u;
            continue;
        }
        int polished = 0;
        if (polished_frame) polished = orc_rng_next(&rng) < polish[entry].chance;   /* :175, before :178 */
        float d = orc_dot(rs.norm, dir);
        v3 spec = V3(dir.x - 2.0f * rs.norm.x * d, dir.y - 2.0f * rs.norm.y * d, dir.z - 2.0f * rs.norm.z * d);
        v3 rd = rng_next_dir(&rng);
        v3 sc = orc_normalize(V3(rs.norm.x + rd.x, rs.norm.y + rd.y, rs.norm.z + rd.z));
        float scatter = polished ? polish[entry].scatter : mat_at(s, rs.voxel)->scatter;   /* :180 */
        v3 nd = orc_normalize(V3(orc_mix(spec.x, sc.x, scatter), orc_mix(spec.y, sc.y, scatter), orc_mix(spec.z, sc.z, scatter)));
        v3 tint = polished ? V3(polish[entry].color[0], polish[entry].color[1], polish[entry].color[2]) : rs.color;   /* :185 */
        thr.x *= tint.x; thr.y *= tint.y; thr.z *= tint.z;
        origin = V3(rs.pos.x + rs.norm.x * ORC_SHADOW_BIAS, rs.pos.y + rs.norm.y * ORC_SHADOW_BIAS, rs.pos.z + rs.norm.z * ORC_SHADOW_BIAS);
        dir = nd;
    }
    return light;
}

/* A w x h path-trace frame of samples sample_base .. sample_base + spp - 1 (seeded as orc_render seeds sample s), their mean
 * in rgb[h][w][3], the primary segment's id word in ids[h][w]; returns how many times a path passed through a voxel.  Like
 * orc_render, pixels beyond the last whole 8 x 8 tile are not traced: the caller passes zeroed arrays. */
uint64_t ref_render_path_translucent(const orc_scene *scene, const float *emission, const ref_polish *polish, const ref_translucency *tr,
                                     uint32_t w, uint32_t h, uint32_t spp, uint32_t seed, uint32_t sample_base, float *rgb, uint32_t *ids) {
    const uint32_t x1 = w & ~7u, y1 = h & ~7u, nspp = spp ? spp : 1u;
    int polished_frame = 0, translucent_frame = 0;
    for (uint32_t i = 0; i < 256u; i++) {
        polished_frame |= polish[i].chance != 0.0f;
        translucent_frame |= tr[i].chance != 0.0f;
    }
    uint64_t total = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : total)
    for (int32_t py = 0; py < (int32_t)y1; py++) {
        for (uint32_t px = 0; px < x1; px++) {
            const size_t o = (size_t)py * w + px;
            v3 sum = V3(0.0f, 0.0f, 0.0f);
            uint32_t id = 0;
            for (uint32_t sm = 0; sm < nspp; sm++) {
                uint32_t sid = 0;
                uint64_t np = 0;
                v3 l = trace_path_translucent(scene, emission, polish, tr, polished_frame, translucent_frame, px, (uint32_t)py,
                                              path_seed(px, (uint32_t)py, w, h, sample_base + sm, seed), &sid, &np);
                sum.x += l.x; sum.y += l.y; sum.z += l.z;
                total += np;
                if (sm == 0) id = sid;
            }
            rgb[o * 3 + 0] = sum.x / (float)nspp;
            rgb[o * 3 + 1] = sum.y / (float)nspp;
            rgb[o * 3 + 2] = sum.z / (float)nspp;
            ids[o] = id;
        }
    }
    return total;
}

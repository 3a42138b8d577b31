/* tests/polish_ref.c — the path trace with the per-material emission and polish tables (include/vrt.h: vrt_write_emission,
 * vrt_write_polish), for the tests.  TEST INFRASTRUCTURE ONLY: compiled by tests/polish_ref.py with oracle/Makefile's CFLAGS
 * into a temporary directory.
 *
 * oracle/vrt_oracle.c's trace_path_into has neither table (the live Material has neither field).  This restates its loop with
 * the emission term of path_tracer.wgsl:183-184, as tests/emission_ref.c does, and — when the frame is polished: some entry's
 * chance is not 0 — with the three lines of :175, :180 and :185: on every hit one draw u ahead of rng_next_dir's six, and
 * where u < the chance of the voxel's entry, the entry's scatter in place of the material's and the entry's colour, as
 * written, in place of mc in thr *= mc.  Both are selects.  With no chance that is not 0 nothing is drawn and the loop is
 * emission_ref.c's.  The march, the sky and the RNG are the oracle's own functions (this file includes it), so every
 * direction is bit for bit the oracle's and the kernels'. */
#include "../oracle/vrt_oracle.c"

typedef struct {   /* include/vrt.h: vrt_polish */
    float color[3];
    float chance;
    float scatter;
    uint32_t _reserved[3];
} ref_polish;

static v3 trace_path_polished(const orc_scene *s, const float *emission, const ref_polish *polish, int polished_frame, uint32_t px, uint32_t py,
                              uint32_t rng, uint32_t *id, uint64_t *n_polished) {
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
        *n_polished += polished ? 1u : 0u;
    }
    return light;
}

/* A w x h path-trace frame of samples sample_base .. sample_base + spp - 1 (seeded as orc_render seeds sample s), their mean
 * in rgb[h][w][3], the primary segment's id word in ids[h][w]; returns how many bounces went off a coat.  Like orc_render,
 * pixels beyond the last whole 8 x 8 tile are not traced: the caller passes zeroed arrays. */
uint64_t ref_render_path_polished(const orc_scene *scene, const float *emission, const ref_polish *polish, uint32_t w, uint32_t h, uint32_t spp,
                                  uint32_t seed, uint32_t sample_base, float *rgb, uint32_t *ids) {
    const uint32_t x1 = w & ~7u, y1 = h & ~7u, nspp = spp ? spp : 1u;
    int polished_frame = 0;
    for (uint32_t i = 0; i < 256u; i++) polished_frame |= polish[i].chance != 0.0f;
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
                v3 l = trace_path_polished(scene, emission, polish, polished_frame, px, (uint32_t)py,
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

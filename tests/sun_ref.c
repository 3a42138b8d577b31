/* tests/sun_ref.c — the path trace with direct sunlight (include/vrt.h: vrt_set_sun_light) on top of the per-material emission,
 * polish and translucency tables, for the tests.  TEST INFRASTRUCTURE ONLY: compiled by tests/sun_ref.py with oracle/Makefile's
 * CFLAGS into a temporary directory.
 *
 * tests/translucent_ref.c's loop with steps 2 and 4 of vrt_set_sun_light's contract: with a strength that is not 0 every hit on
 * a solid voxel — the primary segment's and the last allowed segment's included — whose face looks at the sun sends a ray
 * there from the bounce origin (shadow_ray's origin and direction, marched by the oracle's own ray_world), and where that
 * ray does not hit, (mc * (k * c)) * thr joins the sample's light right behind the hit's emission term; a segment other than the
 * primary that misses takes the sky of a copy of the scene whose sun_intensity is 0, so the disc is not counted twice.  The sun
 * term draws nothing.  With strength 0 the loop is translucent_ref.c's.  Compiled without contraction: binary32 operation for
 * operation. */
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

enum { SUN_RAYS, SUN_UNOCCLUDED, SUN_DISC_MISSES, SUN_STEPS, SUN_BOUNCE_SEGMENTS, SUN_COUNTS };

/* translucent_ref.c's exit: how far along dir the unit voxel of pos ends on one axis */
static float exit_t(float pos, float dir) {
    const float c = floorf(pos);
    const float far = dir > 0.0f ? c + 1.0f : c;
    return dir != 0.0f ? (far - pos) / dir : INFINITY;
}

static v3 trace_path_sun(const orc_scene *s, const orc_scene *s_no_disc, const float *emission, const ref_polish *polish,
                         const ref_translucency *tr, int polished_frame, int translucent_frame, float strength, uint32_t px, uint32_t py,
                         uint32_t rng, uint32_t *id, uint64_t *n) {
    v3 light = V3(0.0f, 0.0f, 0.0f);
    v3 origin, dir;
    create_ray_from_screen(s, (int32_t)px, (int32_t)py, &origin, &dir);
    v3 thr = V3(1.0f, 1.0f, 1.0f);
    const int sun_lit = strength != 0.0f;
    for (uint32_t bounce = 0; bounce < s->settings.max_ray_bounces; bounce++) {
        hit_result rs = ray_world(s, origin, dir);
        n[SUN_STEPS] += rs.iter_count;
        if (bounce != 0) n[SUN_BOUNCE_SEGMENTS] += 1u;
        if (bounce == 0) *id = id_word(&rs);
        if (!rs.hit) {
            v3 sky = ray_sky(s, origin, dir);
            if (sun_lit && bounce != 0) {   /* step 4: add = +0 */
                const v3 plain = ray_sky(s_no_disc, origin, dir);
                if (plain.x != sky.x || plain.y != sky.y || plain.z != sky.z) n[SUN_DISC_MISSES] += 1u;
                sky = plain;
            }
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
        if (sun_lit && is_solid_hit(s, &rs)) {   /* step 2 */
            const v3 so = V3(rs.pos.x + rs.norm.x * ORC_SHADOW_BIAS, rs.pos.y + rs.norm.y * ORC_SHADOW_BIAS, rs.pos.z + rs.norm.z * ORC_SHADOW_BIAS);
            const v3 sd = orc_normalize(V3(s->settings.sun_pos[0] - (float)s->world.min[0] - so.x,
                                           s->settings.sun_pos[1] - (float)s->world.min[1] - so.y,
                                           s->settings.sun_pos[2] - (float)s->world.min[2] - so.z));
            const float c = orc_dot(rs.norm, sd);
            if (c > 0.0f) {
                const hit_result sh = ray_world(s, so, sd);
                n[SUN_RAYS] += 1u;
                n[SUN_STEPS] += sh.iter_count;
                if (!sh.hit) {
                    const float k = s->settings.sun_intensity * strength;
                    const float w = k * c;
                    n[SUN_UNOCCLUDED] += 1u;
                    light.x += (rs.color.x * w) * thr.x;
                    light.y += (rs.color.y * w) * thr.y;
                    light.z += (rs.color.z * w) * thr.z;
                }
            }
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
            continue;
        }
        int polished = 0;
        if (polished_frame) polished = orc_rng_next(&rng) < polish[entry].chance;
        float d = orc_dot(rs.norm, dir);
        v3 spec = V3(dir.x - 2.0f * rs.norm.x * d, dir.y - 2.0f * rs.norm.y * d, dir.z - 2.0f * rs.norm.z * d);
        v3 rd = rng_next_dir(&rng);
        v3 sc = orc_normalize(V3(rs.norm.x + rd.x, rs.norm.y + rd.y, rs.norm.z + rd.z));
        float scatter = polished ? polish[entry].scatter : mat_at(s, rs.voxel)->scatter;
        v3 nd = orc_normalize(V3(orc_mix(spec.x, sc.x, scatter), orc_mix(spec.y, sc.y, scatter), orc_mix(spec.z, sc.z, scatter)));
        v3 tint = polished ? V3(polish[entry].color[0], polish[entry].color[1], polish[entry].color[2]) : rs.color;
        thr.x *= tint.x; thr.y *= tint.y; thr.z *= tint.z;
        origin = V3(rs.pos.x + rs.norm.x * ORC_SHADOW_BIAS, rs.pos.y + rs.norm.y * ORC_SHADOW_BIAS, rs.pos.z + rs.norm.z * ORC_SHADOW_BIAS);
        dir = nd;
    }
    return light;
}

/* A w x h path-trace frame of samples sample_base .. sample_base + spp - 1 (seeded as orc_render seeds sample s), their mean
 * in rgb[h][w][3], the primary segment's id word in ids[h][w]; counts[SUN_COUNTS]: the sun rays marched, the unoccluded ones,
 * the later segments' misses through the sun's disc, the lookups of every march (segments and sun rays) and the segments
 * behind the primary ones.  Like orc_render, pixels beyond the last whole 8 x 8 tile are not traced: the caller passes zeroed
 * arrays. */
void ref_render_path_sun(const orc_scene *scene, const float *emission, const ref_polish *polish, const ref_translucency *tr, float strength,
                         uint32_t w, uint32_t h, uint32_t spp, uint32_t seed, uint32_t sample_base, float *rgb, uint32_t *ids, uint64_t *counts) {
    const uint32_t x1 = w & ~7u, y1 = h & ~7u, nspp = spp ? spp : 1u;
    int polished_frame = 0, translucent_frame = 0;
    for (uint32_t i = 0; i < 256u; i++) {
        polished_frame |= polish[i].chance != 0.0f;
        translucent_frame |= tr[i].chance != 0.0f;
    }
    orc_scene no_disc = *scene;
    no_disc.settings.sun_intensity = 0.0f;
    uint64_t n0 = 0, n1 = 0, n2 = 0, n3 = 0, n4 = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : n0, n1, n2, n3, n4)
    for (int32_t py = 0; py < (int32_t)y1; py++) {
        for (uint32_t px = 0; px < x1; px++) {
            const size_t o = (size_t)py * w + px;
            v3 sum = V3(0.0f, 0.0f, 0.0f);
            uint32_t id = 0;
            for (uint32_t sm = 0; sm < nspp; sm++) {
                uint32_t sid = 0;
                uint64_t n[SUN_COUNTS] = {0, 0, 0, 0, 0};
                v3 l = trace_path_sun(scene, &no_disc, emission, polish, tr, polished_frame, translucent_frame, strength, px, (uint32_t)py,
                                      path_seed(px, (uint32_t)py, w, h, sample_base + sm, seed), &sid, n);
                sum.x += l.x; sum.y += l.y; sum.z += l.z;
                n0 += n[0]; n1 += n[1]; n2 += n[2]; n3 += n[3]; n4 += n[4];
                if (sm == 0) id = sid;
            }
            rgb[o * 3 + 0] = sum.x / (float)nspp;
            rgb[o * 3 + 1] = sum.y / (float)nspp;
            rgb[o * 3 + 2] = sum.z / (float)nspp;
            ids[o] = id;
        }
    }
    counts[SUN_RAYS] = n0; counts[SUN_UNOCCLUDED] = n1; counts[SUN_DISC_MISSES] = n2; counts[SUN_STEPS] = n3; counts[SUN_BOUNCE_SEGMENTS] = n4;
}

/* one pixel's one sample, for the hand check of the sum order: the light, and counts as above */
void ref_trace_pixel_sun(const orc_scene *scene, const float *emission, const ref_polish *polish, const ref_translucency *tr, float strength,
                         uint32_t w, uint32_t h, uint32_t px, uint32_t py, uint32_t sample, uint32_t seed, float *light, uint64_t *counts) {
    int polished_frame = 0, translucent_frame = 0;
    for (uint32_t i = 0; i < 256u; i++) {
        polished_frame |= polish[i].chance != 0.0f;
        translucent_frame |= tr[i].chance != 0.0f;
    }
    orc_scene no_disc = *scene;
    no_disc.settings.sun_intensity = 0.0f;
    uint32_t id = 0;
    for (int i = 0; i < SUN_COUNTS; i++) counts[i] = 0;
    const v3 l = trace_path_sun(scene, &no_disc, emission, polish, tr, polished_frame, translucent_frame, strength, px, py,
                                path_seed(px, py, w, h, sample, seed), &id, counts);
    light[0] = l.x; light[1] = l.y; light[2] = l.z;
}

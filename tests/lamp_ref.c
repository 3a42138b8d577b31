/* tests/lamp_ref.c — the path trace with lamp light (include/vrt.h: vrt_set_lamp_light) on top of camera sampling, direct
 * sunlight and the per-material emission, polish and translucency tables, for the tests.  TEST INFRASTRUCTURE ONLY: compiled by
 * tests/lamp_ref.py with oracle/Makefile's CFLAGS into a temporary directory.
 *
 * tests/lens_ref.c's loop with steps 2, 4 and 5 of vrt_set_lamp_light's contract added: the emission term only while the path is
 * direct, three draws on every hit ahead of every other draw of the hit, and a ray to a point of a face of the lamp list.  With
 * the lamp strength 0 the loop is lens_ref.c's, operation for operation.  The list itself is made by tests/lamp_ref.py from a
 * dense copy of the world (ref_dense_world below walks the octree with the oracle's find_node) and handed in.  Compiled without
 * contraction. */
#include "lens_ref.c"

typedef struct {   /* include/vrt.h: vrt_lamp_light */
    float strength;
    float max_geometry;
    uint32_t flags;
    uint32_t _reserved;
} ref_lamp_light;

typedef struct {   /* include/vrt.h: vrt_lamp */
    uint16_t pos[3];
    uint16_t voxel;
    uint32_t face;
    uint32_t _reserved;
} ref_lamp;

/* steps: the lookups of every march; bounce segments: the segments behind the primary ones; sun rays and lamp rays marched; the
 * lamp rays that arrived; hits whose emission term was dropped because the path was no longer direct.  Beside them, where the
 * caller asks: per list entry, the lamp rays that arrived at it */
enum { LAMP_STEPS, LAMP_BOUNCE_SEGMENTS, LAMP_SUN_RAYS, LAMP_RAYS, LAMP_UNOCCLUDED, LAMP_EMISSION_DROPPED, LAMP_COUNTS };

/* what a segment of a sample hands to the launches behind it, where the caller asks (ref_render_path_lamp_load): the path goes on
 * into the next segment (it hit, and this was not its last allowed segment); a sun ray was marched from the hit; a lamp ray was */
enum { LOAD_PATH = 1, LOAD_SUN = 2, LOAD_LAMP = 4 };

/* the voxel id of every unit voxel of the world, dense[z][y][x], by the oracle's own walk */
void ref_dense_world(const orc_scene *scene, uint16_t *dense) {
    const int32_t n = (int32_t)scene->world.size_in_chunks * 32;
#pragma omp parallel for schedule(static)
    for (int32_t z = 0; z < n; z++)
        for (int32_t y = 0; y < n; y++)
            for (int32_t x = 0; x < n; x++) {
                const found_node f = find_node(scene, V3((float)x + 0.5f, (float)y + 0.5f, (float)z + 0.5f), 5u);
                dense[((size_t)z * n + y) * n + x] = (uint16_t)node_voxel(node_at(scene, f.root + f.idx));
            }
}

static float comp(v3 v, uint32_t a) { return a == 0u ? v.x : (a == 1u ? v.y : v.z); }

/* one sample: its light; *id: the id word of ITS primary segment */
static v3 trace_path_lamp(const orc_scene *s, const orc_scene *s_no_disc, const float *emission, const ref_polish *polish,
                          const ref_translucency *tr, int polished_frame, int translucent_frame, float sun_strength, const ref_camera_sampling *cs,
                          const ref_lamp_light *ll, const ref_lamp *list, uint32_t N, uint32_t px, uint32_t py, uint32_t rng, uint32_t *id, uint64_t *n,
                          uint32_t *arrived, uint8_t *load, size_t load_stride) {
    v3 light = V3(0.0f, 0.0f, 0.0f);
    v3 origin, dir;
    if (cs->pixel_spread != 0.0f || cs->aperture != 0.0f) {
        float u[4];
        for (int i = 0; i < 4; i++) u[i] = orc_rng_next(&rng);
        v3 w, v;
        lens_ray(s, cs, px, py, u, &origin, &dir, &w, &v);
    } else {
        create_ray_from_screen(s, (int32_t)px, (int32_t)py, &origin, &dir);
    }
    v3 thr = V3(1.0f, 1.0f, 1.0f);
    const int sun_lit = sun_strength != 0.0f, lamp_lit = ll->strength != 0.0f;
    int direct = 1;
    for (uint32_t bounce = 0; bounce < s->settings.max_ray_bounces; bounce++) {
        hit_result rs = ray_world(s, origin, dir);
        n[LAMP_STEPS] += rs.iter_count;
        if (bounce != 0) n[LAMP_BOUNCE_SEGMENTS] += 1u;
        if (bounce == 0) *id = id_word(&rs);
        if (!rs.hit) {
            v3 sky = ray_sky(s, origin, dir);
            if (sun_lit && bounce != 0) sky = ray_sky(s_no_disc, origin, dir);
            light.x += sky.x * thr.x;
            light.y += sky.y * thr.y;
            light.z += sky.z * thr.z;
            break;
        }
        const uint32_t entry = rs.voxel > 255u ? 255u : rs.voxel;
        const float e = emission[entry];
        if (e != 0.0f) {
            if (!lamp_lit || direct) {   /* step 2 */
                light.x += (rs.color.x * e) * thr.x;
                light.y += (rs.color.y * e) * thr.y;
                light.z += (rs.color.z * e) * thr.z;
            } else {
                n[LAMP_EMISSION_DROPPED] += 1u;
            }
        }
        if (sun_lit && is_solid_hit(s, &rs)) {   /* step 3 */
            const v3 so = V3(rs.pos.x + rs.norm.x * ORC_SHADOW_BIAS, rs.pos.y + rs.norm.y * ORC_SHADOW_BIAS, rs.pos.z + rs.norm.z * ORC_SHADOW_BIAS);
            const v3 sd = orc_normalize(V3(s->settings.sun_pos[0] - (float)s->world.min[0] - so.x,
                                           s->settings.sun_pos[1] - (float)s->world.min[1] - so.y,
                                           s->settings.sun_pos[2] - (float)s->world.min[2] - so.z));
            const float c = orc_dot(rs.norm, sd);
            if (c > 0.0f) {
                const hit_result sh = ray_world(s, so, sd);
                n[LAMP_SUN_RAYS] += 1u;
                if (load) load[bounce * load_stride] |= LOAD_SUN;
                n[LAMP_STEPS] += sh.iter_count;
                if (!sh.hit) {
                    const float k = s->settings.sun_intensity * sun_strength;
                    const float w = k * c;
                    light.x += (rs.color.x * w) * thr.x;
                    light.y += (rs.color.y * w) * thr.y;
                    light.z += (rs.color.z * w) * thr.z;
                }
            }
        }
        if (lamp_lit) {
            const float u1 = orc_rng_next(&rng), u2 = orc_rng_next(&rng), u3 = orc_rng_next(&rng);   /* step 4: the last segment's too */
            if (is_solid_hit(s, &rs) && N > 0u) {   /* step 5 */
                const v3 so = V3(rs.pos.x + rs.norm.x * ORC_SHADOW_BIAS, rs.pos.y + rs.norm.y * ORC_SHADOW_BIAS, rs.pos.z + rs.norm.z * ORC_SHADOW_BIAS);
                uint32_t j = (uint32_t)(u1 * (float)N);
                if (j > N - 1u) j = N - 1u;
                const ref_lamp *L = &list[j];
                const uint32_t a = L->face >> 1, sd = L->face & 1u;
                float q[3];
                q[a] = (float)L->pos[a] + (float)sd;
                const uint32_t b = a == 0u ? 1u : 0u, c2 = a == 2u ? 1u : 2u;
                q[b] = (float)L->pos[b] + u2;
                q[c2] = (float)L->pos[c2] + u3;
                const v3 v = V3(q[0] - so.x, q[1] - so.y, q[2] - so.z);
                const float d2 = (v.x * v.x + v.y * v.y) + v.z * v.z;
                const v3 ld = orc_normalize(v);
                const float c = orc_dot(rs.norm, ld);
                const float cl = sd ? -comp(ld, a) : comp(ld, a);
                if (c > 0.0f && cl > 0.0f) {
                    const hit_result lh = ray_world(s, so, ld);
                    n[LAMP_RAYS] += 1u;
                    if (load) load[bounce * load_stride] |= LOAD_LAMP;
                    n[LAMP_STEPS] += lh.iter_count;
                    const int unoccluded = lh.hit && (int)floorf(lh.pos.x) == (int)L->pos[0] && (int)floorf(lh.pos.y) == (int)L->pos[1] &&
                                           (int)floorf(lh.pos.z) == (int)L->pos[2];
                    float g = (c * cl) / d2;
                    if (ll->max_geometry != 0.0f && g > ll->max_geometry) g = ll->max_geometry;
                    const uint32_t lentry = L->voxel > 255u ? 255u : L->voxel;
                    const float k = ((ll->strength * emission[lentry]) * 0.318309886f) * (float)N;
                    const float w = k * g;
                    const orc_material *lm = mat_at(s, L->voxel);
                    v3 lc = V3(lm->color[0], lm->color[1], lm->color[2]);
                    if (a == 0u) { lc.x *= 0.5f; lc.y *= 0.5f; lc.z *= 0.5f; }
                    if (a == 2u) { lc.x *= 0.7f; lc.y *= 0.7f; lc.z *= 0.7f; }
                    if (L->face == 2u) { lc.x *= 0.2f; lc.y *= 0.2f; lc.z *= 0.2f; }
                    if (unoccluded) {
                        n[LAMP_UNOCCLUDED] += 1u;
                        if (arrived) {
#pragma omp atomic
                            arrived[j] += 1u;
                        }
                        light.x += ((rs.color.x * lc.x) * w) * thr.x;
                        light.y += ((rs.color.y * lc.y) * w) * thr.y;
                        light.z += ((rs.color.z * lc.z) * w) * thr.z;
                    }
                }
            }
        }
        if (bounce + 1 == s->settings.max_ray_bounces) break;   /* the last allowed segment: what follows is observed by nothing */
        if (load) load[bounce * load_stride] |= LOAD_PATH;
        if (translucent_frame && orc_rng_next(&rng) < tr[entry].chance) {   /* ut: ahead of u and of the direction; the path stays direct */
            const float tx = exit_t(rs.pos.x, dir.x), ty = exit_t(rs.pos.y, dir.y), tz = exit_t(rs.pos.z, dir.z);
            float t = tx;
            if (ty < t) t = ty;
            if (tz < t) t = tz;
            const float ts = t + 0.001f;
            thr.x *= tr[entry].color[0]; thr.y *= tr[entry].color[1]; thr.z *= tr[entry].color[2];
            origin = V3(rs.pos.x + dir.x * ts, rs.pos.y + dir.y * ts, rs.pos.z + dir.z * ts);
            continue;
        }
        direct = 0;   /* the first bounce */
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

/* lens_ref.c's ref_render_path_lens with the lamp setting and the lamp list; counts[LAMP_COUNTS] as the enum says.  arrived: NULL, or
 * N words that the frame adds to: per list entry, the lamp rays that arrived at it unoccluded (their sum grows by counts[LAMP_UNOCCLUDED]).
 * load: NULL, or load[spp][max_ray_bounces][h][w] bytes, zero on entry: the LOAD_ bits of segment b of sample s of pixel (x, y) */
void ref_render_path_lamp_load(const orc_scene *scene, const float *emission, const ref_polish *polish, const ref_translucency *tr,
                               float sun_strength, const ref_camera_sampling *cs, const ref_lamp_light *ll, const ref_lamp *list, uint32_t N,
                               uint32_t w, uint32_t h, uint32_t spp, uint32_t seed, uint32_t sample_base, float *rgb, uint32_t *ids,
                               uint64_t *counts, uint32_t *arrived, uint8_t *load) {
    const size_t plane = (size_t)w * h;
    const uint32_t x1 = w & ~7u, y1 = h & ~7u, nspp = spp ? spp : 1u;
    const int on = cs->pixel_spread != 0.0f || cs->aperture != 0.0f;
    int polished_frame, translucent_frame;
    frame_kinds(polish, tr, &polished_frame, &translucent_frame);
    orc_scene no_disc = *scene;
    no_disc.settings.sun_intensity = 0.0f;
    uint64_t n0 = 0, n1 = 0, n2 = 0, n3 = 0, n4 = 0, n5 = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : n0, n1, n2, n3, n4, n5)
    for (int32_t py = 0; py < (int32_t)y1; py++) {
        for (uint32_t px = 0; px < x1; px++) {
            const size_t o = (size_t)py * w + px;
            v3 sum = V3(0.0f, 0.0f, 0.0f);
            uint32_t id = 0;
            if (on && scene->settings.max_ray_bounces > 0u) {   /* the pixel's own ray, shaded by nobody */
                v3 origin, dir;
                create_ray_from_screen(scene, (int32_t)px, py, &origin, &dir);
                const hit_result rc = ray_world(scene, origin, dir);
                n0 += rc.iter_count;
                id = id_word(&rc);
            }
            for (uint32_t sm = 0; sm < nspp; sm++) {
                uint32_t sid = 0;
                uint64_t n[LAMP_COUNTS] = {0, 0, 0, 0, 0, 0};
                v3 l = trace_path_lamp(scene, &no_disc, emission, polish, tr, polished_frame, translucent_frame, sun_strength, cs, ll, list, N, px,
                                       (uint32_t)py, path_seed(px, (uint32_t)py, w, h, sample_base + sm, seed), &sid, n, arrived,
                                       load ? load + ((size_t)sm * scene->settings.max_ray_bounces) * plane + o : NULL, plane);
                sum.x += l.x; sum.y += l.y; sum.z += l.z;
                n0 += n[0]; n1 += n[1]; n2 += n[2]; n3 += n[3]; n4 += n[4]; n5 += n[5];
                if (!on && sm == 0) id = sid;
            }
            rgb[o * 3 + 0] = sum.x / (float)nspp;
            rgb[o * 3 + 1] = sum.y / (float)nspp;
            rgb[o * 3 + 2] = sum.z / (float)nspp;
            ids[o] = id;
        }
    }
    counts[0] = n0; counts[1] = n1; counts[2] = n2; counts[3] = n3; counts[4] = n4; counts[5] = n5;
}

void ref_render_path_lamp_arrivals(const orc_scene *scene, const float *emission, const ref_polish *polish, const ref_translucency *tr,
                                   float sun_strength, const ref_camera_sampling *cs, const ref_lamp_light *ll, const ref_lamp *list, uint32_t N,
                                   uint32_t w, uint32_t h, uint32_t spp, uint32_t seed, uint32_t sample_base, float *rgb, uint32_t *ids,
                                   uint64_t *counts, uint32_t *arrived) {
    ref_render_path_lamp_load(scene, emission, polish, tr, sun_strength, cs, ll, list, N, w, h, spp, seed, sample_base, rgb, ids, counts, arrived, NULL);
}

void ref_render_path_lamp(const orc_scene *scene, const float *emission, const ref_polish *polish, const ref_translucency *tr, float sun_strength,
                          const ref_camera_sampling *cs, const ref_lamp_light *ll, const ref_lamp *list, uint32_t N, uint32_t w, uint32_t h, uint32_t spp,
                          uint32_t seed, uint32_t sample_base, float *rgb, uint32_t *ids, uint64_t *counts) {
    ref_render_path_lamp_arrivals(scene, emission, polish, tr, sun_strength, cs, ll, list, N, w, h, spp, seed, sample_base, rgb, ids, counts, NULL);
}

/* one pixel's one sample: its light and its counts */
void ref_trace_pixel_lamp(const orc_scene *scene, const float *emission, const ref_polish *polish, const ref_translucency *tr, float sun_strength,
                          const ref_camera_sampling *cs, const ref_lamp_light *ll, const ref_lamp *list, uint32_t N, uint32_t w, uint32_t h, uint32_t px,
                          uint32_t py, uint32_t sample, uint32_t seed, float *light, uint64_t *counts) {
    int polished_frame, translucent_frame;
    frame_kinds(polish, tr, &polished_frame, &translucent_frame);
    orc_scene no_disc = *scene;
    no_disc.settings.sun_intensity = 0.0f;
    uint32_t id = 0;
    for (int i = 0; i < LAMP_COUNTS; i++) counts[i] = 0;
    const v3 l = trace_path_lamp(scene, &no_disc, emission, polish, tr, polished_frame, translucent_frame, sun_strength, cs, ll, list, N, px, py,
                                 path_seed(px, py, w, h, sample, seed), &id, counts, NULL, NULL, 0);
    light[0] = l.x; light[1] = l.y; light[2] = l.z;
}

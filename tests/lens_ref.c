/* tests/lens_ref.c — the path trace with camera sampling (include/vrt.h: vrt_set_camera_sampling) on top of direct sunlight and
 * the per-material emission, polish and translucency tables, for the tests.  TEST INFRASTRUCTURE ONLY: compiled by
 * tests/lens_ref.py with oracle/Makefile's CFLAGS into a temporary directory.
 *
 * tests/sun_ref.c's loop with steps 1 to 5 of vrt_set_camera_sampling's contract in front of it: with pixel_spread or aperture
 * not 0 every sample takes four draws ahead of everything else and builds a primary ray of its own from them — a point of the
 * pixel's box, a point of the lens — which is marched as an ordinary segment; the id word is the one of the pixel's own pinhole
 * ray, marched once more per frame.  With both 0 the loop is sun_ref.c's.  The ray is written out here operation for operation
 * (not taken from csrc/both/lens_math.h: tests/test_lens_ref.py holds that text to this one).  Compiled without contraction. */
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

typedef struct {   /* include/vrt.h: vrt_camera_sampling */
    float pixel_spread;
    float aperture;
    float focus_distance;
    uint32_t flags;
} ref_camera_sampling;

/* steps: the lookups of every march, the centre ray's included; bounce segments: the segments behind the primary ones; sun rays
 * marched; jitter_changed: samples whose own primary id word is not the centre ray's; lens_moved: samples with o' != origin */
enum { LENS_STEPS, LENS_BOUNCE_SEGMENTS, LENS_SUN_RAYS, LENS_JITTER_CHANGED, LENS_MOVED, LENS_COUNTS };

/* translucent_ref.c's exit: how far along dir the unit voxel of pos ends on one axis */
static float exit_t(float pos, float dir) {
    const float c = floorf(pos);
    const float far = dir > 0.0f ? c + 1.0f : c;
    return dir != 0.0f ? (far - pos) / dir : INFINITY;
}

/* steps 2 and 3: the sample's primary ray from its four draws.  to_focus: what d' is the normalisation of (w itself for a pinhole) */
static void lens_ray(const orc_scene *s, const ref_camera_sampling *cs, uint32_t px, uint32_t py, const float u[4], v3 *o, v3 *d, v3 *w_out,
                     v3 *to_focus) {
    const orc_cam_data *c = &s->cam;
    const float fx = (float)px + (u[0] - 0.5f) * cs->pixel_spread;
    const float fy = (float)py + (u[1] - 0.5f) * cs->pixel_spread;
    const float x = (fx * 2.0f) / c->proj_size[0] - 1.0f;
    const float y = (fy * 2.0f) / c->proj_size[1] - 1.0f;
    const float clip[4] = {x, -y, -1.0f, 1.0f};
    float e0[2];
    for (int i = 0; i < 2; i++) {
        const float *col = &c->inv_proj_mat[i * 4];
        e0[i] = clip[0] * col[0] + clip[1] * col[1] + clip[2] * col[2] + clip[3] * col[3];
    }
    const float eye[4] = {e0[0], e0[1], -1.0f, 0.0f};
    float w[3];
    for (int i = 0; i < 3; i++) {
        const float *col = &c->inv_view_mat[i * 4];
        w[i] = eye[0] * col[0] + eye[1] * col[1] + eye[2] * col[2] + eye[3] * col[3];
    }
    const v3 origin = V3(c->pos[0] - (float)s->world.min[0], c->pos[1] - (float)s->world.min[1], c->pos[2] - (float)s->world.min[2]);
    *w_out = V3(w[0], w[1], w[2]);
    *d = orc_normalize(*w_out);
    *o = origin;
    *to_focus = *w_out;
    if (cs->aperture != 0.0f) {
        const float r = cs->aperture * sqrtf(u[2]);
        const float lx = r * orc_cos2pi(u[3]);
        const float ly = r * orc_cos2pi(u[3] + 0.75f);
        const float *iv = c->inv_view_mat;
        const v3 F = V3(origin.x + d->x * cs->focus_distance, origin.y + d->y * cs->focus_distance, origin.z + d->z * cs->focus_distance);
        *o = V3((origin.x + iv[0] * lx) + iv[1] * ly, (origin.y + iv[4] * lx) + iv[5] * ly, (origin.z + iv[8] * lx) + iv[9] * ly);
        *to_focus = V3(F.x - o->x, F.y - o->y, F.z - o->z);
        *d = orc_normalize(*to_focus);
    }
}

/* one sample: its light; *id: the id word of ITS primary segment */
static v3 trace_path_lens(const orc_scene *s, const orc_scene *s_no_disc, const float *emission, const ref_polish *polish,
                          const ref_translucency *tr, int polished_frame, int translucent_frame, float strength, const ref_camera_sampling *cs,
                          uint32_t px, uint32_t py, uint32_t rng, uint32_t *id, uint64_t *n) {
    v3 light = V3(0.0f, 0.0f, 0.0f);
    v3 origin, dir;
    if (cs->pixel_spread != 0.0f || cs->aperture != 0.0f) {   /* step 1: four draws, whichever of the two is 0 */
        float u[4];
        for (int i = 0; i < 4; i++) u[i] = orc_rng_next(&rng);
        v3 cam, cdir, w, v;
        create_ray_from_screen(s, (int32_t)px, (int32_t)py, &cam, &cdir);
        lens_ray(s, cs, px, py, u, &origin, &dir, &w, &v);
        if (origin.x != cam.x || origin.y != cam.y || origin.z != cam.z) n[LENS_MOVED] += 1u;
    } else {
        create_ray_from_screen(s, (int32_t)px, (int32_t)py, &origin, &dir);
    }
    v3 thr = V3(1.0f, 1.0f, 1.0f);
    const int sun_lit = strength != 0.0f;
    for (uint32_t bounce = 0; bounce < s->settings.max_ray_bounces; bounce++) {
        hit_result rs = ray_world(s, origin, dir);
        n[LENS_STEPS] += rs.iter_count;
        if (bounce != 0) n[LENS_BOUNCE_SEGMENTS] += 1u;
        if (bounce == 0) *id = id_word(&rs);
        if (!rs.hit) {
            v3 sky = ray_sky(s, origin, dir);
            if (sun_lit && bounce != 0) {   /* step 4: add = +0 */
                sky = ray_sky(s_no_disc, origin, dir);
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
                n[LENS_SUN_RAYS] += 1u;
                n[LENS_STEPS] += sh.iter_count;
                if (!sh.hit) {
                    const float k = s->settings.sun_intensity * strength;
                    const float w = k * c;
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

static void frame_kinds(const ref_polish *polish, const ref_translucency *tr, int *polished_frame, int *translucent_frame) {
    *polished_frame = *translucent_frame = 0;
    for (uint32_t i = 0; i < 256u; i++) {
        *polished_frame |= polish[i].chance != 0.0f;
        *translucent_frame |= tr[i].chance != 0.0f;
    }
}

/* A w x h path-trace frame of samples sample_base .. sample_base + spp - 1 (seeded as orc_render seeds sample s), their mean
 * in rgb[h][w][3], the id word of the pixel's own pinhole ray in ids[h][w]; counts[LENS_COUNTS] as the enum says.  With the
 * setting on, the centre ray is marched once per pixel for the id word (step 5) and its lookups are counted.  Like orc_render,
 * pixels beyond the last whole 8 x 8 tile are not traced: the caller passes zeroed arrays. */
void ref_render_path_lens(const orc_scene *scene, const float *emission, const ref_polish *polish, const ref_translucency *tr, float strength,
                          const ref_camera_sampling *cs, uint32_t w, uint32_t h, uint32_t spp, uint32_t seed, uint32_t sample_base, float *rgb,
                          uint32_t *ids, uint64_t *counts) {
    const uint32_t x1 = w & ~7u, y1 = h & ~7u, nspp = spp ? spp : 1u;
    const int on = cs->pixel_spread != 0.0f || cs->aperture != 0.0f;
    int polished_frame, translucent_frame;
    frame_kinds(polish, tr, &polished_frame, &translucent_frame);
    orc_scene no_disc = *scene;
    no_disc.settings.sun_intensity = 0.0f;
    uint64_t n0 = 0, n1 = 0, n2 = 0, n3 = 0, n4 = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : n0, n1, n2, n3, n4)
    for (int32_t py = 0; py < (int32_t)y1; py++) {
        for (uint32_t px = 0; px < x1; px++) {
            const size_t o = (size_t)py * w + px;
            v3 sum = V3(0.0f, 0.0f, 0.0f);
            uint32_t id = 0;
            if (on && scene->settings.max_ray_bounces > 0u) {   /* step 5: the pixel's own ray, shaded by nobody */
                v3 origin, dir;
                create_ray_from_screen(scene, (int32_t)px, py, &origin, &dir);
                const hit_result rc = ray_world(scene, origin, dir);
                n0 += rc.iter_count;
                id = id_word(&rc);
            }
            for (uint32_t sm = 0; sm < nspp; sm++) {
                uint32_t sid = 0;
                uint64_t n[LENS_COUNTS] = {0, 0, 0, 0, 0};
                v3 l = trace_path_lens(scene, &no_disc, emission, polish, tr, polished_frame, translucent_frame, strength, cs, px, (uint32_t)py,
                                       path_seed(px, (uint32_t)py, w, h, sample_base + sm, seed), &sid, n);
                sum.x += l.x; sum.y += l.y; sum.z += l.z;
                if (on && scene->settings.max_ray_bounces > 0u && sid != id) n[LENS_JITTER_CHANGED] += 1u;
                n0 += n[0]; n1 += n[1]; n2 += n[2]; n3 += n[3]; n4 += n[4];
                if (!on && sm == 0) id = sid;
            }
            rgb[o * 3 + 0] = sum.x / (float)nspp;
            rgb[o * 3 + 1] = sum.y / (float)nspp;
            rgb[o * 3 + 2] = sum.z / (float)nspp;
            ids[o] = id;
        }
    }
    counts[LENS_STEPS] = n0; counts[LENS_BOUNCE_SEGMENTS] = n1; counts[LENS_SUN_RAYS] = n2; counts[LENS_JITTER_CHANGED] = n3; counts[LENS_MOVED] = n4;
}

/* the reference's ray of one sample from given draws: out = w (step 2's direction before it is normalised), o', F - o' (w for a
 * pinhole), d' */
void ref_lens_ray(const orc_scene *scene, const ref_camera_sampling *cs, uint32_t px, uint32_t py, const float *u, float *out) {
    v3 o, d, w, v;
    lens_ray(scene, cs, px, py, u, &o, &d, &w, &v);
    const float r[12] = {w.x, w.y, w.z, o.x, o.y, o.z, v.x, v.y, v.z, d.x, d.y, d.z};
    memcpy(out, r, sizeof r);
}

/* one pixel's one sample: its light, the id word of its own primary segment, and the draws u1..u4 its ray was built from */
void ref_trace_pixel_lens(const orc_scene *scene, const float *emission, const ref_polish *polish, const ref_translucency *tr, float strength,
                          const ref_camera_sampling *cs, uint32_t w, uint32_t h, uint32_t px, uint32_t py, uint32_t sample, uint32_t seed, float *light,
                          uint32_t *id, float *u) {
    int polished_frame, translucent_frame;
    frame_kinds(polish, tr, &polished_frame, &translucent_frame);
    orc_scene no_disc = *scene;
    no_disc.settings.sun_intensity = 0.0f;
    uint64_t n[LENS_COUNTS] = {0, 0, 0, 0, 0};
    uint32_t rng = path_seed(px, py, w, h, sample, seed);
    for (int i = 0; i < 4; i++) u[i] = orc_rng_next(&rng);
    const v3 l = trace_path_lens(scene, &no_disc, emission, polish, tr, polished_frame, translucent_frame, strength, cs, px, py,
                                 path_seed(px, py, w, h, sample, seed), id, n);
    light[0] = l.x; light[1] = l.y; light[2] = l.z;
}

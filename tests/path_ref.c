/* tests/path_ref.c — the path trace with every term include/vrt.h adds to it, for the tests: the per-material emission, polish
 * and translucency tables (vrt_write_emission, vrt_write_polish, vrt_write_translucency), direct sunlight (vrt_set_sun_light),
 * camera sampling (vrt_set_camera_sampling) and lamp light (vrt_set_lamp_light).  TEST INFRASTRUCTURE ONLY: compiled by
 * tests/path_ref.py with oracle/Makefile's CFLAGS into a temporary directory; tests/emission_ref.py to tests/lamp_ref.py are
 * views of it with the later terms switched off.
 *
 * oracle/vrt_oracle.c's trace_path_into has none of these terms (the live Material has no such field).  trace_path_terms below
 * is its loop with each term where its contract puts it, and with every one of them off it is that loop bit for bit.  The march,
 * the sky and the RNG are the oracle's own functions (this file includes it), so every direction is bit for bit the oracle's and
 * the kernels'.  Compiled without contraction: the arithmetic below is binary32 operation for operation.  A sample's light is
 * its terms in segment order; a frame's, its samples' lights summed in sample order and divided by spp. */
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

/* What a frame or a sample counts (tests/path_ref.py: Counts, in this order).  steps: the lookups of every march — path segments,
 * sun rays, lamp rays and, with camera sampling on, the centre ray's; bounce segments: the segments behind the primary ones; the
 * sun rays marched and the unoccluded ones; the later segments' misses through the sun's disc; the lamp rays marched and those
 * that arrived; emissive hits whose term was dropped because their path had bounced; bounces off a coat; passes through a voxel;
 * jitter_changed: samples whose own primary id word is not the centre ray's; lens_moved: samples with o' != origin */
enum { N_STEPS, N_BOUNCE_SEGMENTS, N_SUN_RAYS, N_SUN_UNOCCLUDED, N_DISC_MISSES, N_LAMP_RAYS, N_LAMP_UNOCCLUDED, N_EMISSION_DROPPED, N_POLISHED,
       N_PASSES, N_JITTER_CHANGED, N_LENS_MOVED, N_COUNTS };

/* what a segment of a sample hands to the launches behind it, where the caller asks for load planes: the path goes on into the
 * next segment (it hit, and this was not its last allowed segment); a sun ray was marched from the hit; a lamp ray was */
enum { LOAD_PATH = 1, LOAD_SUN = 2, LOAD_LAMP = 4 };

typedef struct {
    const orc_scene *scene, *no_disc;   /* no_disc: a copy whose sun_intensity is 0 */
    const float *emission;
    const ref_polish *polish;
    const ref_translucency *tr;
    int polished_frame, translucent_frame;   /* some entry's chance is not 0 */
    float sun_strength;
    const ref_camera_sampling *cs;
    const ref_lamp_light *ll;
    const ref_lamp *list;
    uint32_t N;
} path_settings;

static path_settings settings_of(const orc_scene *scene, orc_scene *no_disc, const float *emission, const ref_polish *polish,
                                 const ref_translucency *tr, float sun_strength, const ref_camera_sampling *cs, const ref_lamp_light *ll,
                                 const ref_lamp *list, uint32_t N) {
    path_settings p = {scene, no_disc, emission, polish, tr, 0, 0, sun_strength, cs, ll, list, N};
    for (uint32_t i = 0; i < 256u; i++) {
        p.polished_frame |= polish[i].chance != 0.0f;
        p.translucent_frame |= tr[i].chance != 0.0f;
    }
    *no_disc = *scene;
    no_disc->settings.sun_intensity = 0.0f;
    return p;
}

/* vrt_write_translucency step 5's exit: how far along dir the unit voxel of pos ends on one axis */
static float exit_t(float pos, float dir) {
    const float c = floorf(pos);
    const float far = dir > 0.0f ? c + 1.0f : c;
    return dir != 0.0f ? (far - pos) / dir : INFINITY;
}

static float comp(v3 v, uint32_t a) { return a == 0u ? v.x : (a == 1u ? v.y : v.z); }

/* vrt_set_camera_sampling steps 2 and 3: the sample's primary ray from its four draws — a point of the pixel's box, a point of
 * the lens.  to_focus: what d' is the normalisation of (w itself for a pinhole).  Written out here operation for operation, not
 * taken from csrc/both/lens_math.h: tests/test_lens_ref.py holds that text to this one. */
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

/* One sample: its light; *id: the id word of ITS primary segment; n[N_COUNTS] grows.  arrived: NULL, or per list entry the lamp rays
 * that arrived at it; load: NULL, or the sample's LOAD_ bits, segment b's at load[b * load_stride]. */
static v3 trace_path_terms(const path_settings *p, uint32_t px, uint32_t py, uint32_t rng, uint32_t *id, uint64_t *n, uint32_t *arrived,
                           uint8_t *load, size_t load_stride) {
    const orc_scene *s = p->scene;
    v3 light = V3(0.0f, 0.0f, 0.0f);
    v3 origin, dir;
    create_ray_from_screen(s, (int32_t)px, (int32_t)py, &origin, &dir);
    if (p->cs->pixel_spread != 0.0f || p->cs->aperture != 0.0f) {
        /* vrt_set_camera_sampling step 1: four draws ahead of everything else, whichever of the two is 0, and a primary ray of the
         * sample's own from them, marched as an ordinary segment */
        const v3 cam = origin;
        float u[4];
        for (int i = 0; i < 4; i++) u[i] = orc_rng_next(&rng);
        v3 w, v;
        lens_ray(s, p->cs, px, py, u, &origin, &dir, &w, &v);
        if (origin.x != cam.x || origin.y != cam.y || origin.z != cam.z) n[N_LENS_MOVED] += 1u;
    }
    v3 thr = V3(1.0f, 1.0f, 1.0f);
    const int sun_lit = p->sun_strength != 0.0f, lamp_lit = p->ll->strength != 0.0f;
    int direct = 1;   /* no bounce yet: passes leave it so */
    for (uint32_t bounce = 0; bounce < s->settings.max_ray_bounces; bounce++) {
        hit_result rs = ray_world(s, origin, dir);
        n[N_STEPS] += rs.iter_count;
        if (bounce != 0) n[N_BOUNCE_SEGMENTS] += 1u;
        if (bounce == 0) *id = id_word(&rs);
        if (!rs.hit) {
            v3 sky = ray_sky(s, origin, dir);
            if (sun_lit && bounce != 0) {
                /* vrt_set_sun_light step 4: a segment other than the primary that misses takes the sky without the disc (add = +0),
                 * so the disc is not counted twice */
                const v3 plain = ray_sky(p->no_disc, origin, dir);
                if (plain.x != sky.x || plain.y != sky.y || plain.z != sky.z) n[N_DISC_MISSES] += 1u;
                sky = plain;
            }
            light.x += sky.x * thr.x;
            light.y += sky.y * thr.y;
            light.z += sky.z * thr.z;
            break;
        }
        const v3 so = V3(rs.pos.x + rs.norm.x * ORC_SHADOW_BIAS, rs.pos.y + rs.norm.y * ORC_SHADOW_BIAS, rs.pos.z + rs.norm.z * ORC_SHADOW_BIAS);   /* the bounce origin */
        const uint32_t entry = rs.voxel > 255u ? 255u : rs.voxel;
        /* path_tracer.wgsl:183-184, vrt_write_emission: (mc * e) * thr per channel before thr *= mc — mc the hit's colour (rs.color:
         * face shading, the step-count grey), thr the throughput before the hit.  vrt_set_lamp_light step 2: with lamp light on,
         * only while the path is direct — behind a bounce the lamp rays have already brought that light */
        const float e = p->emission[entry];
        if (e != 0.0f) {
            if (!lamp_lit || direct) {
                light.x += (rs.color.x * e) * thr.x;
                light.y += (rs.color.y * e) * thr.y;
                light.z += (rs.color.z * e) * thr.z;
            } else {
                n[N_EMISSION_DROPPED] += 1u;
            }
        }
        if (sun_lit && is_solid_hit(s, &rs)) {
            /* vrt_set_sun_light step 2: every hit on a solid voxel — the primary segment's and the last allowed segment's included —
             * whose face looks at the sun sends a ray there from the bounce origin (shadow_ray's origin and direction), and where
             * it does not hit, (mc * (k * c)) * thr joins the light right behind the emission term.  It draws nothing. */
            const v3 sd = orc_normalize(V3(s->settings.sun_pos[0] - (float)s->world.min[0] - so.x,
                                           s->settings.sun_pos[1] - (float)s->world.min[1] - so.y,
                                           s->settings.sun_pos[2] - (float)s->world.min[2] - so.z));
            const float c = orc_dot(rs.norm, sd);
            if (c > 0.0f) {
                const hit_result sh = ray_world(s, so, sd);
                n[N_SUN_RAYS] += 1u;
                if (load) load[bounce * load_stride] |= LOAD_SUN;
                n[N_STEPS] += sh.iter_count;
                if (!sh.hit) {
                    const float k = s->settings.sun_intensity * p->sun_strength;
                    const float w = k * c;
                    n[N_SUN_UNOCCLUDED] += 1u;
                    light.x += (rs.color.x * w) * thr.x;
                    light.y += (rs.color.y * w) * thr.y;
                    light.z += (rs.color.z * w) * thr.z;
                }
            }
        }
        if (lamp_lit) {
            /* vrt_set_lamp_light step 4: three draws on every hit, the last allowed segment's too, ahead of every other draw of the
             * hit; step 5: a ray from the bounce origin to a point of a face of the lamp list */
            const float u1 = orc_rng_next(&rng), u2 = orc_rng_next(&rng), u3 = orc_rng_next(&rng);
            if (is_solid_hit(s, &rs) && p->N > 0u) {
                uint32_t j = (uint32_t)(u1 * (float)p->N);
                if (j > p->N - 1u) j = p->N - 1u;
                const ref_lamp *L = &p->list[j];
                const uint32_t a = L->face >> 1, side = L->face & 1u;
                float q[3];
                q[a] = (float)L->pos[a] + (float)side;
                const uint32_t b = a == 0u ? 1u : 0u, c2 = a == 2u ? 1u : 2u;
                q[b] = (float)L->pos[b] + u2;
                q[c2] = (float)L->pos[c2] + u3;
                const v3 v = V3(q[0] - so.x, q[1] - so.y, q[2] - so.z);
                const float d2 = (v.x * v.x + v.y * v.y) + v.z * v.z;
                const v3 ld = orc_normalize(v);
                const float c = orc_dot(rs.norm, ld);
                const float cl = side ? -comp(ld, a) : comp(ld, a);
                if (c > 0.0f && cl > 0.0f) {
                    const hit_result lh = ray_world(s, so, ld);
                    n[N_LAMP_RAYS] += 1u;
                    if (load) load[bounce * load_stride] |= LOAD_LAMP;
                    n[N_STEPS] += lh.iter_count;
                    const int unoccluded = lh.hit && (int)floorf(lh.pos.x) == (int)L->pos[0] && (int)floorf(lh.pos.y) == (int)L->pos[1] &&
                                           (int)floorf(lh.pos.z) == (int)L->pos[2];
                    float g = (c * cl) / d2;
                    if (p->ll->max_geometry != 0.0f && g > p->ll->max_geometry) g = p->ll->max_geometry;
                    const uint32_t lentry = L->voxel > 255u ? 255u : L->voxel;
                    const float k = ((p->ll->strength * p->emission[lentry]) * 0.318309886f) * (float)p->N;
                    const float w = k * g;
                    const orc_material *lm = mat_at(s, L->voxel);
                    v3 lc = V3(lm->color[0], lm->color[1], lm->color[2]);   /* the lamp face's own shading */
                    if (a == 0u) { lc.x *= 0.5f; lc.y *= 0.5f; lc.z *= 0.5f; }
                    if (a == 2u) { lc.x *= 0.7f; lc.y *= 0.7f; lc.z *= 0.7f; }
                    if (L->face == 2u) { lc.x *= 0.2f; lc.y *= 0.2f; lc.z *= 0.2f; }
                    if (unoccluded) {
                        n[N_LAMP_UNOCCLUDED] += 1u;
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
        /* The last allowed segment: the next direction and throughput are observed by nothing, so nothing below is drawn.  (The
         * oracle's loop and path_tracer.wgsl go on to compute them; no output can tell.) */
        if (bounce + 1 == s->settings.max_ray_bounces) break;
        if (load) load[bounce * load_stride] |= LOAD_PATH;
        if (p->translucent_frame && orc_rng_next(&rng) < p->tr[entry].chance) {
            /* vrt_write_translucency steps 3 to 5: in a translucent frame every hit after which the path may go on draws ut ahead of
             * the coat's draw and the direction's six, and where ut < the entry's chance the path passes: no further draw, thr *=
             * the entry's colour as written, dir unchanged, the origin moved across the one unit voxel that holds the hit position
             * in the form the march advances across an air node.  The path stays direct. */
            const float tx = exit_t(rs.pos.x, dir.x), ty = exit_t(rs.pos.y, dir.y), tz = exit_t(rs.pos.z, dir.z);
            float t = tx;
            if (ty < t) t = ty;
            if (tz < t) t = tz;
            const float ts = t + 0.001f;
            thr.x *= p->tr[entry].color[0]; thr.y *= p->tr[entry].color[1]; thr.z *= p->tr[entry].color[2];
            origin = V3(rs.pos.x + dir.x * ts, rs.pos.y + dir.y * ts, rs.pos.z + dir.z * ts);
            n[N_PASSES] += 1u;
            continue;
        }
        direct = 0;   /* the first bounce */
        /* vrt_write_polish, path_tracer.wgsl:175, :180 and :185: in a polished frame one draw u ahead of rng_next_dir's six (:178),
         * and where u < the entry's chance, the entry's scatter in place of the material's and the entry's colour, as written, in
         * place of mc in thr *= mc.  Both are selects. */
        int polished = 0;
        if (p->polished_frame) polished = orc_rng_next(&rng) < p->polish[entry].chance;
        float d = orc_dot(rs.norm, dir);
        v3 spec = V3(dir.x - 2.0f * rs.norm.x * d, dir.y - 2.0f * rs.norm.y * d, dir.z - 2.0f * rs.norm.z * d);
        v3 rd = rng_next_dir(&rng);
        v3 sc = orc_normalize(V3(rs.norm.x + rd.x, rs.norm.y + rd.y, rs.norm.z + rd.z));
        float scatter = polished ? p->polish[entry].scatter : mat_at(s, rs.voxel)->scatter;
        v3 nd = orc_normalize(V3(orc_mix(spec.x, sc.x, scatter), orc_mix(spec.y, sc.y, scatter), orc_mix(spec.z, sc.z, scatter)));
        v3 tint = polished ? V3(p->polish[entry].color[0], p->polish[entry].color[1], p->polish[entry].color[2]) : rs.color;
        thr.x *= tint.x; thr.y *= tint.y; thr.z *= tint.z;
        origin = so;
        dir = nd;
        n[N_POLISHED] += polished ? 1u : 0u;
    }
    return light;
}

/* A w x h path-trace frame of samples sample_base .. sample_base + spp - 1 (seeded as orc_render seeds sample s), their mean in
 * rgb[h][w][3], the id word of the pixel's own pinhole ray in ids[h][w], counts[N_COUNTS] as the enum says.  With camera sampling
 * on, the centre ray is marched once per pixel for the id word (vrt_set_camera_sampling step 5) and its lookups are counted; with
 * it off, the id word is the first sample's primary segment's.  arrived: NULL, or N words that the frame adds to: per list entry,
 * the lamp rays that arrived at it unoccluded.  load: NULL, or load[spp][max_ray_bounces][h][w] bytes, zero on entry: the LOAD_
 * bits of segment b of sample s of pixel (x, y).  Like orc_render, pixels beyond the last whole 8 x 8 tile are not traced: the
 * caller passes zeroed arrays. */
void ref_render_path(const orc_scene *scene, const float *emission, const ref_polish *polish, const ref_translucency *tr, float sun_strength,
                     const ref_camera_sampling *cs, const ref_lamp_light *ll, const ref_lamp *list, uint32_t N, uint32_t w, uint32_t h, uint32_t seed,
                     uint32_t spp, uint32_t sample_base, float *rgb, uint32_t *ids, uint64_t *counts, uint32_t *arrived, uint8_t *load) {
    const size_t plane = (size_t)w * h;
    const uint32_t x1 = w & ~7u, y1 = h & ~7u, nspp = spp ? spp : 1u;
    const int centre = (cs->pixel_spread != 0.0f || cs->aperture != 0.0f) && scene->settings.max_ray_bounces > 0u;
    orc_scene no_disc;
    const path_settings p = settings_of(scene, &no_disc, emission, polish, tr, sun_strength, cs, ll, list, N);
    uint64_t n[N_COUNTS] = {0};
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : n[:N_COUNTS])
    for (int32_t py = 0; py < (int32_t)y1; py++) {
        for (uint32_t px = 0; px < x1; px++) {
            const size_t o = (size_t)py * w + px;
            v3 sum = V3(0.0f, 0.0f, 0.0f);
            uint32_t id = 0;
            if (centre) {   /* the pixel's own ray, shaded by nobody */
                v3 origin, dir;
                create_ray_from_screen(scene, (int32_t)px, py, &origin, &dir);
                const hit_result rc = ray_world(scene, origin, dir);
                n[N_STEPS] += rc.iter_count;
                id = id_word(&rc);
            }
            for (uint32_t sm = 0; sm < nspp; sm++) {
                uint32_t sid = 0;
                v3 l = trace_path_terms(&p, px, (uint32_t)py, path_seed(px, (uint32_t)py, w, h, sample_base + sm, seed), &sid, n, arrived,
                                  load ? load + ((size_t)sm * scene->settings.max_ray_bounces) * plane + o : NULL, plane);
                sum.x += l.x; sum.y += l.y; sum.z += l.z;
                if (centre && sid != id) n[N_JITTER_CHANGED] += 1u;
                if (!centre && sm == 0) id = sid;
            }
            rgb[o * 3 + 0] = sum.x / (float)nspp;
            rgb[o * 3 + 1] = sum.y / (float)nspp;
            rgb[o * 3 + 2] = sum.z / (float)nspp;
            ids[o] = id;
        }
    }
    memcpy(counts, n, sizeof n);
}

/* one pixel's one sample: its light, the id word of its own primary segment, the first four draws of its stream (what its ray is
 * built from when camera sampling is on) and its counts */
void ref_trace_pixel(const orc_scene *scene, const float *emission, const ref_polish *polish, const ref_translucency *tr, float sun_strength,
                     const ref_camera_sampling *cs, const ref_lamp_light *ll, const ref_lamp *list, uint32_t N, uint32_t w, uint32_t h, uint32_t seed,
                     uint32_t px, uint32_t py, uint32_t sample, float *light, uint32_t *id, float *u, uint64_t *counts) {
    orc_scene no_disc;
    const path_settings p = settings_of(scene, &no_disc, emission, polish, tr, sun_strength, cs, ll, list, N);
    uint32_t rng = path_seed(px, py, w, h, sample, seed);
    for (int i = 0; i < 4; i++) u[i] = orc_rng_next(&rng);
    memset(counts, 0, N_COUNTS * sizeof *counts);
    *id = 0;
    const v3 l = trace_path_terms(&p, px, py, path_seed(px, py, w, h, sample, seed), id, counts, NULL, NULL, 0);
    light[0] = l.x; light[1] = l.y; light[2] = l.z;
}

/* the ray of one sample from given draws: out = w (step 2's direction before it is normalised), o', F - o' (w for a pinhole), d' */
void ref_lens_ray(const orc_scene *scene, const ref_camera_sampling *cs, uint32_t px, uint32_t py, const float *u, float *out) {
    v3 o, d, w, v;
    lens_ray(scene, cs, px, py, u, &o, &d, &w, &v);
    const float r[12] = {w.x, w.y, w.z, o.x, o.y, o.z, v.x, v.y, v.z, d.x, d.y, d.z};
    memcpy(out, r, sizeof r);
}

/* the voxel id of every unit voxel of the world, dense[z][y][x], by the oracle's own walk: what tests/lamp_ref.py makes the lamp
 * list from */
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

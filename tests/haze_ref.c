/* tests/haze_ref.c — the path trace with haze (vrt_set_haze, include/vrt.h), for the tests: the contract's steps on top of the
 * emission, polish and translucency tables and direct sunlight.  TEST INFRASTRUCTURE ONLY: compiled by tests/haze_ref.py with
 * oracle/Makefile's CFLAGS into a temporary directory.
 *
 * tests/path_ref.c's loop is a static function without a hook between its march and what follows it, so the loop is restated here
 * with camera sampling, lamp light and water left out (a haze frame has none of them).  The march, the sky, the RNG and
 * rng_next_dir are the oracle's own functions (this file includes it).  The logarithm, the distance and the exit from the world box
 * are written out again here in this file's own words, not taken from csrc/both/haze_math.h: tests/test_haze_ref.py holds the
 * library's exports to them value for value.  Compiled without contraction.  With the setting off (density == 0) the loop is
 * path_ref.c's with those terms off: tests/test_haze_ref.py holds it to that. */
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

typedef struct {   /* include/vrt.h: vrt_haze */
    float density;
    float albedo[3];
    uint32_t flags;
    uint32_t _reserved[3];
} ref_haze;

/* What a frame or a sample counts (tests/haze_ref.py: Counts, in this order).  steps: the lookups of every march, path segments and
 * sun rays; bounce segments: the segments behind the primary ones (a scatter event's continuation is one); sun rays: every one
 * marched, a hit's or an event's; scatter events on primary segments, on later ones, and — counted in those two as well — on the
 * last allowed segment; events on segments whose march hit and on segments whose march missed; the sun rays events sent and how many
 * of those were unoccluded; segments without an event; passes through a translucent voxel; bounces off a coat */
enum { N_STEPS, N_BOUNCE_SEGMENTS, N_SUN_RAYS, N_SUN_UNOCCLUDED, N_EV_PRIMARY, N_EV_LATER, N_EV_LAST, N_EV_HIT, N_EV_MISS, N_EV_SUN_RAYS,
       N_EV_SUN_UNOCCLUDED, N_NO_EVENT, N_PASSES, N_POLISHED, N_COUNTS };

/* ln(x): x = m * 2^e, m in (sqrt(1/2), sqrt(2)]; ln m = 2 atanh(s), s = (m - 1) / (m + 1), atanh's series up to s^11 */
static float hz_log(float x) {
    const uint32_t bits = orc_f2bits(x);
    int32_t e = (int32_t)(bits >> 23) - 127;
    float m = orc_bits2f((bits & 0x007FFFFFu) | 0x3F800000u);
    if (m > 1.41421354f) {
        m = m * 0.5f;
        e = e + 1;
    }
    const float s = (m - 1.0f) / (m + 1.0f);
    const float z = s * s;
    float poly = z * 0.0909090936f;
    poly = z * (0.111111112f + poly);
    poly = z * (0.142857149f + poly);
    poly = z * (0.2f + poly);
    poly = z * (0.333333343f + poly);
    return (float)e * 0.693147182f + (s + s * poly) * 2.0f;
}

/* step 2: how far the draw u reaches */
static float hz_distance(float u, float inv) {
    float uc = u;
    if (u < 1.0e-10f) uc = 1.0e-10f;
    const float l = hz_log(uc);
    return (-l) * inv;
}

/* step 3, a miss: where the ray leaves the box (0, world_max)^3; 0 from an origin that is not strictly inside it */
static float hz_exit(const float o[3], const float d[3], float world_max) {
    float L = INFINITY;
    for (int k = 2; k >= 0; k--) {   /* min(e.x, min(e.y, e.z)): z first */
        if (!(o[k] > 0.0f && o[k] < world_max)) return 0.0f;
    }
    for (int k = 2; k >= 0; k--) {
        float e = INFINITY;
        if (d[k] > 0.0f) e = (world_max - o[k]) / d[k];
        else if (d[k] < 0.0f) e = (0.0f - o[k]) / d[k];
        L = fminf(e, L);
    }
    return L;
}

float ref_haze_log(float x) { return hz_log(x); }
float ref_haze_distance(float u, float inv) { return hz_distance(u, inv); }
float ref_haze_exit(const float *o, const float *d, float world_max) { return hz_exit(o, d, world_max); }

typedef struct {
    const orc_scene *scene, *no_disc;   /* no_disc: sun_intensity 0 */
    const float *emission;
    const ref_polish *polish;
    const ref_translucency *tr;
    int polished_frame, translucent_frame;
    float sun_strength;
    const ref_haze *hz;
    float inv;
} haze_settings;

static float exit_t(float pos, float dir) {
    const float c = floorf(pos);
    const float far = dir > 0.0f ? c + 1.0f : c;
    return dir != 0.0f ? (far - pos) / dir : INFINITY;
}

static v3 sun_dir_from(const orc_scene *s, v3 p) {
    return orc_normalize(V3(s->settings.sun_pos[0] - (float)s->world.min[0] - p.x, s->settings.sun_pos[1] - (float)s->world.min[1] - p.y,
                            s->settings.sun_pos[2] - (float)s->world.min[2] - p.z));
}

/* One sample: its light; *id: the id word of its primary segment's own march; n[N_COUNTS] grows; ev: NULL, or the sample's event
 * flags, ev[b * ev_stride] = 1 where segment b ended in a scatter event. */
static v3 trace_path_haze(const haze_settings *p, uint32_t px, uint32_t py, uint32_t rng, uint32_t *id, uint64_t *n, uint8_t *ev, size_t ev_stride) {
    const orc_scene *s = p->scene;
    const int on = p->hz->density != 0.0f;
    const float world_max = (float)s->world.size;
    v3 light = V3(0.0f, 0.0f, 0.0f);
    v3 origin, dir;
    create_ray_from_screen(s, (int32_t)px, (int32_t)py, &origin, &dir);
    v3 thr = V3(1.0f, 1.0f, 1.0f);
    const int sun_lit = p->sun_strength != 0.0f;
    const uint32_t last = s->settings.max_ray_bounces - 1u;
    for (uint32_t bounce = 0; bounce < s->settings.max_ray_bounces; bounce++) {
        /* step 1: the march, unchanged */
        const hit_result rs = ray_world(s, origin, dir);
        n[N_STEPS] += rs.iter_count;
        if (bounce != 0) n[N_BOUNCE_SEGMENTS] += 1u;
        if (bounce == 0) *id = id_word(&rs);
        if (on) {
            /* steps 2 and 3 */
            const float t = hz_distance(orc_rng_next(&rng), p->inv);
            const float o[3] = {origin.x, origin.y, origin.z}, d[3] = {dir.x, dir.y, dir.z};
            float L;
            if (rs.hit) {
                const v3 v = V3(rs.pos.x - origin.x, rs.pos.y - origin.y, rs.pos.z - origin.z);
                L = sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z);
                for (int k = 0; k < 3; k++)
                    if (!(o[k] > 0.0f && o[k] < world_max)) L = 0.0f;   /* the origin ray_world treats as outside (a NaN too) */
            } else {
                L = hz_exit(o, d, world_max);
            }
            if (t < L) {
                /* step 4: the scatter event */
                const v3 x = V3(origin.x + dir.x * t, origin.y + dir.y * t, origin.z + dir.z * t);
                n[bounce == 0 ? N_EV_PRIMARY : N_EV_LATER] += 1u;
                if (bounce == last) n[N_EV_LAST] += 1u;
                n[rs.hit ? N_EV_HIT : N_EV_MISS] += 1u;
                if (ev) ev[bounce * ev_stride] = 1u;
                if (sun_lit) {
                    const v3 sd = sun_dir_from(s, x);
                    const float q = (sd.x * sd.x + sd.y * sd.y) + sd.z * sd.z;
                    if (q > 0.5f) {
                        const hit_result sh = ray_world(s, x, sd);
                        n[N_SUN_RAYS] += 1u;
                        n[N_EV_SUN_RAYS] += 1u;
                        n[N_STEPS] += sh.iter_count;
                        if (!sh.hit) {
                            const float k = s->settings.sun_intensity * p->sun_strength;
                            const float w = k * 0.25f;
                            n[N_SUN_UNOCCLUDED] += 1u;
                            n[N_EV_SUN_UNOCCLUDED] += 1u;
                            light.x += (p->hz->albedo[0] * w) * thr.x;
                            light.y += (p->hz->albedo[1] * w) * thr.y;
                            light.z += (p->hz->albedo[2] * w) * thr.z;
                        }
                    }
                }
                if (bounce == last) break;
                thr.x *= p->hz->albedo[0]; thr.y *= p->hz->albedo[1]; thr.z *= p->hz->albedo[2];
                dir = rng_next_dir(&rng);
                origin = x;
                continue;
            }
            n[N_NO_EVENT] += 1u;
        }
        /* step 5: path_ref.c's text */
        if (!rs.hit) {
            const v3 sky = ray_sky((sun_lit && bounce != 0) ? p->no_disc : s, origin, dir);
            light.x += sky.x * thr.x;
            light.y += sky.y * thr.y;
            light.z += sky.z * thr.z;
            break;
        }
        const v3 so = V3(rs.pos.x + rs.norm.x * ORC_SHADOW_BIAS, rs.pos.y + rs.norm.y * ORC_SHADOW_BIAS, rs.pos.z + rs.norm.z * ORC_SHADOW_BIAS);
        const uint32_t entry = rs.voxel > 255u ? 255u : rs.voxel;
        const float e = p->emission[entry];
        if (e != 0.0f) {
            light.x += (rs.color.x * e) * thr.x;
            light.y += (rs.color.y * e) * thr.y;
            light.z += (rs.color.z * e) * thr.z;
        }
        if (sun_lit && is_solid_hit(s, &rs)) {
            const v3 sd = sun_dir_from(s, so);
            const float c = orc_dot(rs.norm, sd);
            if (c > 0.0f) {
                const hit_result sh = ray_world(s, so, sd);
                n[N_SUN_RAYS] += 1u;
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
        if (bounce == last) break;
        if (p->translucent_frame && orc_rng_next(&rng) < p->tr[entry].chance) {
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
        int polished = 0;
        if (p->polished_frame) polished = orc_rng_next(&rng) < p->polish[entry].chance;
        const float dn = orc_dot(rs.norm, dir);
        const v3 spec = V3(dir.x - 2.0f * rs.norm.x * dn, dir.y - 2.0f * rs.norm.y * dn, dir.z - 2.0f * rs.norm.z * dn);
        const v3 rd = rng_next_dir(&rng);
        const v3 sc = orc_normalize(V3(rs.norm.x + rd.x, rs.norm.y + rd.y, rs.norm.z + rd.z));
        const float scatter = polished ? p->polish[entry].scatter : mat_at(s, rs.voxel)->scatter;
        const v3 nd = orc_normalize(V3(orc_mix(spec.x, sc.x, scatter), orc_mix(spec.y, sc.y, scatter), orc_mix(spec.z, sc.z, scatter)));
        const v3 tint = polished ? V3(p->polish[entry].color[0], p->polish[entry].color[1], p->polish[entry].color[2]) : rs.color;
        thr.x *= tint.x; thr.y *= tint.y; thr.z *= tint.z;
        origin = so;
        dir = nd;
        n[N_POLISHED] += polished ? 1u : 0u;
    }
    return light;
}

static haze_settings settings_of(const orc_scene *scene, orc_scene *no_disc, const float *emission, const ref_polish *polish, const ref_translucency *tr,
                                 float sun_strength, const ref_haze *hz) {
    haze_settings p = {scene, no_disc, emission, polish, tr, 0, 0, sun_strength, hz, hz->density != 0.0f ? 1.0f / hz->density : 0.0f};
    for (uint32_t i = 0; i < 256u; i++) {
        p.polished_frame |= polish[i].chance != 0.0f;
        p.translucent_frame |= tr[i].chance != 0.0f;
    }
    *no_disc = *scene;
    no_disc->settings.sun_intensity = 0.0f;
    return p;
}

/* A w x h frame of samples sample_base .. sample_base + spp - 1, their mean in rgb[h][w][3], the id word of the first sample's
 * primary segment in ids[h][w], counts[N_COUNTS].  Like orc_render, pixels beyond the last whole 8 x 8 tile are not traced: the
 * caller passes zeroed arrays.  ev: NULL, or ev[spp][max_ray_bounces][h][w] bytes, zero on entry: 1 where the segment scattered. */
void ref_render_haze(const orc_scene *scene, const float *emission, const ref_polish *polish, const ref_translucency *tr, float sun_strength,
                     const ref_haze *hz, uint32_t w, uint32_t h, uint32_t seed, uint32_t spp, uint32_t sample_base, float *rgb, uint32_t *ids,
                     uint64_t *counts, uint8_t *ev) {
    const uint32_t x1 = w & ~7u, y1 = h & ~7u, nspp = spp ? spp : 1u;
    const size_t plane = (size_t)w * h;
    orc_scene no_disc;
    const haze_settings p = settings_of(scene, &no_disc, emission, polish, tr, sun_strength, hz);
    uint64_t n[N_COUNTS] = {0};
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : n[:N_COUNTS])
    for (int32_t py = 0; py < (int32_t)y1; py++) {
        for (uint32_t px = 0; px < x1; px++) {
            const size_t o = (size_t)py * w + px;
            v3 sum = V3(0.0f, 0.0f, 0.0f);
            uint32_t id = 0;
            for (uint32_t sm = 0; sm < nspp; sm++) {
                uint32_t sid = 0;
                const v3 l = trace_path_haze(&p, px, (uint32_t)py, path_seed(px, (uint32_t)py, w, h, sample_base + sm, seed), &sid, n,
                                             ev ? ev + ((size_t)sm * scene->settings.max_ray_bounces) * plane + o : NULL, plane);
                sum.x += l.x; sum.y += l.y; sum.z += l.z;
                if (sm == 0) id = sid;
            }
            rgb[o * 3 + 0] = sum.x / (float)nspp;
            rgb[o * 3 + 1] = sum.y / (float)nspp;
            rgb[o * 3 + 2] = sum.z / (float)nspp;
            ids[o] = id;
        }
    }
    memcpy(counts, n, sizeof n);
}

/* one pixel's one sample: its light, the id word of its primary segment, its counts, and ev[max_ray_bounces]: 1 where the segment
 * scattered (zero on entry) */
void ref_trace_pixel_haze(const orc_scene *scene, const float *emission, const ref_polish *polish, const ref_translucency *tr, float sun_strength,
                          const ref_haze *hz, uint32_t w, uint32_t h, uint32_t seed, uint32_t px, uint32_t py, uint32_t sample, float *light, uint32_t *id,
                          uint64_t *counts, uint8_t *ev) {
    orc_scene no_disc;
    const haze_settings p = settings_of(scene, &no_disc, emission, polish, tr, sun_strength, hz);
    memset(counts, 0, N_COUNTS * sizeof *counts);
    *id = 0;
    const v3 l = trace_path_haze(&p, px, py, path_seed(px, py, w, h, sample, seed), id, counts, ev, 1);
    light[0] = l.x; light[1] = l.y; light[2] = l.z;
}

/* samples sample_base .. sample_base + n - 1 of one pixel, without tables: their counts summed (n may be large: one call) */
void ref_count_pixel_haze(const orc_scene *scene, float sun_strength, const ref_haze *hz, uint32_t w, uint32_t h, uint32_t seed, uint32_t px, uint32_t py,
                          uint32_t sample_base, uint32_t n, uint64_t *counts) {
    static const float emission[256];
    static const ref_polish polish[256];
    static const ref_translucency tr[256];
    orc_scene no_disc;
    const haze_settings p = settings_of(scene, &no_disc, emission, polish, tr, sun_strength, hz);
    memset(counts, 0, N_COUNTS * sizeof *counts);
    for (uint32_t sm = 0; sm < n; sm++) {
        uint32_t id = 0;
        (void)trace_path_haze(&p, px, py, path_seed(px, py, w, h, sample_base + sm, seed), &id, counts, NULL, 0);
    }
}

/* a pixel's primary ray: origin (world-local) and direction */
void ref_primary_ray(const orc_scene *scene, uint32_t px, uint32_t py, float *o, float *d) {
    v3 origin, dir;
    create_ray_from_screen(scene, (int32_t)px, (int32_t)py, &origin, &dir);
    o[0] = origin.x; o[1] = origin.y; o[2] = origin.z;
    d[0] = dir.x; d[1] = dir.y; d[2] = dir.z;
}

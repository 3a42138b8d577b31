/* tests/refract_ref.c — the path trace with water optics and refraction (vrt_set_water_optics + vrt_set_water_refraction,
 * include/vrt.h), for the tests.  TEST INFRASTRUCTURE ONLY: compiled by tests/refract_ref.py with oracle/Makefile's CFLAGS into a
 * temporary directory.
 *
 * tests/water_ref.c's loop restated with A to C of the refraction contract written out again, operation for operation: the two
 * bends, the span walk and the underside event.  Nothing of csrc/both/refract_math.h or csrc/both/cast_dda.h is included: the DDA
 * is restated from the contract and from tests/cast_ray_cases.py's description of cast_ray.  The march, the sky and the RNG are the
 * oracle's own functions, as in water_ref.c.  Compiled without contraction.
 *
 * With ior == 0 the loop is water_ref.c's: tests/test_refract_ref.py holds its frames to that file's bit for bit.  With ior == 1 an
 * entering direction is normalize(d) and an underside event still happens, so such a frame is not the frame with the setting off:
 * it may differ from it in last bits above the water and differs plainly below it. */
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

typedef struct {   /* include/vrt.h: vrt_water_optics */
    float absorb[3];
    float reflectance;
    uint32_t flags;
    uint32_t _reserved[3];
} ref_water_optics;

typedef struct {   /* include/vrt.h: vrt_water_refraction */
    float ior;
    uint32_t max_span;
    uint32_t flags;
    uint32_t _reserved;
} ref_water_refraction;

/* What a frame or a sample counts (tests/refract_ref.py: Counts, in this order; water_ref.c's, then refraction's).  steps: the lookups of every march, path segments
 * and sun rays; bounce segments: the segments behind the primary ones (a surface event's continuation is one); surface events and
 * how many of them reflected and went through; wet segments with water_dist > 0; wet segments that hit; primary segments that
 * start wet with water_dist > 0; bounce segments that start wet; hits on a solid voxel at the end of a wet segment (the bed seen
 * through water) */
enum { N_STEPS, N_BOUNCE_SEGMENTS, N_SUN_RAYS, N_SUN_UNOCCLUDED, N_SURFACE, N_REFLECTED, N_TRANSMITTED, N_WET_W, N_WET_HIT, N_WET_PRIMARY_W,
       N_WET_BOUNCES, N_PASSES, N_POLISHED,
       /* underside events (those on a path's last allowed segment included) and how many of them were totally reflected,
        * reflected by the draw and sent out into the air; entering transmissions bent; walks that ended on a solid voxel, that
        * were still in liquid after max_span steps, that crossed from one liquid id into another; underside events whose air voxel
        * lies where chunk_roots holds no chunk or outside the world box */
       N_UNDER, N_UNDER_TOTAL, N_UNDER_FRESNEL, N_UNDER_OUT, N_BENT, N_WALK_SOLID, N_WALK_CAP, N_WALK_CROSS, N_UNDER_NO_CHUNK, N_COUNTS };

/* what segment b of a sample hands to the launches behind it, where the caller asks for load planes (tests/path_ref.c's LOAD_
 * bits, with the wet start in the lamp ray's place — a water frame has no lamp rays): the path goes on into segment b + 1 (a
 * surface event's continuation is one); a sun ray was marched from segment b's hit; segment b started in a liquid of the table */
enum { LOAD_PATH = 1, LOAD_SUN = 2, LOAD_WET = 4 };

static float ref_exp_neg(float t) {
    if (!(t >= 0.0f)) return t != t ? t : 1.0f;
    if (t >= 128.0f) return 0.0f;
    const float x = -t;
    const float kf = floorf(x * 1.44269502f + 0.5f);
    const float r = (x - kf * 0.693359375f) - kf * -2.12194442e-4f;
    const float q = 0.5f + r * (0.166666672f + r * (0.0416666679f + r * (0.00833333377f + r * (0.00138888892f + r * 1.98412701e-4f))));
    const float p = (1.0f + r) + (r * r) * q;
    const int32_t k = (int32_t)kf;
    const uint32_t bp = orc_f2bits(p);
    const int32_t E = (int32_t)(bp >> 23) + k;
    if (E >= 1) return orc_bits2f(bp + ((uint32_t)k << 23));
    const uint32_t shift = (uint32_t)(1 - E);
    if (shift > 24u) return 0.0f;
    const uint32_t m = (bp & 0x007FFFFFu) | 0x00800000u;
    const uint32_t half = 1u << (shift - 1u), rem = m & ((half << 1) - 1u);
    uint32_t bits = m >> shift;
    if (rem > half || (rem == half && (bits & 1u))) bits += 1u;
    return orc_bits2f(bits);
}


/* step 1: the voxel at floor(o) as vrt_get_voxels answers — 0 outside the world box, 0 where there is no chunk */
static uint32_t voxel_at_floor(const orc_scene *s, v3 o) {
    const float fx = floorf(o.x), fy = floorf(o.y), fz = floorf(o.z);
    const float size = (float)s->world.size;
    if (!(fx >= 0.0f && fy >= 0.0f && fz >= 0.0f && fx < size && fy < size && fz < size)) return 0u;
    const uint32_t x = (uint32_t)fx, y = (uint32_t)fy, z = (uint32_t)fz, w = s->world.size_in_chunks;
    const uint32_t ch = (x >> 5) + w * ((y >> 5) + w * (z >> 5));
    const uint32_t root = ch < s->n_chunk_roots ? s->chunk_roots[ch] : 0u;
    if (root == 0u) return 0u;
    const v3 min = V3((float)((x >> 5) * 32u), (float)((y >> 5) * 32u), (float)((z >> 5) * 32u));
    const found_node f = find_chunk_node(s, V3(fx + 0.5f, fy + 0.5f, fz + 0.5f), 5u, min, root);
    return node_voxel(node_at(s, f.root + f.idx));
}

static int is_table_liquid(const orc_scene *s, uint32_t voxel) { return mat_at(s, voxel)->is_liquid == 1u; }

/* ---- B: the span walk.  cast_ray's DDA (common/src/math.rs:153-226, as tests/cast_ray_cases.py describes it) restated ---- */
typedef struct {
    float dist;
    int32_t prev[3], m[3];
    uint32_t v, steps;
    int ended, event, crossed;
} ref_span;

/* vrt_get_voxels' answer at an integer position, world-local */
static uint32_t voxel_at_int(const orc_scene *s, int32_t x, int32_t y, int32_t z) {
    const int32_t size = (int32_t)s->world.size;
    if (x < 0 || y < 0 || z < 0 || x >= size || y >= size || z >= size) return 0u;
    return voxel_at_floor(s, V3((float)x, (float)y, (float)z));
}

/* whether an integer position lies outside the world box or where chunk_roots holds no chunk */
static int no_chunk_at(const orc_scene *s, const int32_t m[3]) {
    const int32_t size = (int32_t)s->world.size;
    if (m[0] < 0 || m[1] < 0 || m[2] < 0 || m[0] >= size || m[1] >= size || m[2] >= size) return 1;
    const uint32_t w = s->world.size_in_chunks;
    const uint32_t ch = ((uint32_t)m[0] >> 5) + w * (((uint32_t)m[1] >> 5) + w * ((uint32_t)m[2] >> 5));
    return (ch < s->n_chunk_roots ? s->chunk_roots[ch] : 0u) == 0u;
}

static ref_span span_walk(const orc_scene *s, v3 o, v3 d, uint32_t max_span) {
    ref_span r;
    memset(&r, 0, sizeof r);
    /* ray_unit_step_size: sqrt(1 + (b/a)^2 + (c/a)^2), summed left to right */
    const float usx = sqrtf(1.0f + (d.y / d.x) * (d.y / d.x) + (d.z / d.x) * (d.z / d.x));
    const float usy = sqrtf(1.0f + (d.x / d.y) * (d.x / d.y) + (d.z / d.y) * (d.z / d.y));
    const float usz = sqrtf(1.0f + (d.x / d.z) * (d.x / d.z) + (d.y / d.z) * (d.y / d.z));
    int32_t m[3] = {(int32_t)floorf(o.x), (int32_t)floorf(o.y), (int32_t)floorf(o.z)};
    const int32_t step[3] = {d.x < 0.0f ? -1 : 1, d.y < 0.0f ? -1 : 1, d.z < 0.0f ? -1 : 1};
    float lx = d.x < 0.0f ? (o.x - (float)m[0]) * usx : ((float)(m[0] + 1) - o.x) * usx;
    float ly = d.y < 0.0f ? (o.y - (float)m[1]) * usy : ((float)(m[1] + 1) - o.y) * usy;
    float lz = d.z < 0.0f ? (o.z - (float)m[2]) * usz : ((float)(m[2] + 1) - o.z) * usz;
    uint32_t last = voxel_at_int(s, m[0], m[1], m[2]);   /* the liquid that made the segment wet */
    for (uint32_t i = 0; i < max_span; i++) {
        r.prev[0] = m[0]; r.prev[1] = m[1]; r.prev[2] = m[2];
        if (lx < ly && lx < lz) {   /* x, then z, else y: the reference's order of the branches */
            m[0] += step[0];
            r.dist = lx;
            lx += usx;
        } else if (lz < lx && lz < ly) {
            m[2] += step[2];
            r.dist = lz;
            lz += usz;
        } else {
            m[1] += step[1];
            r.dist = ly;
            ly += usy;
        }
        r.steps = i + 1u;
        r.v = voxel_at_int(s, m[0], m[1], m[2]);
        if (!is_table_liquid(s, r.v)) {
            r.ended = 1;
            break;
        }
        if (r.v != last) r.crossed = 1;
        last = r.v;
    }
    r.m[0] = m[0]; r.m[1] = m[1]; r.m[2] = m[2];
    r.event = r.ended && r.v == 0u && isfinite(r.dist) && r.dist >= 0.0f;
    return r;
}

void ref_refract_span(const orc_scene *s, const float *o, const float *d, uint32_t max_span, float *dist, int32_t *prev, int32_t *m, uint32_t *v_steps,
                      int32_t *flags) {
    const ref_span r = span_walk(s, V3(o[0], o[1], o[2]), V3(d[0], d[1], d[2]), max_span);
    *dist = r.dist;
    memcpy(prev, r.prev, sizeof r.prev);
    memcpy(m, r.m, sizeof r.m);
    v_steps[0] = r.v; v_steps[1] = r.steps;
    flags[0] = r.ended; flags[1] = r.event; flags[2] = r.crossed;
}

/* ---- A: the bend of a transmitted surface event ---- */
static v3 bend_in(float eta, v3 d, v3 norm) {
    const float dn = orc_dot(norm, d);
    const float c = fabsf(dn);
    const v3 nn = dn < 0.0f ? norm : V3(-norm.x, -norm.y, -norm.z);
    const float s2 = (eta * eta) * (1.0f - c * c);
    const float ct = sqrtf(1.0f - s2);
    const float g = eta * c - ct;
    return orc_normalize(V3(eta * d.x + g * nn.x, eta * d.y + g * nn.y, eta * d.z + g * nn.z));
}

/* ---- C: the underside event's choice.  Returns 1 total, 2 reflected by the draw, 3 out; *dout: d' ---- */
static int bend_out(float ior, float reflectance, v3 d, v3 n, float u, v3 *dout) {
    const float dn = orc_dot(n, d);
    const float c = fabsf(dn);
    const float s2 = (ior * ior) * (1.0f - c * c);
    int branch = 1;
    float ct = 0.0f;
    if (s2 < 1.0f) {
        ct = sqrtf(1.0f - s2);
        const float mm = 1.0f - ct, m5 = (mm * mm) * (mm * mm) * mm;
        const float F = reflectance + (1.0f - reflectance) * m5;
        branch = u < F ? 2 : 3;
    }
    if (branch == 3) {
        const float g = ior * c - ct;
        *dout = orc_normalize(V3(ior * d.x + g * n.x, ior * d.y + g * n.y, ior * d.z + g * n.z));
    } else {
        *dout = V3(d.x - 2.0f * n.x * dn, d.y - 2.0f * n.y * dn, d.z - 2.0f * n.z * dn);
    }
    return branch;
}

/* the bends alone: leaving == 0: A with eta = 1.0f / ior (returns 0); otherwise C */
int ref_refract_bend(float ior, float reflectance, const float *d, const float *n, float u, int leaving, float *out) {
    v3 r;
    int branch = 0;
    if (leaving) branch = bend_out(ior, reflectance, V3(d[0], d[1], d[2]), V3(n[0], n[1], n[2]), u, &r);
    else r = bend_in(1.0f / ior, V3(d[0], d[1], d[2]), V3(n[0], n[1], n[2]));
    out[0] = r.x; out[1] = r.y; out[2] = r.z;
    return branch;
}

typedef struct {
    const orc_scene *scene, *dry, *no_disc;   /* dry: every is_liquid cleared; no_disc: sun_intensity 0 */
    const float *emission;
    const ref_polish *polish;
    const ref_translucency *tr;
    int polished_frame, translucent_frame;
    float sun_strength;
    const ref_water_optics *wo;
    float ior, eta;        /* vrt_set_water_refraction: ior (0: off), 1.0f / ior */
    uint32_t max_span;     /* ... its max_span, 0 replaced by 64 */
} water_settings;

static float exit_t(float pos, float dir) {
    const float c = floorf(pos);
    const float far = dir > 0.0f ? c + 1.0f : c;
    return dir != 0.0f ? (far - pos) / dir : INFINITY;
}

/* One sample: its light; *id: the id word of its primary segment's own march; n[N_COUNTS] grows; thr_bed: NULL, or where the
 * throughput at the sample's first hit on a solid voxel at the end of a wet segment is kept (untouched if there is none); load:
 * NULL, or the sample's LOAD_ bits, segment b's at load[b * load_stride]; prim: NULL, or where the branch of the primary segment's
 * underside event is kept (0 none, 1 total, 2 reflected by the draw, 3 out; 4: an event on the last allowed segment). */
static v3 trace_path_water(const water_settings *p, uint32_t px, uint32_t py, uint32_t rng, uint32_t *id, uint64_t *n, float *thr_bed, uint8_t *load,
                           size_t load_stride, uint8_t *prim) {
    const orc_scene *s = p->scene;
    const int on = p->wo->flags != 0u;
    v3 light = V3(0.0f, 0.0f, 0.0f);
    v3 origin, dir;
    create_ray_from_screen(s, (int32_t)px, (int32_t)py, &origin, &dir);
    v3 thr = V3(1.0f, 1.0f, 1.0f);
    const int sun_lit = p->sun_strength != 0.0f;
    int bed_seen = 0;
    for (uint32_t bounce = 0; bounce < s->settings.max_ray_bounces; bounce++) {
        /* steps 1 to 3 */
        const int wet = !on || is_table_liquid(s, voxel_at_floor(s, origin));
        /* B: the walk, ahead of the march and of the absorption */
        ref_span sp;
        memset(&sp, 0, sizeof sp);
        if (on && wet && p->ior != 0.0f) {
            sp = span_walk(s, origin, dir, p->max_span);
            if (sp.ended && sp.v != 0u) n[N_WALK_SOLID] += 1u;
            if (!sp.ended) n[N_WALK_CAP] += 1u;
            if (sp.crossed) n[N_WALK_CROSS] += 1u;
        }
        hit_result rs = ray_world(wet ? s : p->dry, origin, dir);   /* the frame's own march: the id word, the steps */
        n[N_STEPS] += rs.iter_count;
        if (bounce != 0) n[N_BOUNCE_SEGMENTS] += 1u;
        if (bounce == 0) *id = id_word(&rs);
        if (sp.event) {
            /* C: the underside event; nothing else of the march is used */
            const v3 nrm = V3((float)(sp.prev[0] - sp.m[0]), (float)(sp.prev[1] - sp.m[1]), (float)(sp.prev[2] - sp.m[2]));
            const v3 x = V3(origin.x + dir.x * sp.dist, origin.y + dir.y * sp.dist, origin.z + dir.z * sp.dist);
            if (load) load[bounce * load_stride] |= LOAD_WET;
            thr.x *= ref_exp_neg(p->wo->absorb[0] * sp.dist);
            thr.y *= ref_exp_neg(p->wo->absorb[1] * sp.dist);
            thr.z *= ref_exp_neg(p->wo->absorb[2] * sp.dist);
            n[N_UNDER] += 1u;
            if (no_chunk_at(s, sp.m)) n[N_UNDER_NO_CHUNK] += 1u;
            if (bounce != 0) n[N_WET_BOUNCES] += 1u;
            if (bounce + 1 == s->settings.max_ray_bounces) {
                if (prim && bounce == 0) *prim = 4;
                break;
            }
            const float u = orc_rng_next(&rng);
            v3 nd;
            const int branch = bend_out(p->ior, p->wo->reflectance, dir, nrm, u, &nd);
            if (branch == 3) origin = V3(x.x - nrm.x * ORC_SHADOW_BIAS, x.y - nrm.y * ORC_SHADOW_BIAS, x.z - nrm.z * ORC_SHADOW_BIAS);
            else origin = V3(x.x + nrm.x * ORC_SHADOW_BIAS, x.y + nrm.y * ORC_SHADOW_BIAS, x.z + nrm.z * ORC_SHADOW_BIAS);
            dir = nd;
            n[branch == 1 ? N_UNDER_TOTAL : branch == 2 ? N_UNDER_FRESNEL : N_UNDER_OUT] += 1u;
            if (prim && bounce == 0) *prim = (uint8_t)branch;
            if (load) load[bounce * load_stride] |= LOAD_PATH;
            continue;
        }
        if (on && wet) {
            const float w = rs.water_dist;
            if (load) load[bounce * load_stride] |= LOAD_WET;
            thr.x *= ref_exp_neg(p->wo->absorb[0] * w);
            thr.y *= ref_exp_neg(p->wo->absorb[1] * w);
            thr.z *= ref_exp_neg(p->wo->absorb[2] * w);
            if (w > 0.0f) n[N_WET_W] += 1u;
            if (rs.hit) n[N_WET_HIT] += 1u;
            if (bounce == 0 && w > 0.0f) n[N_WET_PRIMARY_W] += 1u;
            if (bounce != 0) n[N_WET_BOUNCES] += 1u;
            if (rs.hit && is_solid_hit(s, &rs) && thr_bed && !bed_seen) {
                thr_bed[0] = thr.x; thr_bed[1] = thr.y; thr_bed[2] = thr.z;
                bed_seen = 1;
            }
        }
        if (!rs.hit) {
            const v3 sky = ray_sky((sun_lit && bounce != 0) ? p->no_disc : s, origin, dir);
            light.x += sky.x * thr.x;
            light.y += sky.y * thr.y;
            light.z += sky.z * thr.z;
            break;
        }
        if (on && !wet && is_table_liquid(s, rs.voxel)) {
            /* step 4, the surface event.  (On the last allowed segment nothing of it is observed, so nothing is drawn.) */
            n[N_SURFACE] += 1u;
            if (bounce + 1 == s->settings.max_ray_bounces) break;
            const float u = orc_rng_next(&rng);
            const float dn = orc_dot(rs.norm, dir);
            const float c = fabsf(dn), m = 1.0f - c, m5 = (m * m) * (m * m) * m;
            const float F = p->wo->reflectance + (1.0f - p->wo->reflectance) * m5;
            if (u < F) {
                origin = V3(rs.pos.x + rs.norm.x * ORC_SHADOW_BIAS, rs.pos.y + rs.norm.y * ORC_SHADOW_BIAS, rs.pos.z + rs.norm.z * ORC_SHADOW_BIAS);
                dir = V3(dir.x - 2.0f * rs.norm.x * dn, dir.y - 2.0f * rs.norm.y * dn, dir.z - 2.0f * rs.norm.z * dn);
                n[N_REFLECTED] += 1u;
            } else {
                origin = rs.pos;
                if (p->ior != 0.0f) {   /* A */
                    dir = bend_in(p->eta, dir, rs.norm);
                    n[N_BENT] += 1u;
                }
                n[N_TRANSMITTED] += 1u;
            }
            if (load) load[bounce * load_stride] |= LOAD_PATH;
            continue;
        }
        /* step 5: path_ref.c's text */
        const v3 so = V3(rs.pos.x + rs.norm.x * ORC_SHADOW_BIAS, rs.pos.y + rs.norm.y * ORC_SHADOW_BIAS, rs.pos.z + rs.norm.z * ORC_SHADOW_BIAS);
        const uint32_t entry = rs.voxel > 255u ? 255u : rs.voxel;
        const float e = p->emission[entry];
        if (e != 0.0f) {
            light.x += (rs.color.x * e) * thr.x;
            light.y += (rs.color.y * e) * thr.y;
            light.z += (rs.color.z * e) * thr.z;
        }
        if (sun_lit && is_solid_hit(s, &rs)) {
            const v3 sd = orc_normalize(V3(s->settings.sun_pos[0] - (float)s->world.min[0] - so.x,
                                           s->settings.sun_pos[1] - (float)s->world.min[1] - so.y,
                                           s->settings.sun_pos[2] - (float)s->world.min[2] - so.z));
            const float c = orc_dot(rs.norm, sd);
            if (c > 0.0f) {
                const hit_result sh = ray_world(s, so, sd);   /* liquids passed, unattenuated */
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
        if (bounce + 1 == s->settings.max_ray_bounces) break;
        if (p->translucent_frame && orc_rng_next(&rng) < p->tr[entry].chance) {
            const float tx = exit_t(rs.pos.x, dir.x), ty = exit_t(rs.pos.y, dir.y), tz = exit_t(rs.pos.z, dir.z);
            float t = tx;
            if (ty < t) t = ty;
            if (tz < t) t = tz;
            const float ts = t + 0.001f;
            thr.x *= p->tr[entry].color[0]; thr.y *= p->tr[entry].color[1]; thr.z *= p->tr[entry].color[2];
            origin = V3(rs.pos.x + dir.x * ts, rs.pos.y + dir.y * ts, rs.pos.z + dir.z * ts);
            n[N_PASSES] += 1u;
            if (load) load[bounce * load_stride] |= LOAD_PATH;
            continue;
        }
        int polished = 0;
        if (p->polished_frame) polished = orc_rng_next(&rng) < p->polish[entry].chance;
        const float d = orc_dot(rs.norm, dir);
        const v3 spec = V3(dir.x - 2.0f * rs.norm.x * d, dir.y - 2.0f * rs.norm.y * d, dir.z - 2.0f * rs.norm.z * d);
        const v3 rd = rng_next_dir(&rng);
        const v3 sc = orc_normalize(V3(rs.norm.x + rd.x, rs.norm.y + rd.y, rs.norm.z + rd.z));
        const float scatter = polished ? p->polish[entry].scatter : mat_at(s, rs.voxel)->scatter;
        const v3 nd = orc_normalize(V3(orc_mix(spec.x, sc.x, scatter), orc_mix(spec.y, sc.y, scatter), orc_mix(spec.z, sc.z, scatter)));
        const v3 tint = polished ? V3(p->polish[entry].color[0], p->polish[entry].color[1], p->polish[entry].color[2]) : rs.color;
        thr.x *= tint.x; thr.y *= tint.y; thr.z *= tint.z;
        origin = so;
        dir = nd;
        n[N_POLISHED] += polished ? 1u : 0u;
        if (load) load[bounce * load_stride] |= LOAD_PATH;
    }
    return light;
}

typedef struct {
    orc_scene dry, no_disc;
    orc_material dry_mats[256];
} water_scenes;

static water_settings settings_of(const orc_scene *scene, water_scenes *ws, const float *emission, const ref_polish *polish, const ref_translucency *tr,
                                  float sun_strength, const ref_water_optics *wo, const ref_water_refraction *wr) {
    water_settings p = {scene, &ws->dry, &ws->no_disc, emission, polish, tr, 0, 0, sun_strength, wo, wr->ior, wr->ior != 0.0f ? 1.0f / wr->ior : 0.0f,
                        wr->max_span ? wr->max_span : 64u};
    for (uint32_t i = 0; i < 256u; i++) {
        p.polished_frame |= polish[i].chance != 0.0f;
        p.translucent_frame |= tr[i].chance != 0.0f;
        ws->dry_mats[i] = scene->materials[i];
        ws->dry_mats[i].is_liquid = 0u;
    }
    ws->dry = *scene;
    ws->dry.materials = ws->dry_mats;
    ws->no_disc = *scene;
    ws->no_disc.settings.sun_intensity = 0.0f;
    return p;
}

/* A w x h frame of samples sample_base .. sample_base + spp - 1, their mean in rgb[h][w][3], the id word of the first sample's
 * primary segment in ids[h][w], counts[N_COUNTS].  Like orc_render, pixels beyond the last whole 8 x 8 tile are not traced: the
 * caller passes zeroed arrays.  load: NULL, or load[spp][max_ray_bounces][h][w] bytes, zero on entry: the LOAD_ bits.  prim: NULL, or
 * prim[h][w] bytes, zero on entry: the branch of the first sample's primary underside event (trace_path_water). */
void ref_render_refract(const orc_scene *scene, const float *emission, const ref_polish *polish, const ref_translucency *tr, float sun_strength,
                        const ref_water_optics *wo, const ref_water_refraction *wr, uint32_t w, uint32_t h, uint32_t seed, uint32_t spp,
                        uint32_t sample_base, float *rgb, uint32_t *ids, uint64_t *counts, uint8_t *load, uint8_t *prim) {
    const uint32_t x1 = w & ~7u, y1 = h & ~7u, nspp = spp ? spp : 1u;
    const size_t plane = (size_t)w * h;
    water_scenes ws;
    const water_settings p = settings_of(scene, &ws, emission, polish, tr, sun_strength, wo, wr);
    uint64_t n[N_COUNTS] = {0};
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : n[:N_COUNTS])
    for (int32_t py = 0; py < (int32_t)y1; py++) {
        for (uint32_t px = 0; px < x1; px++) {
            const size_t o = (size_t)py * w + px;
            v3 sum = V3(0.0f, 0.0f, 0.0f);
            uint32_t id = 0;
            for (uint32_t sm = 0; sm < nspp; sm++) {
                uint32_t sid = 0;
                const v3 l = trace_path_water(&p, px, (uint32_t)py, path_seed(px, (uint32_t)py, w, h, sample_base + sm, seed), &sid, n, NULL,
                                              load ? load + ((size_t)sm * scene->settings.max_ray_bounces) * plane + o : NULL, plane,
                                              (prim && sm == 0) ? prim + o : NULL);
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

/* one pixel's one sample: its light, the id word of its primary segment, its counts, and thr_bed[3]: the throughput at its first
 * hit on a solid voxel at the end of a wet segment (left as passed in if there is none) */
void ref_trace_pixel_refract(const orc_scene *scene, const float *emission, const ref_polish *polish, const ref_translucency *tr, float sun_strength,
                             const ref_water_optics *wo, const ref_water_refraction *wr, uint32_t w, uint32_t h, uint32_t seed, uint32_t px, uint32_t py,
                             uint32_t sample, float *light, uint32_t *id, uint64_t *counts, float *thr_bed) {
    water_scenes ws;
    const water_settings p = settings_of(scene, &ws, emission, polish, tr, sun_strength, wo, wr);
    memset(counts, 0, N_COUNTS * sizeof *counts);
    *id = 0;
    const v3 l = trace_path_water(&p, px, py, path_seed(px, py, w, h, sample, seed), id, counts, thr_bed, NULL, 0, NULL);
    light[0] = l.x; light[1] = l.y; light[2] = l.z;
}

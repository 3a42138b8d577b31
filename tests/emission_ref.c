/* tests/emission_ref.c — the path trace with the per-material emission table (include/vrt.h: vrt_write_emission), for the
 * tests.  TEST INFRASTRUCTURE ONLY: compiled by tests/emission_ref.py with oracle/Makefile's CFLAGS into a temporary directory.
 *
 * oracle/vrt_oracle.c's trace_path_into has no emission (the live Material has none).  This restates its loop with the
 * term of path_tracer.wgsl:183-184 and nothing else changed: on every hit whose voxel's entry e is not 0, the sample's light
 * gains (mc * e) * thr per channel before thr *= mc — mc the hit's colour (rs.color: face shading, the step-count grey),
 * thr the throughput before the hit.  A sample's light is its terms in segment order; the frame's, its samples' lights
 * summed in sample order and divided by spp.  The march, the sky and the RNG are the oracle's own functions (this file
 * includes it), so every direction is bit for bit the oracle's and the kernels'. */
#include "../oracle/vrt_oracle.c"

static v3 trace_path_emissive(const orc_scene *s, const float *emission, uint32_t px, uint32_t py, uint32_t rng, uint32_t *id) {
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
        const float e = emission[rs.voxel > 255u ? 255u : rs.voxel];
        if (e != 0.0f) {
            light.x += (rs.color.x * e) * thr.x;
            light.y += (rs.color.y * e) * thr.y;
            light.z += (rs.color.z * e) * thr.z;
        }
        float d = orc_dot(rs.norm, dir);
        v3 spec = V3(dir.x - 2.0f * rs.norm.x * d, dir.y - 2.0f * rs.norm.y * d, dir.z - 2.0f * rs.norm.z * d);
        v3 rd = rng_next_dir(&rng);
        v3 sc = orc_normalize(V3(rs.norm.x + rd.x, rs.norm.y + rd.y, rs.norm.z + rd.z));
        float scatter = mat_at(s, rs.voxel)->scatter;
        v3 nd = orc_normalize(V3(orc_mix(spec.x, sc.x, scatter), orc_mix(spec.y, sc.y, scatter), orc_mix(spec.z, sc.z, scatter)));
        thr.x *= rs.color.x; thr.y *= rs.color.y; thr.z *= rs.color.z;
        origin = V3(rs.pos.x + rs.norm.x * ORC_SHADOW_BIAS, rs.pos.y + rs.norm.y * ORC_SHADOW_BIAS, rs.pos.z + rs.norm.z * ORC_SHADOW_BIAS);
        dir = nd;
    }
    return light;
}

/* A w x h path-trace frame of samples sample_base .. sample_base + spp - 1 (seeded as orc_render seeds sample s), their mean
 * in rgb[h][w][3], the primary segment's id word in ids[h][w].  Like orc_render, pixels beyond the last whole 8 x 8 tile are
 * not traced: the caller passes zeroed arrays. */
void ref_render_path_emissive(const orc_scene *scene, const float *emission, uint32_t w, uint32_t h, uint32_t spp, uint32_t seed,
                              uint32_t sample_base, float *rgb, uint32_t *ids) {
    const uint32_t x1 = w & ~7u, y1 = h & ~7u, nspp = spp ? spp : 1u;
#pragma omp parallel for schedule(dynamic, 1)
    for (int32_t py = 0; py < (int32_t)y1; py++) {
        for (uint32_t px = 0; px < x1; px++) {
            const size_t o = (size_t)py * w + px;
            v3 sum = V3(0.0f, 0.0f, 0.0f);
            uint32_t id = 0;
            for (uint32_t sm = 0; sm < nspp; sm++) {
                uint32_t sid = 0;
                v3 l = trace_path_emissive(scene, emission, px, (uint32_t)py, path_seed(px, (uint32_t)py, w, h, sample_base + sm, seed), &sid);
                sum.x += l.x; sum.y += l.y; sum.z += l.z;
                if (sm == 0) id = sid;
            }
            rgb[o * 3 + 0] = sum.x / (float)nspp;
            rgb[o * 3 + 1] = sum.y / (float)nspp;
            rgb[o * 3 + 2] = sum.z / (float)nspp;
            ids[o] = id;
        }
    }
}

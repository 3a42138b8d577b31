/* tests/denoise_ref.c — the edge-stopped a-trous filter of vrt_set_denoise (include/vrt.h), for the tests.  TEST INFRASTRUCTURE
 * ONLY: compiled by tests/denoise_ref.py with oracle/Makefile's CFLAGS into a temporary directory.
 *
 * An independent statement of the filter as include/vrt.h words it: plain arrays, plain loops, no code of the package (it does
 * not include csrc/both/denoise_math.h).  The guide words come from the oracle's own primary march (this file includes the
 * oracle for create_ray_from_screen, ray_world and id_word). */
#include "../oracle/vrt_oracle.c"

#define REF_KEY_MASK (ORC_ID_VOXEL_MASK | ORC_ID_HIT | ORC_ID_NX | ORC_ID_NY | ORC_ID_NZ | ORC_ID_WATER)

static int ref_filterable(uint32_t id) { return (id & ORC_ID_HIT) && (id & (ORC_ID_NX | ORC_ID_NY | ORC_ID_NZ)); }

/* The guide words of a w x h frame of the scene's camera: for a filterable pixel the integer coordinate of the hit face's
 * plane, floor(pos[a] + 0.5) on the lowest axis a whose normal bit is set; 0 for every other pixel and beyond the last whole
 * 8 x 8 tile.  ids (may be NULL) receives the primary march's id words. */
void ref_guide(const orc_scene *scene, uint32_t w, uint32_t h, uint32_t *guide, uint32_t *ids) {
    const uint32_t x1 = w & ~7u, y1 = h & ~7u;
    memset(guide, 0, (size_t)w * h * sizeof(uint32_t));
    if (ids) memset(ids, 0, (size_t)w * h * sizeof(uint32_t));
#pragma omp parallel for schedule(dynamic, 1)
    for (int32_t py = 0; py < (int32_t)y1; py++) {
        for (uint32_t px = 0; px < x1; px++) {
            v3 origin, dir;
            create_ray_from_screen(scene, (int32_t)px, py, &origin, &dir);
            const hit_result rs = ray_world(scene, origin, dir);
            const uint32_t id = id_word(&rs);
            const size_t o = (size_t)py * w + px;
            if (ids) ids[o] = id;
            if (!ref_filterable(id)) continue;
            const float p = (id & ORC_ID_NX) ? rs.pos.x : ((id & ORC_ID_NY) ? rs.pos.y : rs.pos.z);
            guide[o] = (uint32_t)(int32_t)floorf(p + 0.5f);
        }
    }
}

/* `passes` passes over rgb[h][w][3] -> out[h][w][3] (tmp: scratch of the same size).  sigma_color 0: no colour stop. */
void ref_denoise(const float *rgb, const uint32_t *ids, const uint32_t *guide, uint32_t w, uint32_t h, uint32_t passes, float sigma_color,
                 float *out, float *tmp) {
    static const float hk[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    const int32_t x1 = (int32_t)(w & ~7u), y1 = (int32_t)(h & ~7u);
    const size_t bytes = (size_t)w * h * 3 * sizeof(float);
    float *a = out, *b = tmp;
    if (passes & 1u) { a = tmp; b = out; }   /* the last pass writes `out` */
    memcpy(a, rgb, bytes);
    for (uint32_t i = 0; i < passes; i++) {
        const int32_t s = (int32_t)(1u << i);
        float *const src = a, *const dst = b;
        memcpy(dst, src, bytes);   /* every pixel that is not filtered is copied through */
#pragma omp parallel for schedule(static)
        for (int32_t y = 0; y < y1; y++) {
            for (int32_t x = 0; x < x1; x++) {
                const size_t p = (size_t)y * w + (size_t)x;
                if (!ref_filterable(ids[p])) continue;
                const float cpr = src[p * 3], cpg = src[p * 3 + 1], cpb = src[p * 3 + 2];
                float sum_r = 0.0f, sum_g = 0.0f, sum_b = 0.0f, wsum = 0.0f;
                for (int32_t dy = -2; dy <= 2; dy++) {
                    for (int32_t dx = -2; dx <= 2; dx++) {
                        const int32_t qx = x + s * dx, qy = y + s * dy;
                        if (qx < 0 || qy < 0 || qx >= x1 || qy >= y1) continue;
                        const size_t q = (size_t)qy * w + (size_t)qx;
                        if ((ids[q] & REF_KEY_MASK) != (ids[p] & REF_KEY_MASK) || guide[q] != guide[p]) continue;
                        float wt = hk[dy + 2] * hk[dx + 2];
                        const float cqr = src[q * 3], cqg = src[q * 3 + 1], cqb = src[q * 3 + 2];
                        if (sigma_color != 0.0f) {
                            const float sg = sigma_color / (float)(1u << i);
                            const float dr = cqr - cpr, dg = cqg - cpg, db = cqb - cpb;
                            const float d2 = (dr * dr + dg * dg) + db * db;
                            wt = wt * ((sg * sg) / ((sg * sg) + d2));
                        }
                        sum_r = sum_r + wt * cqr;
                        sum_g = sum_g + wt * cqg;
                        sum_b = sum_b + wt * cqb;
                        wsum = wsum + wt;
                    }
                }
                dst[p * 3] = sum_r / wsum;
                dst[p * 3 + 1] = sum_g / wsum;
                dst[p * 3 + 2] = sum_b / wsum;
            }
        }
        a = dst;
        b = src;
    }
    if (a != out) memcpy(out, a, bytes);   /* (passes == 0) */
}

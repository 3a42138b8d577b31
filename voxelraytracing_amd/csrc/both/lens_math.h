// lens_math.h — the camera sampling of vrt_set_camera_sampling (include/vrt.h), once: a sample's own primary ray from its four
// draws, up to the two vectors that are normalised.  vrt_path_lens.h's kernels and host_capi.cpp's vrth_lens_ray both compile this
// text.  Only f32 add, subtract, multiply, divide and square root occur, in the order include/vrt.h states; it relies on
// -ffp-contract=off on both sides (both.h).  The divides and the square root are handed in: the host passes the plain
// operators, a kernel the forms its wave chose (vrt_march.h: the same correctly rounded results without the general case's
// scaffolding); the normalisations between and behind the two halves are the caller's (orc_normalize / normalize_wave).
#pragma once
#include "both.h"

namespace vrt {

// cos(2*pi*u) by quadrant and polynomial: vrt_path_common.h's vcos2pi (restated: a header of both/ includes nothing of the
// project, and that kernel text stays where its kernels' code was built from).  u + 0.75 reaches 1.75: the quadrant is taken & 3
VRT_BOTH float lens_cos2pi(float u) {
    const float t = u * 4.0f;
    const float q = floorf(t);
    const float a = (t - q) * 1.57079637f;
    const float a2 = a * a;
    const float sn = a * (1.0f + a2 * (-0.166666672f + a2 * (0.00833333377f + a2 * (-0.000198412701f + a2 * (2.75573188e-06f + a2 * -2.50521079e-08f)))));
    const float cs = 1.0f + a2 * (-0.5f + a2 * (0.0416666679f + a2 * (-0.00138888892f + a2 * (2.48015876e-05f + a2 * (-2.75573199e-07f + a2 * 2.08767559e-09f)))));
    const int qi = (int)q & 3;
    return qi == 0 ? cs : (qi == 1 ? -sn : (qi == 2 ? -cs : sn));
}

struct LensV3 { float x, y, z; };

// Step 2: the sample's position on the pixel grid, and create_ray_from_screen's products with it — the direction before it is
// normalised.  ip / iv: cam.inv_proj_mat / cam.inv_view_mat (column-major, as create_ray reads them).
template <class Div>
VRT_BOTH LensV3 lens_pixel_dir(uint32_t px, uint32_t py, float u1, float u2, float pixel_spread, const float *proj_size, const float *ip,
                               const float *iv, Div &&div) {
    const float fx = (float)px + (u1 - 0.5f) * pixel_spread;
    const float fy = (float)py + (u2 - 0.5f) * pixel_spread;
    const float x = div(fx * 2.0f, proj_size[0]) - 1.0f;
    const float y = div(fy * 2.0f, proj_size[1]) - 1.0f;
    const float c0 = x, c1 = -y, c2 = -1.0f, c3 = 1.0f;
    const float e0 = c0 * ip[0] + c1 * ip[1] + c2 * ip[2] + c3 * ip[3];
    const float e1 = c0 * ip[4] + c1 * ip[5] + c2 * ip[6] + c3 * ip[7];
    const float e2 = -1.0f, e3 = 0.0f;
    return LensV3{e0 * iv[0] + e1 * iv[1] + e2 * iv[2] + e3 * iv[3], e0 * iv[4] + e1 * iv[5] + e2 * iv[6] + e3 * iv[7],
                  e0 * iv[8] + e1 * iv[9] + e2 * iv[10] + e3 * iv[11]};
}

// Step 3 with an aperture that is not 0: the point of the lens the sample leaves from (o) and the vector from it to the point of
// the pixel's ray that is in focus (to_focus = F - o, not normalised).  origin: cam.pos - f32(world.min); d: step 2's direction,
// normalised.
template <class Sqrt>
VRT_BOTH void lens_thin(const LensV3 &origin, const LensV3 &d, float u3, float u4, float aperture, float focus_distance, const float *iv,
                        Sqrt &&sqrt_of, LensV3 &o, LensV3 &to_focus) {
    const float r = aperture * sqrt_of(u3);
    const float lx = r * lens_cos2pi(u4);
    const float ly = r * lens_cos2pi(u4 + 0.75f);
    const LensV3 F{origin.x + d.x * focus_distance, origin.y + d.y * focus_distance, origin.z + d.z * focus_distance};
    o = LensV3{(origin.x + iv[0] * lx) + iv[1] * ly, (origin.y + iv[4] * lx) + iv[5] * ly, (origin.z + iv[8] * lx) + iv[9] * ly};
    to_focus = LensV3{F.x - o.x, F.y - o.y, F.z - o.z};
}

}  // namespace vrt

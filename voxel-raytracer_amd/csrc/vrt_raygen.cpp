// vrt_raygen.cpp -- the part of ray generation (shaders/raytracing.comp:624-641) that does not depend on the pixel as a whole,
// made once per projection on the host. Pure arithmetic: no device, no context (also linked into the test-support library).
#include <cmath>
#include <cstring>
#include <vector>

#include "vrt_miss.h"

namespace vrt_internal {

// ---- ray generation, the part that does not depend on the pixel as a whole ---------------------------------------------
// comp:626-634: u = px / W * 2 - 1, v likewise, view = invProjection * (u, v, -1, 1), view /= view.w. For the inverse of
// any perspective or orthographic projection x depends on u alone, y on v alone, z and w on neither, so the W + H + 1
// distinct values are computed here once per (matrix, W, H) -- by the SAME float operations in the same order, which is
// what makes them the same bits (this file is compiled with -ffp-contract=off like the kernels; x86-64 float arithmetic is
// IEEE binary32) -- and the kernels read them (View::gen_x/gen_y/gen_z) instead of making two integer->float conversions,
// five divisions and a 4x4 product per pixel. A zero term's SIGN can depend on the other coordinate ((+0) * v): each value
// is therefore evaluated with the other coordinate at +1 and at -1 and must come out the same bits, otherwise the table
// is refused and the kernels run the shader's own prologue. Returns false when the matrix is not of that shape.
bool build_ray_table(const float *m, int W, int H, std::vector<float> &tab, float &z_out) {
    static const int kZeros[10] = {4, 8, 12, 1, 9, 13, 2, 6, 3, 7};   // column-major m[c * 4 + r]
    for (int k : kZeros)
        if (!(m[k] == 0.0f)) return false;
    const auto row = [&](int r, float u, float v) {   // mat_vec() of vrt_common.hip.h with (x, y, z, w) = (u, v, -1, 1)
        return (m[0 * 4 + r] * u + m[1 * 4 + r] * v) + (m[2 * 4 + r] * -1.0f + m[3 * 4 + r] * 1.0f);
    };
    const auto same = [](float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; };
    const float w = row(3, 1.0f, 1.0f), z = row(2, 1.0f, 1.0f);
    for (int k = 1; k < 4; ++k) {
        const float u = (k & 1) ? -1.0f : 1.0f, v = (k & 2) ? -1.0f : 1.0f;
        if (!same(row(3, u, v), w) || !same(row(2, u, v), z)) return false;
    }
    if (!(w == w) || !(z == z)) return false;
    const bool divide = fabsf(w) > 1e-6f;
    tab.resize((size_t)W + (size_t)H);
    double hi = 0.0;
    for (int px = 0; px < W; ++px) {
        const float u = ((float)px / (float)W) * 2.0f - 1.0f;
        const float x = row(0, u, 1.0f);
        if (!same(x, row(0, u, -1.0f))) return false;
        const float q = divide ? x / w : x;
        if (!(fabs((double)q) <= 1.0995e12)) return false;   // 2^40; also refuses NaN
        hi = fabs((double)q) > hi ? fabs((double)q) : hi;
        tab[(size_t)px] = q;
    }
    for (int py = 0; py < H; ++py) {
        const float v = ((float)py / (float)H) * 2.0f - 1.0f;
        const float y = row(1, 1.0f, v);
        if (!same(y, row(1, -1.0f, v))) return false;
        const float q = divide ? y / w : y;
        if (!(fabs((double)q) <= 1.0995e12)) return false;
        tab[(size_t)W + (size_t)py] = q;
    }
    z_out = divide ? z / w : z;
    // range of the first normalisation, dot = (x^2 + y^2) + z^2 >= z^2: inside [2^-80, 2^82], its root inside [2^-40, 2^41]
    const double az = fabs((double)z_out);
    return az >= 9.0949e-13 && az <= 1.0995e12;   // 2^-40 .. 2^40
}

// The second normalisation takes |invView3x3 * d| for a unit d: between the matrix' smallest and largest singular value.
// With F2 the squared Frobenius norm, sigma_max <= sqrt(F2) and sigma_min = |det| / (sigma_1 sigma_2) >= 2 |det| / F2.
// True when that keeps the squared length inside [2^-62, 2^42] with room for the rounding of the product.
bool view_matrix_in_range(const float *m) {
    double a[3][3], f2 = 0.0;
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) { a[r][c] = (double)m[c * 4 + r]; f2 += a[r][c] * a[r][c]; }
    if (!(f2 >= 9.0949e-13 && f2 <= 1.0995e12)) return false;      // 2^-40 .. 2^40, refuses NaN
    const double det = a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
                       a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
    return det * det >= 2.3842e-7 * f2 * f2 * f2;                   // sigma_min >= 2^-10 sqrt(F2)  <=  det^2 >= 2^-22 F2^3
}

// The miss-tile build's view (vrt_miss.h ViewParams) in two parts. miss_table_fit(), once per ray table (tab = gen_x[0..W) then
// gen_y[0..H), z = gen_z): the affine fit gen_x[px] = gx0 + px * gdx (and y), the tables' largest distance from it in pixels, the
// largest |g|^2. miss_view_params(), per view: inv_view as View::inv_view, gro = cam_pos * voxel_scale as the kernel computes it.
// The margin covers, in pixels,
//   * the tables' distance from the fit;
//   * the rays' own float error: a direction within a relative 1e-5 * cond(invView3x3) of inv_view3x3 * (gen_x, gen_y, gen_z)
//     (the prologue's normalisations and product and the march's renormalisation take a few ulps, 2^-24 each) moves the
//     table point by that much times |g|^2 / |gz|;
//   * 1.5 pixels on top.
// False when the view gives no usable mask (degenerate tables, a singular or non-finite matrix, an eye beyond miss::kMaxEye, a
// margin above 16 pixels).
bool miss_table_fit(const float *tab, float z, int W, int H, vrt::miss::TableFit &f) {
    if (W < 1 || H < 1) return false;
    const float *tx = tab, *ty = tab + W;
    f.gx0 = tx[0]; f.gdx = W > 1 ? ((double)tx[W - 1] - (double)tx[0]) / (double)(W - 1) : 1.0;
    f.gy0 = ty[0]; f.gdy = H > 1 ? ((double)ty[H - 1] - (double)ty[0]) / (double)(H - 1) : 1.0;
    f.gz = z;
    if (!(std::fabs(f.gdx) > 0.0) || !(std::fabs(f.gdy) > 0.0) || !(std::fabs(f.gz) > 0.0)) return false;
    double dev = 0.0;   // largest distance from the fit, in pixels
    for (int px = 0; px < W; ++px) dev = std::fmax(dev, std::fabs(((double)tx[px] - (f.gx0 + px * f.gdx)) / f.gdx));
    for (int py = 0; py < H; ++py) dev = std::fmax(dev, std::fabs(((double)ty[py] - (f.gy0 + py * f.gdy)) / f.gdy));
    const double xm = std::fmax(std::fabs((double)tx[0]), std::fabs((double)tx[W - 1]));
    const double ym = std::fmax(std::fabs((double)ty[0]), std::fabs((double)ty[H - 1]));
    f.dev_px = dev;
    f.gmax2 = xm * xm + ym * ym + f.gz * f.gz;
    f.width = W; f.height = H;
    return dev == dev && f.gmax2 == f.gmax2;
}

bool miss_view_params(const float *inv_view, const float gro[3], const vrt::miss::TableFit &f, vrt::miss::ViewParams &v) {
    double a[3][3], f2 = 0.0;
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) { a[r][c] = (double)inv_view[c * 4 + r]; f2 += a[r][c] * a[r][c]; }
    const double det = a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
                       a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
    if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return false;
    double g2 = 0.0;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {   // adjugate / det: inverse[r][c] = cofactor(c, r) / det
            const int r0 = (c + 1) % 3, r1 = (c + 2) % 3, c0 = (r + 1) % 3, c1 = (r + 2) % 3;
            v.m[r * 3 + c] = (a[r0][c0] * a[r1][c1] - a[r0][c1] * a[r1][c0]) / det;
            g2 += v.m[r * 3 + c] * v.m[r * 3 + c];
        }
    for (int k = 0; k < 3; ++k) {
        if (!(std::fabs((double)gro[k]) <= vrt::miss::kMaxEye)) return false;
        v.eye[k] = (double)gro[k];
    }
    v.gx0 = f.gx0; v.gdx = f.gdx; v.gy0 = f.gy0; v.gdy = f.gdy; v.gz = f.gz;
    const double eps = 1e-5 * std::sqrt(f2 * g2);   // cond_F(invView3x3) >= 3 for any matrix, 3 for a rotation
    const double err = eps * f.gmax2 / std::fabs(f.gz) / std::fmin(std::fabs(f.gdx), std::fabs(f.gdy));
    v.margin_px = 1.5 + f.dev_px + err;
    if (!(v.margin_px <= 16.0)) return false;
    v.width = f.width; v.height = f.height;
    v.tiles_x = (f.width + vrt::miss::kTile - 1) / vrt::miss::kTile;
    v.tiles_y = (f.height + vrt::miss::kTile - 1) / vrt::miss::kTile;
    return true;
}

}  // namespace vrt_internal

// lanczos_resize_ycc_layout.cpp -- what the YCbCr entries (lanczos_resize_ycc_*, lanczos_resize_ycc_out, lanczos_resize_ycc16;
// DESIGN.md 4.5) need no device for: the one resolver of lanczos_ycc_source and lanczos_ycc_dest for samples of 1 or 2 bytes, the
// tight layout the *_init entries fill, Pillow's colour tables in both directions and the integer matrices of the wide frames.
// Pure host code, as lanczos_resize_route.cpp is: no HIP call, and nothing here calls into another unit, so a host program links
// it alone (tests/native/ycc_layout_check.cpp).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "lanczos_resize.hpp"

namespace lz {

// ---- layouts -----------------------------------------------------------------------------------------------------------------

template <class L>
int ycc_layout_resolve(const L* l, int w, int h, int B, bool aligned_origin, int x0, int y0, YccLayout* s) {
    if (!l) return LANCZOS_ERR_BAD_ARG;
    for (int32_t r : l->reserved)
        if (r != 0) return LANCZOS_ERR_BAD_ARG;
    if (l->layout != LANCZOS_YCC_PLANAR && l->layout != LANCZOS_YCC_NV12 && l->layout != LANCZOS_YCC_NV21) return LANCZOS_ERR_BAD_ARG;
    if ((l->sub_x | l->sub_y) & ~1) return LANCZOS_ERR_BAD_ARG;
    const bool nv = l->layout != LANCZOS_YCC_PLANAR;
    if (nv && (l->sub_x != 1 || l->cb_offset != l->cr_offset)) return LANCZOS_ERR_BAD_ARG;
    if (aligned_origin && ((x0 & l->sub_x) || (y0 & l->sub_y))) return LANCZOS_ERR_BAD_ARG;   // (a subsampling is 0 or 1)
    const long long cw = ((long long)w + l->sub_x) >> l->sub_x, ch = ((long long)h + l->sub_y) >> l->sub_y;
    const long long c_row = (nv ? 2 : 1) * B * cw, cap = (long long)1 << 40;
    if (l->y_row_stride < (long long)B * w || l->c_row_stride < c_row || l->y_row_stride > cap || l->c_row_stride > cap)
        return LANCZOS_ERR_BAD_ARG;
    if (l->cb_offset < 0 || l->cr_offset < 0 || l->cb_offset > ((long long)1 << 56) || l->cr_offset > ((long long)1 << 56))
        return LANCZOS_ERR_BAD_ARG;
    if ((l->y_row_stride | l->c_row_stride | l->cb_offset | l->cr_offset) & (B - 1)) return LANCZOS_ERR_BAD_ARG;   // words lie on words
    // a plane is its pitched rows, all of them: the resize kernels' range checks cover whole rows
    const long long y_end = h * l->y_row_stride, c_len = ch * l->c_row_stride;
    const long long b0 = l->cb_offset, b1 = b0 + c_len, r0 = l->cr_offset, r1 = r0 + c_len;
    if (b0 < y_end || r0 < y_end) return LANCZOS_ERR_BAD_ARG;                 // a chroma plane inside the luma plane
    if (!nv && b0 < r1 && r0 < b1) return LANCZOS_ERR_BAD_ARG;                // Cb over Cr
    s->layout = l->layout, s->sx = l->sub_x, s->sy = l->sub_y, s->cw = (int)cw, s->ch = (int)ch;
    s->y_rs = (size_t)l->y_row_stride, s->c_rs = (size_t)l->c_row_stride;
    s->cb_off = (size_t)b0, s->cr_off = (size_t)r0;
    s->extent = (size_t)std::max(b1, r1);
    s->named = (size_t)(std::max(b0, r0) + (ch - 1) * l->c_row_stride + c_row);
    return LANCZOS_OK;
}

template <class L>
int ycc_layout_init(L* l, int w, int h, int B, int layout, int sub_x, int sub_y) {
    if ((sub_x | sub_y) & ~1) return LANCZOS_ERR_BAD_ARG;
    const int64_t cw = (w + sub_x) >> sub_x, ch = (h + sub_y) >> sub_y, luma = (int64_t)w * h * B;
    *l = L{};
    l->layout = layout, l->sub_x = sub_x, l->sub_y = sub_y;
    l->y_row_stride = (int64_t)B * w, l->cb_offset = luma;
    if (layout == LANCZOS_YCC_PLANAR) l->c_row_stride = B * cw, l->cr_offset = luma + B * cw * ch;
    else l->c_row_stride = 2 * B * cw, l->cr_offset = luma;
    YccLayout s;
    return ycc_layout_resolve(l, w, h, B, false, 0, 0, &s);
}

template int ycc_layout_resolve(const lanczos_ycc_source*, int, int, int, bool, int, int, YccLayout*);
template int ycc_layout_resolve(const lanczos_ycc_dest*, int, int, int, bool, int, int, YccLayout*);
template int ycc_layout_init(lanczos_ycc_source*, int, int, int, int, int, int);
template int ycc_layout_init(lanczos_ycc_dest*, int, int, int, int, int, int);

// ---- the standard tables of 8-bit frames -------------------------------------------------------------------------------------

// (int)(k * (i - off) * 64 + 0.5): in double, truncated toward zero, as Pillow's ImagingConvertYCbCr2RGB tables are built
static int32_t ycc_entry(double k, int i, int off) { return (int32_t)(k * (i - off) * 64 + 0.5); }

bool ycc_table(int standard, int32_t* t) {
    double ky = 1.0, r_cr, g_cb, g_cr, b_cb;
    int y_off = 0, y_add = 0;
    if (standard == LANCZOS_YCC_JFIF) {
        r_cr = 1.402, g_cb = -0.34414, g_cr = -0.71414, b_cb = 1.772;
    } else if (standard == LANCZOS_YCC_BT601 || standard == LANCZOS_YCC_BT709) {
        const double kr = standard == LANCZOS_YCC_BT601 ? 0.299 : 0.2126, kb = standard == LANCZOS_YCC_BT601 ? 0.114 : 0.0722;
        const double kg = 1.0 - kr - kb, kc = 255.0 / 224.0;
        ky = 255.0 / 219.0, y_off = 16, y_add = 32;
        r_cr = 2.0 * (1.0 - kr) * kc, b_cb = 2.0 * (1.0 - kb) * kc;
        g_cb = -2.0 * (1.0 - kb) * kb / kg * kc, g_cr = -2.0 * (1.0 - kr) * kr / kg * kc;
    } else {
        return false;
    }
    const double k[3][2] = {{0.0, r_cr}, {g_cb, g_cr}, {b_cb, 0.0}};   // [c][cb, cr]
    for (int c = 0; c < 3; c++)
        for (int i = 0; i < 256; i++) {
            // the full-range luma entry is 64 i exactly; a limited-range one carries the + 32 that makes the shift round
            t[(c * 3 + 0) * 256 + i] = standard == LANCZOS_YCC_JFIF ? 64 * i : ycc_entry(ky, i, y_off) + y_add;
            t[(c * 3 + 1) * 256 + i] = k[c][0] == 0.0 ? 0 : ycc_entry(k[c][0], i, 128);
            t[(c * 3 + 2) * 256 + i] = k[c][1] == 0.0 ? 0 : ycc_entry(k[c][1], i, 128);
        }
    return true;
}

// (int)(k * i * 64 + 0.5): in double, truncated toward zero, as Pillow's ImagingConvertRGB2YCbCr tables are built
static int32_t ycc_forward_entry(double k, int i) { return (int32_t)(k * i * 64 + 0.5); }

bool ycc_table_forward(int standard, int32_t* t) {
    double k[3][3];
    int add[3];
    if (standard == LANCZOS_YCC_JFIF) {
        const double jfif[3][3] = {{0.299, 0.587, 0.114}, {-0.16874, -0.33126, 0.5}, {0.5, -0.41869, -0.08131}};
        memcpy(k, jfif, sizeof(k));
        add[0] = 0, add[1] = add[2] = 128 * 64;
    } else if (standard == LANCZOS_YCC_BT601 || standard == LANCZOS_YCC_BT709) {
        const double kr = standard == LANCZOS_YCC_BT601 ? 0.299 : 0.2126, kb = standard == LANCZOS_YCC_BT601 ? 0.114 : 0.0722;
        const double kg = 1.0 - kr - kb, sy = 219.0 / 255.0, sc = 224.0 / 255.0;
        const double ub = 2.0 * (1.0 - kb), ur = 2.0 * (1.0 - kr);
        const double m[3][3] = {{kr * sy, kg * sy, kb * sy}, {-kr / ub * sc, -kg / ub * sc, 0.5 * sc}, {0.5 * sc, -kg / ur * sc, -kb / ur * sc}};
        memcpy(k, m, sizeof(k));
        add[0] = 16 * 64 + 32, add[1] = add[2] = 128 * 64 + 32;   // the + 32 makes the shift round
    } else {
        return false;
    }
    for (int c = 0; c < 3; c++)
        for (int j = 0; j < 3; j++)
            for (int i = 0; i < 256; i++) t[(c * 3 + j) * 256 + i] = ycc_forward_entry(k[c][j], i) + (j == 0 ? add[c] : 0);
    return true;
}

// ---- the integer matrices of 16-bit frames -----------------------------------------------------------------------------------

int ycc16_matrix_validate(const lanczos_ycc16_matrix* m) {
    if (!m) return LANCZOS_ERR_BAD_ARG;
    for (int c = 0; c < 3; c++) {
        for (int j = 0; j < 3; j++)
            if (m->k[c][j] <= -(1 << 24) || m->k[c][j] >= (1 << 24)) return LANCZOS_ERR_BAD_ARG;
        if (m->sub[c] < 0 || m->sub[c] > 65535) return LANCZOS_ERR_BAD_ARG;
    }
    if (m->shift < 0 || m->shift > 30 || m->max < 0 || m->max > 65535) return LANCZOS_ERR_BAD_ARG;
    for (int32_t r : m->reserved)
        if (r != 0) return LANCZOS_ERR_BAD_ARG;
    return LANCZOS_OK;
}

bool ycc16_matrix_init(lanczos_ycc16_matrix* m, int standard, int depth, bool msb_aligned, bool full_range) {
    double kr, kb;
    if (standard == LANCZOS_YCC_JFIF || standard == LANCZOS_YCC_BT601) kr = 0.299, kb = 0.114;
    else if (standard == LANCZOS_YCC_BT709) kr = 0.2126, kb = 0.0722;
    else if (standard == LANCZOS_YCC_BT2020) kr = 0.2627, kb = 0.0593;
    else return false;
    if (depth < 8 || depth > 16) return false;
    const double kg = 1.0 - kr - kb;
    const double unit = msb_aligned ? (double)(1 << (16 - depth)) : 1.0;
    const double full = (double)((1 << depth) - 1);
    const double ky = 65535.0 / ((full_range ? full : (double)(219 << (depth - 8))) * unit);
    const double kc = 65535.0 / ((full_range ? full : (double)(224 << (depth - 8))) * unit);
    const double real[3][3] = {{ky, 0.0, 2.0 * (1.0 - kr) * kc},
                               {ky, -2.0 * (1.0 - kb) * kb / kg * kc, -2.0 * (1.0 - kr) * kr / kg * kc},
                               {ky, 2.0 * (1.0 - kb) * kc, 0.0}};
    *m = lanczos_ycc16_matrix{};
    // the largest shift that keeps every rounded entry below 2^23 in magnitude
    for (int shift = 30; shift >= 0; shift--) {
        bool fits = true;
        for (int c = 0; c < 3; c++)
            for (int j = 0; j < 3; j++) {
                const long long v = llround(real[c][j] * (double)(1ll << shift));
                if (v <= -(1ll << 23) || v >= (1ll << 23)) fits = false;
                else m->k[c][j] = (int32_t)v;
            }
        if (fits) {
            m->shift = shift;
            break;
        }
        if (shift == 0) return false;   // (no standard gets here: the largest coefficient is below 600)
    }
    m->sub[0] = full_range ? 0 : (int32_t)((16 << (depth - 8)) * unit);
    m->sub[1] = m->sub[2] = (int32_t)((1 << (depth - 1)) * unit);
    m->max = 65535;
    return true;
}

}  // namespace lz

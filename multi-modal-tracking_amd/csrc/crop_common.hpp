// Device functions shared by the two crop kernels: the tracker's (preprocess.hip, mmt_sample_target*)
// and the training input's (train_input.hip, mmt_train_crops_table).  Both restate sample_target
// (lib/train/data/processing_utils.py:15-77) and OpenCV's 8-bit INTER_LINEAR resize as the header of
// preprocess.hip describes; keeping them here makes both kernels compute the same bits.
#pragma once
#include "common.hpp"

// Parity is bit-exact against separately rounded torch / numpy / Python ops: no FMA contraction.
#pragma clang fp contract(off)

// Python's int(round(v)) for the crop corner: round half to even.
MMT_DEV int py_round(double v) { return (int)rint(v); }

MMT_DEV int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

MMT_DEV short coef(float v) {  // saturate_cast<short>(v * INTER_RESIZE_COEF_SCALE): cvRound
    const int r = (int)rintf(v * 2048.f);
    return (short)clampi(r, -32768, 32767);
}

struct Geo {
    int x1, y1, crop, xlim, ylim;  // padded-crop origin, size, and the first image column/row not copied
};

MMT_DEV Geo crop_geometry(const double* __restrict__ box, double factor, int H, int W) {
    const double x = box[0], y = box[1], w = box[2], h = box[3];
    Geo g;
    g.crop = (int)ceil(sqrt(w * h) * factor);
    g.x1 = py_round(x + 0.5 * w - g.crop * 0.5);
    g.y1 = py_round(y + 0.5 * h - g.crop * 0.5);
    // im[y1+y1_pad : y2-y2_pad, x1+x1_pad : x2-x2_pad] with x2_pad = max(x2 - W + 1, 0): when the crop
    // runs past the right (bottom) edge, the last image column (row) is not copied either.
    const int x2 = g.x1 + g.crop, y2 = g.y1 + g.crop;
    g.xlim = x2 >= W ? W - 1 : W;
    g.ylim = y2 >= H ? H - 1 : H;
    return g;
}

// The taps and weights of one output coordinate d of the linear path, for a crop of `crop` pixels
// and scale = crop / out_sz.  Columns are clamped with the weight moved to one tap (edge = true);
// rows keep their weights and clamp the tap indices (edge = false).
struct Taps {
    int s0, s1;  // source indices inside the padded crop
    float f;     // weight of s1; 1 - f is the weight of s0
};

MMT_DEV Taps linear_taps(int d, double scale, int crop, bool edge) {
    Taps t;
    float f = (float)((d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= s;
    if (edge) {
        if (s < 0) f = 0.f, s = 0;
        if (s >= crop - 1) f = 0.f, s = crop - 1;
        t.s0 = s;
        t.s1 = min(s + 1, crop - 1);  // its weight is 0 whenever s + 1 is past the edge
    } else {
        t.s0 = clampi(s, 0, crop - 1);
        t.s1 = clampi(s + 1, 0, crop - 1);
    }
    t.f = f;
    return t;
}

// exactly 1/2: cv2.resize takes INTER_LINEAR to INTER_AREA
MMT_DEV bool is_area2(double scale) {
    const int is = (int)rint(scale);
    return is == 2 && fabs(scale - is) < 2.220446049250313e-16;
}

struct Px3 {
    int v[3];
};

// The resized uint8 crop's pixel (dy, dx), three channels: src(r, c) is the padded crop's pixel
// (image pixel or the constant border 0) as a Px3, read once per tap.  crop < 1 gives 0.
template <class Src>
MMT_DEV void resize_pixel(const Src& src, int crop, int os, int dy, int dx, int v[3]) {
    v[0] = v[1] = v[2] = 0;
    if (crop < 1) return;
    const double inv = (double)os / crop, scale = 1.0 / inv;
    if (is_area2(scale)) {
        const Px3 p00 = src(2 * dy, 2 * dx), p01 = src(2 * dy, 2 * dx + 1), p10 = src(2 * dy + 1, 2 * dx),
                  p11 = src(2 * dy + 1, 2 * dx + 1);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[ch] = (p00.v[ch] + p01.v[ch] + p10.v[ch] + p11.v[ch] + 2) >> 2;
    } else {
        const Taps tx = linear_taps(dx, scale, crop, true), ty = linear_taps(dy, scale, crop, false);
        const int a0 = coef(1.f - tx.f), a1 = coef(tx.f), b0 = coef(1.f - ty.f), b1 = coef(ty.f);
        const Px3 p00 = src(ty.s0, tx.s0), p01 = src(ty.s0, tx.s1), p10 = src(ty.s1, tx.s0), p11 = src(ty.s1, tx.s1);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int h0 = p00.v[ch] * a0 + p01.v[ch] * a1;
            const int h1 = p10.v[ch] * a0 + p11.v[ch] * a1;
            const int t = (((h0 >> 4) * b0) >> 16) + (((h1 >> 4) * b1) >> 16);
            v[ch] = clampi((t + 2) >> 2, 0, 255);
        }
    }
}

// cv2.applyColorMap on a 3-channel crop: BGR2GRAY, GRAY2BGR, per-channel LUT
MMT_DEV void colour_map(const uint8_t* __restrict__ lut, int v[3]) {
    const int gray = (v[0] * 1868 + v[1] * 9617 + v[2] * 4899 + (1 << 13)) >> 14;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) v[ch] = lut[gray * 3 + ch];
}

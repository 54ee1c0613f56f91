// One patch pixel of the person crop (crop.hip: all detections of one frame; frames.hip: all detections of many frames): OpenCV's 8-bit
// INTER_LINEAR warpAffine + ToTensor + Normalize, the arithmetic described at the top of crop.hip.  Both kernels call this one function, so a
// clip's patches are the per-frame patches bit for bit.
#pragma once
#include "common.h"

// M: the INVERSE 2x3 map of person b (patch pixel -> frame pixel); idx: pixel y * out_w + (x - x_begin) of the produced column range
__device__ __forceinline__ void crop_normalize_pixel(const uint8_t* __restrict__ frame, int H, int W, long row_stride, const double* __restrict__ M,
                                                     int b, int idx, int patch_h, int x_begin, int out_w, float* __restrict__ out,
                                                     uint8_t* __restrict__ raw, float m0, float m1, float m2, float s0, float s1, float s2) {
    const int y = idx / out_w, x = x_begin + idx % out_w;
    // imgwarp.cpp warpAffine: adelta / bdelta / X0 / Y0 are cvRound'ed (round half to even) products in AB_SCALE units
    const int adelta = (int)__double2ll_rn(M[0] * x * 1024.0), bdelta = (int)__double2ll_rn(M[3] * x * 1024.0);
    // explicit mul / add: an fma contraction of M1*y + M2 could move a tie and break bit-parity with the CPU restatement
    const int X0 = (int)__double2ll_rn(__dadd_rn(__dmul_rn(M[1], (double)y), M[2]) * 1024.0) + 16;
    const int Y0 = (int)__double2ll_rn(__dadd_rn(__dmul_rn(M[4], (double)y), M[5]) * 1024.0) + 16;
    const int X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;
    const int sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31;
    const int w00 = (32 - fy) * (32 - fx) * 32, w01 = (32 - fy) * fx * 32, w10 = fy * (32 - fx) * 32, w11 = fy * fx * 32;
    int acc[3] = {1 << 14, 1 << 14, 1 << 14};
    auto tap = [&](int yy, int xx, int w) {
        if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W && w) {
            const uint8_t* p = frame + (size_t)yy * row_stride + (size_t)xx * 3;
            acc[0] += w * p[0]; acc[1] += w * p[1]; acc[2] += w * p[2];
        }
    };
    tap(sy, sx, w00); tap(sy, sx + 1, w01); tap(sy + 1, sx, w10); tap(sy + 1, sx + 1, w11);
    const float mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
    const size_t plane = (size_t)out_w * patch_h;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int v = acc[c] >> 15;
        out[((size_t)b * 3 + c) * plane + idx] = (__fdiv_rn((float)v, 255.0f) - mean[c]) / sd[c];
        if (raw) raw[(((size_t)b * patch_h + y) * out_w + (x - x_begin)) * 3 + c] = (uint8_t)v;
    }
}

// MXFP8 number format of the MX pilot of the ViT inference path (gemm_blk_mx.hip, vit_ops.hip): OCP FP8 E4M3 elements ("e4m3fn", max 448, subnormals
// kept, NOT the fnuz encoding) in blocks of 32 consecutive elements along K that share one E8M0 scale byte s, value 2^(s - 127).
//
//   scale rule:    e = the smallest integer with amax <= 448 * 2^e, clamped to [-127, 127]; an all-zero block gets e = -127; s = e + 127.
//                  (never saturates: every |x| * 2^-e <= 448)
//   element:       q = RNE(x * 2^-e) to e4m3fn, subnormals (multiples of 2^-9 below 2^-6) kept
//
// Both are done in integer / exact fp32 arithmetic here rather than by the hardware convert, so that the bits are those of the rule above (and of a
// torch `float8_e4m3fn` cast of the same fp32 product, which the tests use as the reference).
//
// Layouts (rows padded to a multiple of 32; padded rows hold zeros when written by the quantiser / LayerNorm pass):
//   data    [rows/32][K/16][32][16] bytes  -- the 512-byte unit of the bf16 operand layout [rows/32][K/8][32][8] with 16 FP8 per row
//   scales  [rows/32][K/128][32][4] bytes  -- byte j of row r in group g is the scale of the 32-block 4 g + j of that row: one dword per lane and
//                                             128-deep K step, which is what a v_mfma_scale_f32_32x32x64_f8f6f4 lane needs for two K sub-steps
#pragma once
#include "common.h"

// e of the scale rule for a block maximum amax >= 0.  448 = 1.75 * 2^8: with amax = m * 2^E, m in [1, 2), amax <= 448 * 2^e <=> e >= E - 8 when
// m <= 1.75, else e >= E - 7.  fp32 zero / subnormal maxima are below 448 * 2^-127 and take the clamp.
__device__ __forceinline__ int mx_scale_exp(float amax) {
    const uint32_t b = __float_as_uint(amax);
    const int be = (int)(b >> 23);
    if (be == 0) return -127;
    int e = be - 127 - ((b & 0x7fffffu) <= 0x600000u ? 8 : 7);
    return e < -127 ? -127 : (e > 127 ? 127 : e);
}

// 2^-e as an exact fp32 (2^-127 is the subnormal 0x00400000)
__device__ __forceinline__ float mx_inv_scale(int e) {
    return e == 127 ? __uint_as_float(0x00400000u) : __uint_as_float((uint32_t)(127 - e) << 23);
}

// fp32 -> e4m3fn byte, round to nearest even, for |v| <= 448 (what the scale rule guarantees).  Normal range: round the fp32 significand to 3 bits
// (a carry moves into the exponent), then re-bias 127 -> 7.  Below 2^-6: the value in units of 2^-9 rounded with rint (RNE); 8 units = 0x08 = 2^-6,
// the smallest normal, so the two ranges meet without a seam.  The sign is kept for zeros too (torch casts -0.0 to 0x80).
__device__ __forceinline__ uint32_t mx_e4m3(float v) {
    const uint32_t b = __float_as_uint(v);
    const uint32_t s = (b >> 24) & 0x80u;
    const float a = fabsf(v);
    uint32_t q;
    if (a < 0.015625f) {
        q = (uint32_t)__builtin_rintf(a * 512.0f);
    } else {
        uint32_t u = b & 0x7fffffffu;
        u += 0x7ffffu + ((u >> 20) & 1u);
        q = (((u >> 23) - 120u) << 3) | ((u >> 20) & 7u);
    }
    return s | q;
}

// four values (already multiplied by 2^-e) -> four e4m3 bytes, first value in the low byte
__device__ __forceinline__ uint32_t mx_pack4(float a, float b, float c, float d) {
    return mx_e4m3(a) | (mx_e4m3(b) << 8) | (mx_e4m3(c) << 16) | (mx_e4m3(d) << 24);
}

// Clip inference, input side: the two per-frame preparations of the demo (demo/tester.py:95-146) for MANY frames per launch.
//
// whmr_crop_normalize_frames   = whmr_crop_normalize (crop.hip) over a device table with one row per detection: each row names its own frame
//   (pointer, H, W, row stride) and its inverse affine map, so all persons of all frames of a clip -- frames of any sizes -- leave in ONE launch.
//   The pixel arithmetic is crop_dev.h's, shared with the per-frame kernel.
//
// whmr_resize_normalize_frames = Normalize(ToTensor(Resize(short side))) of F equal-size uint8 frames (tester.py:47-53,101-103).  The resize is Pillow's
//   Image.resize(..., BILINEAR) in its 8-bit integer arithmetic [3P Pillow ImagingResample, restated as augment.hip does for the bicubic filter]:
//   triangle filter of support max(1, in / out), taps computed in float64 exactly as precompute_coeffs does (no fused multiply-add: see the pragma),
//   normalised, rounded to 22 fractional bits; accumulator started at one half, shifted, clipped; horizontal pass into a uint8 intermediate, then
//   the vertical pass.  A dimension whose size does not change is not resampled: its pass takes the one source byte (what `copy` selects below), so
//   with both unchanged the launches only move and normalise bytes.  The normalisation (v / 255 - mean) / std is fused into the vertical pass as two
//   true fp32 divisions -- what torchvision's ToTensor + Normalize compute.
//   Both passes are bandwidth-bound (per 720p frame: 2.8 MB read, 2.3 MB intermediate written and read, 7.7 MB fp32 written).  A thread owns FOUR
//   neighbouring output pixels = 12 bytes: the intermediate's rows are pitched to 16 bytes, so the horizontal pass stores and the vertical pass
//   loads its 12 bytes as three aligned dwords per tap row (lanes contiguous: 768 bytes per wave instruction), and the fp32 output leaves as four
//   consecutive floats per channel and thread.  The source rows (3 W bytes, any alignment) are read bytewise; neighbouring lanes read neighbouring
//   bytes of one line, and each source byte is fetched from HBM once.
//   The tap tables are built on the device by whmr_resize_coeffs, once per (H, W, h, w); the caller keeps them.
#include "common.h"
#include "crop_dev.h"
#include "../../include/whmr_hip.h"

// every float64 / fp32 expression below restates host arithmetic bit for bit: no contraction into fused multiply-adds
#pragma clang fp contract(off)

static_assert(sizeof(whmr_frame_crop_item) == 72, "table layout");

__global__ __launch_bounds__(256) void crop_normalize_frames_kernel(const whmr_frame_crop_item* __restrict__ items, int patch_h, int x_begin, int out_w,
                                                                    float* __restrict__ out, uint8_t* __restrict__ raw, float m0, float m1, float m2,
                                                                    float s0, float s1, float s2) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= out_w * patch_h) return;
    const whmr_frame_crop_item& it = items[blockIdx.y];
    crop_normalize_pixel(it.frame, it.H, it.W, (long)it.row_stride, it.inv, blockIdx.y, idx, patch_h, x_begin, out_w, out, raw, m0, m1, m2, s0, s1, s2);
}

extern "C" int whmr_crop_normalize_frames(const void* items, int P, int patch_w, int patch_h, int x_begin, int x_end, float* out, uint8_t* raw,
                                          const float* mean3, const float* std3, void* stream) {
    const int out_w = x_end - x_begin;
    if (!items || P <= 0 || P > 65535 || out_w <= 0 || x_begin < 0 || x_end > patch_w || patch_h <= 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(crop_normalize_frames_kernel, dim3((out_w * patch_h + 255) / 256, P), dim3(256), 0, (hipStream_t)stream,
                       (const whmr_frame_crop_item*)items, patch_h, x_begin, out_w, out, raw, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    WHMR_CHECK_LAUNCH();
    return 0;
}

// ----------------------------------------------------------------------------- Pillow's bilinear resize
#define PREC 22

// ImagingResample's ksize of one axis: 2 ceil(support) + 1, support = max(1, in / out)
static int resize_ksize(int in_size, int out_size) {
    const double scale = (double)in_size / (double)out_size;
    return (int)ceil(scale < 1.0 ? 1.0 : scale) * 2 + 1;
}

__device__ __forceinline__ double bilinear_filter(double x) {
    x = fabs(x);
    return x < 1.0 ? 1.0 - x : 0.0;
}

// taps of one axis (blockIdx.y: 0 = x, 1 = y): row xx of [out][2 + ksize] int32 = (first input index, number of taps, taps)
__global__ __launch_bounds__(256) void resize_coef_kernel(int in_w, int out_w, int kx, int in_h, int out_h, int ky, int32_t* __restrict__ coef) {
    const int axis = blockIdx.y, xx = blockIdx.x * 256 + threadIdx.x;
    const int in_size = axis ? in_h : in_w, out_size = axis ? out_h : out_w, ksize = axis ? ky : kx;
    if (xx >= out_size) return;
    int32_t* row = coef + (axis ? (int64_t)out_w * (2 + kx) : 0) + (int64_t)xx * (2 + ksize);
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * filterscale, ss = 1.0 / filterscale;
    const double center = 0.0 + ((double)xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    if (xmax > ksize) xmax = ksize;                       // cannot happen (ksize = 2 ceil(support) + 1); keeps every store inside the row
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += bilinear_filter(((double)(x + xmin) - center + 0.5) * ss);
    row[0] = xmin;
    row[1] = xmax;
    for (int x = 0; x < xmax; ++x) {
        double w = bilinear_filter(((double)(x + xmin) - center + 0.5) * ss);
        if (ww != 0.0) w /= ww;
        row[2 + x] = w < 0 ? (int)(-0.5 + w * (double)(1 << PREC)) : (int)(0.5 + w * (double)(1 << PREC));
    }
}

extern "C" int whmr_resize_coeffs(int in_w, int out_w, int in_h, int out_h, int32_t* coef, long coef_words, void* stream) {
    if (in_w <= 0 || out_w <= 0 || in_h <= 0 || out_h <= 0 || !coef) return (int)hipErrorInvalidValue;
    const int kx = resize_ksize(in_w, out_w), ky = resize_ksize(in_h, out_h);
    if ((long)out_w * (2 + kx) + (long)out_h * (2 + ky) > coef_words) return (int)hipErrorInvalidValue;
    const int longest = out_w > out_h ? out_w : out_h;
    hipLaunchKernelGGL(resize_coef_kernel, dim3((longest + 255) / 256, 2), dim3(256), 0, (hipStream_t)stream, in_w, out_w, kx, in_h, out_h, ky, coef);
    WHMR_CHECK_LAUNCH();
    return 0;
}

__device__ __forceinline__ int clip8(int acc) { return min(max(acc >> PREC, 0), 255); }

// horizontal pass: frames [F, H, W, 3] -> mid [F * H rows of `pitch` bytes], w pixels each; thread = output pixels 4 g .. 4 g + 3 of one row
__global__ __launch_bounds__(256) void resize_hpass_kernel(const uint8_t* __restrict__ frames, int H, int W, int w, int kx, int copy,
                                                           const int32_t* __restrict__ coef, uint8_t* __restrict__ mid, int64_t pitch) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (4 * g >= w) return;
    const int64_t line_no = (int64_t)blockIdx.z * H + blockIdx.y;
    const uint8_t* line = frames + line_no * ((int64_t)W * 3);
    uint32_t pk[3] = {0u, 0u, 0u};                            // pixels past w stay zero: inside the row's pitch, never read
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int xx = 4 * g + j;
        if (xx < w) {
            const int32_t* row = coef + (int64_t)xx * (2 + kx);
            const int lo = copy ? xx : row[0];
            const int n = copy ? 1 : min(row[1], W - lo);
            int acc[3] = {1 << (PREC - 1), 1 << (PREC - 1), 1 << (PREC - 1)};
            const uint8_t* p = line + (int64_t)lo * 3;
            for (int k = 0; k < n; ++k, p += 3) {
                const int wt = copy ? (1 << PREC) : row[2 + k];          // the one tap of an unchanged axis: (half + (v << 22)) >> 22 == v
                acc[0] += wt * p[0]; acc[1] += wt * p[1]; acc[2] += wt * p[2];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int i = 3 * j + c;
                pk[i >> 2] |= (uint32_t)clip8(acc[c]) << (8 * (i & 3));
            }
        }
    }
    uint32_t* o = (uint32_t*)(mid + line_no * pitch + (int64_t)12 * g);
    o[0] = pk[0]; o[1] = pk[1]; o[2] = pk[2];
}

// vertical pass + ToTensor + Normalize: mid -> out [F, 3, h, w] fp32 (and out_u8 [F, h, w, 3]); thread = output pixels 4 g .. 4 g + 3 of one output row
__global__ __launch_bounds__(256) void resize_vpass_kernel(const uint8_t* __restrict__ mid, int64_t pitch, int H, int h, int w, int coef_off, int ky,
                                                           int copy, const int32_t* __restrict__ coef, float* __restrict__ out,
                                                           uint8_t* __restrict__ out_u8, float m0, float m1, float m2, float s0, float s1, float s2) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (4 * g >= w) return;
    const int yy = blockIdx.y;
    const int64_t f = blockIdx.z;
    const int32_t* row = coef + coef_off + (int64_t)yy * (2 + ky);             // the same for the whole workgroup: scalar loads
    const int lo = copy ? yy : row[0];
    const int n = copy ? 1 : min(row[1], H - lo);
    int acc[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] = 1 << (PREC - 1);
    const uint8_t* p = mid + (f * H + lo) * pitch + (int64_t)12 * g;
    for (int k = 0; k < n; ++k, p += pitch) {
        const int wt = copy ? (1 << PREC) : row[2 + k];
        const uint32_t* q = (const uint32_t*)p;
        const uint32_t d[3] = {q[0], q[1], q[2]};
#pragma unroll
        for (int i = 0; i < 12; ++i) acc[i] += wt * (int)((d[i >> 2] >> (8 * (i & 3))) & 255u);
    }
    const float mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float* o = out + ((f * 3 + c) * h + yy) * w + 4 * g;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (4 * g + j < w) {
                const int v = clip8(acc[3 * j + c]);
                o[j] = __fdiv_rn(__fdiv_rn((float)v, 255.0f) - mean[c], sd[c]);
                if (out_u8) out_u8[((f * h + yy) * w + 4 * g + j) * 3 + c] = (uint8_t)v;
            }
        }
    }
}

// bytes per row of the intermediate: 12 per group of four pixels, rounded up to 16
static long resize_mid_pitch(int w) { return (((long)(w + 3) / 4) * 12 + 15) / 16 * 16; }

extern "C" int whmr_resize_normalize_frames(const uint8_t* frames, int F, int H, int W, int h, int w, const int32_t* coef, long coef_words,
                                            uint8_t* mid, long mid_bytes, float* out, uint8_t* out_u8, const float* mean3, const float* std3,
                                            void* stream) {
    if (!frames || !coef || !mid || !out || F <= 0 || F > 65535 || H <= 0 || H > 65535 || W <= 0 || h <= 0 || h > 65535 || w <= 0)
        return (int)hipErrorInvalidValue;
    const int kx = resize_ksize(W, w), ky = resize_ksize(H, h);
    const long pitch = resize_mid_pitch(w);
    if ((long)w * (2 + kx) + (long)h * (2 + ky) > coef_words || (long)F * H * pitch > mid_bytes || ((uintptr_t)mid & 15)) return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const unsigned gx = (unsigned)(((w + 3) / 4 + 255) / 256);
    hipLaunchKernelGGL(resize_hpass_kernel, dim3(gx, H, F), dim3(256), 0, s, frames, H, W, w, kx, (int)(w == W), coef, mid, (int64_t)pitch);
    WHMR_CHECK_LAUNCH();
    hipLaunchKernelGGL(resize_vpass_kernel, dim3(gx, h, F), dim3(256), 0, s, (const uint8_t*)mid, (int64_t)pitch, H, h, w, w * (2 + kx), ky, (int)(h == H),
                       coef, out, out_u8, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    WHMR_CHECK_LAUNCH();
    return 0;
}

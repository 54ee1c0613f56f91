// Training-batch maker: the sample-making of BaseDataset.__getitem__ (datasets/base_dataset.py:249-384) for a whole batch.
//
// whmr_augment_crop   = rgb_processing (base_dataset.py:183-207) over utils/imutils.py:crop (:54-88) + Normalize + [:, :, 32:-32]:
//   1. integer box [ul, br) of the person, zero outside the source image (clamped reads through the per-sample table, never an address outside it);
//   2. rot != 0: the box widened by pad, turned about its centre, bilinear v00 + a (v01 - v00) in fp32 on float64 coordinates, zero outside,
//      TRUNCATED to uint8, pad removed                                         [3P skimage.transform.rotate, restated from its definition: unpinned]
//   3. resize to 256 x 256 with Pillow's antialiased bicubic (a = -0.5, support 2 max(1, box / 256)) in its 8-bit integer arithmetic: taps
//      computed in float64 exactly as precompute_coeffs does (no fused multiply-add: see the pragma), normalised, rounded to 22 fractional bits,
//      accumulator started at one half, shifted, clipped -- horizontal pass, then vertical pass           [3P Pillow ImagingResample, restated]
//   4. mirror in x when flip;
//   4a. occluders (whmr_augment_crop_occluded only; USE_SYNTHETIC_OCCLUSION, base_dataset.py:192-194): up to 7 pastes per sample, in order; each
//      resizes an RGBA object [h, w, 4] of the resident bank to (nw, nh) by area averaging and blends it over the patch at [start, start + (nw, nh)):
//      a = fp32(A) / 255, dst = uint8(a src + (1 - a) dst) in fp32, truncated.  The resize is DEFINED in integers: along an axis of source length S
//      and resized length n, output u covers [u S, (u + 1) S) and source texel j covers [j n, (j + 1) n) in units of 1 / n texel; the weight is the
//      integer overlap (weights of an axis sum to S); a channel is (2 sum(wy wx v) + D) // (2 D), D = w h (round half up), alpha included.  Within
//      0.5 of the float64 area average, the identity at n == S.             [3P PARE occlude_with_pascal_objects over cv2 INTER_AREA: parity unpinned]
//   5. min(255, max(0, v pn[c])) truncated to uint8, / 255, - mean, / std, NCHW fp32.
//   Only the 192 columns the model reads (32 .. 223 of 256) go through either pass.
//   Four launches: taps (B x 2 x 256 threads), rotation (rot != 0 samples), horizontal pass -> [box_h, 192, 3] uint8 scratch, vertical pass +
//   stages 4 / 4a / 5 (4a: a second instantiation of the vertical-pass kernel, no extra launch and no extra pass over the patch).  The intermediate lives in a global scratch, not in LDS: a box is up to thousands of rows high and its 192 x 3 bytes per row
//   are read ~2 support / scale = 4 times by the vertical pass from L2; an LDS tile would have to re-run the horizontal pass on the overlap rows.
//
// whmr_augment_labels = j2d_processing / j3d_processing / pose_processing / keypoints_world / bbox_info (base_dataset.py:209-247,294-373) with
//   imutils.transform's astype(int) + 1, flip_kp / flip_pose, rot_aa (cv2.Rodrigues both ways, restated from its documentation): one workgroup
//   per sample, float64, rows gathered from the resident annotation arrays by sample_index.
#include "common.h"

// every float64 / fp32 expression below restates host arithmetic bit for bit: no contraction into fused multiply-adds
#pragma clang fp contract(off)

struct whmr_augment_item {
    const uint8_t* img;                       // source image [H, W, 3] uint8, row_stride bytes per row
    int64_t row_stride, sample_index;
    int64_t rot_off, mid_off, coef_off;       // this sample's slices of the three scratch buffers (bytes, bytes, int32 words)
    int32_t H, W, ul_x, ul_y, bw, bh;         // box of rot = 0: [ul, ul + (bw, bh))
    int32_t pad, flip, is_smpl, ksize_x, ksize_y, reserved;      // pad = 0 <=> rot = 0
    double T[9];                              // get_transform(center, sc * scale, res, rot)
    double M[6];                              // rotated padded-box pixel (x, y) reads the padded box at (M0 x + M1 y + M2, M3 x + M4 y + M5)
    double j3d_cs[2], aa_cs[2];               // (cos, sin) of -rot pi / 180 and of deg2rad(-rot)
    double pn[3], rot, scale, center[2];
};
static_assert(sizeof(whmr_augment_item) == 304, "table layout");

struct whmr_augment_labels_io {
    const double *pose, *betas, *keypoints, *S, *smpl_2dkps;         // [N, 72], [N, 10], [N, 49, 3], [N, 24, 4] | null, [N, 24, 3] | null
    const float* has_smpl; const int32_t* gender; const uint8_t* mask;      // [N], [N], [B, 431] (0 / 1)
    float *o_pose, *o_betas, *o_keypoints, *o_keypoints_world, *o_smpl_2dkps, *o_pose_3d, *o_meta_mask, *o_has_smpl;
    double* o_scale; float* o_center; int64_t *o_orig_shape, *o_is_flipped; float* o_rot_angle; int32_t* o_gender; int64_t* o_sample_index;
    float *o_bbox_height, *o_bbox_width, *o_focal, *o_bbox_info; int64_t* o_has_pose_3d;
};

#define RES 256
#define X0 32
#define OUT_W 192
#define PREC 22

__device__ __forceinline__ double bicubic_filter(double x) {
    x = fabs(x);
    if (x < 1.0) return ((1.5 * x - 2.5) * x) * x + 1.0;
    if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * -0.5;
    return 0.0;
}

// taps of one axis: row xx of [256][2 + ksize] int32 = (first input index, number of taps, taps)
__global__ __launch_bounds__(256) void augment_coef_kernel(const whmr_augment_item* __restrict__ items, int32_t* __restrict__ coef) {
    const whmr_augment_item& it = items[blockIdx.y];
    const int axis = blockIdx.x, xx = threadIdx.x;
    const int in_size = axis ? it.bh : it.bw, ksize = axis ? it.ksize_y : it.ksize_x;
    int32_t* row = coef + it.coef_off + (axis ? (int64_t)RES * (2 + it.ksize_x) : 0) + (int64_t)xx * (2 + ksize);
    const double scale = (double)in_size / (double)RES;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * filterscale, ss = 1.0 / filterscale;
    const double center = 0.0 + ((double)xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    if (xmax > ksize) xmax = ksize;                       // cannot happen (ksize = 2 ceil(support) + 1); keeps every store inside the row
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += bicubic_filter(((double)(x + xmin) - center + 0.5) * ss);
    row[0] = xmin;
    row[1] = xmax;
    for (int x = 0; x < xmax; ++x) {
        double w = bicubic_filter(((double)(x + xmin) - center + 0.5) * ss);
        if (ww != 0.0) w /= ww;
        row[2 + x] = w < 0 ? (int)(-0.5 + w * (double)(1 << PREC)) : (int)(0.5 + w * (double)(1 << PREC));
    }
}

// pixel (yy, xx) of the box [ul - pad, br + pad): the source image where it covers it, zero elsewhere
__device__ __forceinline__ void box_pixel(const whmr_augment_item& it, int yy, int xx, int pad, float v[3]) {
    const int sy = it.ul_y - pad + yy, sx = it.ul_x - pad + xx;
    const bool in = yy >= 0 && xx >= 0 && yy < it.bh + 2 * pad && xx < it.bw + 2 * pad && (unsigned)sy < (unsigned)it.H && (unsigned)sx < (unsigned)it.W;
    if (in) {
        const uint8_t* p = it.img + (int64_t)sy * it.row_stride + (int64_t)sx * 3;
        v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
    } else {
        v[0] = v[1] = v[2] = 0.f;
    }
}

// stage 2 for the samples with rot != 0: the rotated box without its pad border, [bh, bw, 3] uint8
__global__ __launch_bounds__(256) void augment_rotate_kernel(const whmr_augment_item* __restrict__ items, uint8_t* __restrict__ rot_scratch) {
    const whmr_augment_item& it = items[blockIdx.y];
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (it.pad <= 0 || idx >= (int64_t)it.bw * it.bh) return;
    const int y = (int)(idx / it.bw), x = (int)(idx % it.bw);
    const double X = (double)(x + it.pad), Y = (double)(y + it.pad);
    const double xi = (it.M[0] * X + it.M[1] * Y) + it.M[2], yi = (it.M[3] * X + it.M[4] * Y) + it.M[5];
    const double xl = floor(xi), yl = floor(yi);
    const int x_lo = (int)xl, y_lo = (int)yl, x_hi = (int)ceil(xi), y_hi = (int)ceil(yi);
    const float a = (float)(xi - xl), b = (float)(yi - yl);
    float v00[3], v01[3], v10[3], v11[3];
    box_pixel(it, y_lo, x_lo, it.pad, v00); box_pixel(it, y_lo, x_hi, it.pad, v01);
    box_pixel(it, y_hi, x_lo, it.pad, v10); box_pixel(it, y_hi, x_hi, it.pad, v11);
    uint8_t* o = rot_scratch + it.rot_off + idx * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float top = v00[c] + a * (v01[c] - v00[c]), bot = v10[c] + a * (v11[c] - v10[c]);
        const float v = top + b * (bot - top);
        o[c] = (uint8_t)fminf(fmaxf(v, 0.f), 255.f);                    // truncation (imutils.py:83)
    }
}

__device__ __forceinline__ int clip8(int acc) { return min(max(acc >> PREC, 0), 255); }

// stage 3, horizontal: columns 32 .. 223 of the 256 -> mid [bh, 192, 3] uint8
__global__ __launch_bounds__(256) void augment_hpass_kernel(const whmr_augment_item* __restrict__ items, const int32_t* __restrict__ coef,
                                                            const uint8_t* __restrict__ rot_scratch, uint8_t* __restrict__ mid) {
    const whmr_augment_item& it = items[blockIdx.y];
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)it.bh * OUT_W) return;
    const int y = (int)(idx / OUT_W), xx = X0 + (int)(idx % OUT_W);
    const int32_t* row = coef + it.coef_off + (int64_t)xx * (2 + it.ksize_x);
    const int xmin = row[0], n = row[1];
    int acc[3] = {1 << (PREC - 1), 1 << (PREC - 1), 1 << (PREC - 1)};
    if (it.pad > 0) {
        const uint8_t* p = rot_scratch + it.rot_off + ((int64_t)y * it.bw + xmin) * 3;
        for (int k = 0; k < n; ++k, p += 3) {
            const int w = row[2 + k];
            acc[0] += w * p[0]; acc[1] += w * p[1]; acc[2] += w * p[2];
        }
    } else {
        const int sy = it.ul_y + y;
        if ((unsigned)sy < (unsigned)it.H) {
            const uint8_t* line = it.img + (int64_t)sy * it.row_stride;
            for (int k = 0; k < n; ++k) {
                const int sx = it.ul_x + xmin + k;
                if ((unsigned)sx < (unsigned)it.W) {
                    const int w = row[2 + k];
                    const uint8_t* p = line + (int64_t)sx * 3;
                    acc[0] += w * p[0]; acc[1] += w * p[1]; acc[2] += w * p[2];
                }
            }
        }
    }
    uint8_t* o = mid + it.mid_off + idx * 3;
    o[0] = (uint8_t)clip8(acc[0]); o[1] = (uint8_t)clip8(acc[1]); o[2] = (uint8_t)clip8(acc[2]);
}

// stage 4a: the occluder bank (RGBA texels, objects back to back), its table of (byte offset, h, w) per object, the paste rows
// (object, nw, nh, start_x, start_y) of the whole batch and the [B + 1] row pointers into them
struct occluder_args {
    const uint8_t* bank; int64_t bank_bytes;
    const int64_t* table; int n_objects;
    const int32_t* pastes; const int32_t* paste_ptr; int n_pastes;
};
#define OCC_MAX_SIDE 32767          // u * w and j * n stay below 2^30

// the pastes of sample b over pixel (x, y) of the 256 x 256 patch, in order; rows [wg_y0, wg_y1] are those of the calling workgroup.  Everything up
// to the rectangle test depends on blockIdx only: the loop's trip count and its early exits are workgroup-uniform, the rows are scalar loads.
__device__ __forceinline__ void occlude_pixel(const occluder_args& oc, int b, int x, int y, int wg_y0, int wg_y1, int px[3]) {
    const int p0 = max(oc.paste_ptr[b], 0), p1 = min(oc.paste_ptr[b + 1], oc.n_pastes);         // never a row outside the paste array
    for (int p = p0; p < p1; ++p) {
        const int32_t* ps = oc.pastes + (int64_t)p * 5;
        const int oi = ps[0], nw = ps[1], nh = ps[2], sx = ps[3], sy = ps[4];
        if (nw <= 0 || nh <= 0 || sy > wg_y1 || (int64_t)sy + nh <= wg_y0 || (unsigned)oi >= (unsigned)oc.n_objects) continue;
        const int64_t off = oc.table[3 * (int64_t)oi], h64 = oc.table[3 * (int64_t)oi + 1], w64 = oc.table[3 * (int64_t)oi + 2];
        if (off < 0 || (off & 3) || h64 < 1 || w64 < 1 || h64 > OCC_MAX_SIDE || w64 > OCC_MAX_SIDE || nw > w64 || nh > h64
            || h64 * w64 * 255 >= ((int64_t)1 << 31) || off + h64 * w64 * 4 > oc.bank_bytes) continue;                                  // an object that is not wholly inside the bank is not read
        const int h = (int)h64, w = (int)w64;
        const int64_t u64 = (int64_t)x - sx, v64 = (int64_t)y - sy;
        if (u64 < 0 || u64 >= nw || v64 < 0 || v64 >= nh) continue;                            // per lane from here on
        const int u = (int)u64, v = (int)v64;
        const uint32_t* tex = (const uint32_t*)(oc.bank + off);                                // one texel = R | G << 8 | B << 16 | A << 24
        const int ux0 = u * w, ux1 = ux0 + w, vy0 = v * h, vy1 = vy0 + h;                      // the output texel's extent in 1 / nw, 1 / nh texels
        const int jx0 = ux0 / nw, jx1 = min((ux1 - 1) / nw, w - 1), jy0 = vy0 / nh, jy1 = min((vy1 - 1) / nh, h - 1);
        uint32_t sum[4] = {0u, 0u, 0u, 0u};                                                     // <= 255 w h < 2^31 (the host rejects larger objects)
        for (int jy = jy0; jy <= jy1; ++jy) {
            const uint32_t wy = (uint32_t)(min((jy + 1) * nh, vy1) - max(jy * nh, vy0));
            const uint32_t* line = tex + (int64_t)jy * w;
            uint32_t r[4] = {0u, 0u, 0u, 0u};
            for (int jx = jx0; jx <= jx1; ++jx) {
                const uint32_t wx = (uint32_t)(min((jx + 1) * nw, ux1) - max(jx * nw, ux0));
                const uint32_t t = line[jx];
                r[0] += wx * (t & 255u); r[1] += wx * ((t >> 8) & 255u); r[2] += wx * ((t >> 16) & 255u); r[3] += wx * (t >> 24);
            }
            sum[0] += wy * r[0]; sum[1] += wy * r[1]; sum[2] += wy * r[2]; sum[3] += wy * r[3];
        }
        const uint32_t D = (uint32_t)w * (uint32_t)h;
        uint32_t val[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {                                                           // (2 sum + D) // (2 D) without leaving 32 bits
            const uint32_t q = sum[c] / D, rem = sum[c] - q * D;
            val[c] = q + (2u * rem >= D ? 1u : 0u);
        }
        const float a = __fdiv_rn((float)val[3], 255.0f), na = 1.0f - a;
#pragma unroll
        for (int c = 0; c < 3; ++c) px[c] = (int)(a * (float)val[c] + na * (float)px[c]);      // truncation into the uint8 patch
    }
}

// stage 3, vertical + stages 4, 5 (OCC: + stage 4a between them; the instantiation without it is the kernel of whmr_augment_crop)
template <bool OCC>
__global__ __launch_bounds__(256) void augment_vpass_kernel(const whmr_augment_item* __restrict__ items, const int32_t* __restrict__ coef,
                                                            const uint8_t* __restrict__ mid, float* __restrict__ out, uint8_t* __restrict__ raw,
                                                            float m0, float m1, float m2, float s0, float s1, float s2, occluder_args oc) {
    const int b = blockIdx.y;
    const whmr_augment_item& it = items[b];
    const int idx = blockIdx.x * 256 + threadIdx.x;              // grid.x = 256 * 192 / 256
    const int yy = idx / OUT_W, j = idx % OUT_W;
    const int jj = it.flip ? OUT_W - 1 - j : j;                   // column 255 - (32 + j) of the 256 = mid column 191 - j
    const int32_t* row = coef + it.coef_off + (int64_t)RES * (2 + it.ksize_x) + (int64_t)yy * (2 + it.ksize_y);
    const int ymin = row[0], n = row[1];
    int acc[3] = {1 << (PREC - 1), 1 << (PREC - 1), 1 << (PREC - 1)};
    const uint8_t* p = mid + it.mid_off + ((int64_t)ymin * OUT_W + jj) * 3;
    for (int k = 0; k < n; ++k, p += OUT_W * 3) {
        const int w = row[2 + k];
        acc[0] += w * p[0]; acc[1] += w * p[1]; acc[2] += w * p[2];
    }
    int px[3] = {clip8(acc[0]), clip8(acc[1]), clip8(acc[2])};
    if constexpr (OCC) occlude_pixel(oc, b, X0 + j, yy, (int)(blockIdx.x * 256) / OUT_W, (int)(blockIdx.x * 256 + 255) / OUT_W, px);
    const float mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double noisy = fmin(255.0, fmax(0.0, (double)px[c] * it.pn[c]));
        const int v = (int)noisy;                                 // the float product goes back into a uint8 array (base_dataset.py:202-204)
        out[(((int64_t)b * 3 + c) * RES + yy) * OUT_W + j] = __fdiv_rn(__fdiv_rn((float)v, 255.0f) - mean[c], sd[c]);
        if (raw) raw[(((int64_t)b * RES + yy) * OUT_W + j) * 3 + c] = (uint8_t)v;
    }
}

static int augment_crop_launch(const void* items, int B, int max_box_w, int max_box_h, int any_rot, void* rot_scratch, void* mid_scratch,
                               int32_t* coef_scratch, float* out, uint8_t* raw, const float* mean3, const float* std3, const occluder_args* oc,
                               void* stream) {
    if (B <= 0 || max_box_w <= 0 || max_box_h <= 0) return (int)hipErrorInvalidValue;
    const whmr_augment_item* it = (const whmr_augment_item*)items;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(augment_coef_kernel, dim3(2, B), dim3(256), 0, s, it, coef_scratch);
    WHMR_CHECK_LAUNCH();
    if (any_rot) {
        hipLaunchKernelGGL(augment_rotate_kernel, dim3((unsigned)(((int64_t)max_box_w * max_box_h + 255) / 256), B), dim3(256), 0, s, it,
                           (uint8_t*)rot_scratch);
        WHMR_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(augment_hpass_kernel, dim3((unsigned)(((int64_t)max_box_h * OUT_W + 255) / 256), B), dim3(256), 0, s, it, coef_scratch,
                       (const uint8_t*)rot_scratch, (uint8_t*)mid_scratch);
    WHMR_CHECK_LAUNCH();
    if (oc)
        hipLaunchKernelGGL(augment_vpass_kernel<true>, dim3(RES * OUT_W / 256, B), dim3(256), 0, s, it, coef_scratch, (const uint8_t*)mid_scratch, out,
                           raw, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], *oc);
    else
        hipLaunchKernelGGL(augment_vpass_kernel<false>, dim3(RES * OUT_W / 256, B), dim3(256), 0, s, it, coef_scratch, (const uint8_t*)mid_scratch, out,
                           raw, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], occluder_args{});
    WHMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int whmr_augment_crop(const void* items, int B, int max_box_w, int max_box_h, int any_rot, void* rot_scratch, void* mid_scratch,
                                 int32_t* coef_scratch, float* out, uint8_t* raw, const float* mean3, const float* std3, void* stream) {
    return augment_crop_launch(items, B, max_box_w, max_box_h, any_rot, rot_scratch, mid_scratch, coef_scratch, out, raw, mean3, std3, nullptr, stream);
}

extern "C" int whmr_augment_crop_occluded(const void* items, int B, int max_box_w, int max_box_h, int any_rot, void* rot_scratch, void* mid_scratch,
                                          int32_t* coef_scratch, float* out, uint8_t* raw, const float* mean3, const float* std3,
                                          const uint8_t* bank, int64_t bank_bytes, const int64_t* bank_table, int n_objects, const int32_t* pastes,
                                          const int32_t* paste_ptr, int n_pastes, void* stream) {
    if (n_pastes < 0 || n_objects < 0 || bank_bytes < 0) return (int)hipErrorInvalidValue;
    if (n_pastes > 0 && (!bank || ((uintptr_t)bank & 3) || bank_bytes < 4 || !bank_table || n_objects < 1 || !pastes || !paste_ptr)) return (int)hipErrorInvalidValue;
    const occluder_args oc = {bank, bank_bytes, bank_table, n_objects, pastes, paste_ptr, n_pastes};
    return augment_crop_launch(items, B, max_box_w, max_box_h, any_rot, rot_scratch, mid_scratch, coef_scratch, out, raw, mean3, std3,
                               n_pastes > 0 ? &oc : nullptr, stream);
}

// ----------------------------------------------------------------------------- labels
// out[i] = in[PERM[i]]: the mirror permutations of w-hmr_amd/core/constants.py
__constant__ int8_t PERM_SMPL24[24] = {0, 2, 1, 3, 5, 4, 6, 8, 7, 9, 11, 10, 12, 14, 13, 15, 17, 16, 19, 18, 21, 20, 23, 22};
__constant__ int8_t PERM_J24[24] = {5, 4, 3, 2, 1, 0, 11, 10, 9, 8, 7, 6, 12, 13, 14, 15, 16, 17, 18, 19, 21, 20, 23, 22};
__constant__ int8_t PERM_OP25[25] = {0, 1, 5, 6, 7, 2, 3, 4, 8, 12, 13, 14, 9, 10, 11, 16, 15, 18, 17, 22, 23, 24, 19, 20, 21};

__device__ __forceinline__ int perm24(int i, int is_smpl) { return is_smpl ? PERM_SMPL24[i] : PERM_J24[i]; }
__device__ __forceinline__ int perm49(int i, int is_smpl) { return i < 25 ? PERM_OP25[i] : 25 + perm24(i - 25, is_smpl); }

// j2d_processing of one point before its flip: transform(kp + 1) with its astype(int) + 1, then 2 v / 256 - 1
__device__ __forceinline__ void j2d_point(const double* T, double x, double y, double& nx, double& ny) {
    const double px = (x + 1.0) - 1.0, py = (y + 1.0) - 1.0;
    const double u = (T[0] * px + T[1] * py) + T[2], v = (T[3] * px + T[4] * py) + T[5];
    nx = 2.0 * (double)((long long)u + 1) / 256.0 - 1.0;
    ny = 2.0 * (double)((long long)v + 1) / 256.0 - 1.0;
}

// rot_aa (imutils.py:135-146): Rodrigues -> R_z(-rot) . R -> axis-angle (cv2's branch for sin(theta) / 2 < 1e-5)
__device__ void rot_aa3(const double* aa, double cs, double sn, double* out) {
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const double theta = sqrt(aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2]);
    if (theta >= 2.220446049250313e-16) {
        const double c = cos(theta), s = sin(theta), c1 = 1.0 - c, x = aa[0] / theta, y = aa[1] / theta, z = aa[2] / theta;
        R[0] = c + c1 * x * x; R[1] = c1 * x * y - s * z; R[2] = c1 * x * z + s * y;
        R[3] = c1 * x * y + s * z; R[4] = c + c1 * y * y; R[5] = c1 * y * z - s * x;
        R[6] = c1 * x * z - s * y; R[7] = c1 * y * z + s * x; R[8] = c + c1 * z * z;
    }
    double Q[9];
    for (int j = 0; j < 3; ++j) {
        Q[j] = cs * R[j] - sn * R[3 + j];
        Q[3 + j] = sn * R[j] + cs * R[3 + j];
        Q[6 + j] = R[6 + j];
    }
    double r[3] = {Q[7] - Q[5], Q[2] - Q[6], Q[3] - Q[1]};
    const double s = sqrt((r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) * 0.25);
    const double c = fmin(1.0, fmax(-1.0, (Q[0] + Q[4] + Q[8] - 1.0) * 0.5));
    const double th = acos(c);
    if (s < 1e-5) {
        if (c > 0) { out[0] = out[1] = out[2] = 0.0; return; }
        double x = sqrt(fmax((Q[0] + 1.0) * 0.5, 0.0));
        double y = sqrt(fmax((Q[4] + 1.0) * 0.5, 0.0)) * (Q[1] < 0 ? -1.0 : 1.0);
        double z = sqrt(fmax((Q[8] + 1.0) * 0.5, 0.0)) * (Q[2] < 0 ? -1.0 : 1.0);
        if (fabs(x) < fabs(y) && fabs(x) < fabs(z) && (Q[5] > 0) != (y * z > 0)) z = -z;
        const double k = th / sqrt(x * x + y * y + z * z);
        out[0] = x * k; out[1] = y * k; out[2] = z * k;
        return;
    }
    const double k = th / (2.0 * s);
    out[0] = r[0] * k; out[1] = r[1] * k; out[2] = r[2] * k;
}

__global__ __launch_bounds__(128) void augment_labels_kernel(const whmr_augment_item* __restrict__ items, whmr_augment_labels_io io) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const whmr_augment_item& it = items[b];
    const int64_t n = it.sample_index;
    const int flip = it.flip, pad = it.pad;
    const int ul_x = it.ul_x - pad, ul_y = it.ul_y - pad, br_x = it.ul_x + it.bw + pad, br_y = it.ul_y + it.bh + pad;      // get_crop_shape
    const float res_x = (float)(br_x - ul_x), res_y = (float)(br_y - ul_y);
    const float has_smpl = io.has_smpl[n];
    __shared__ double root[3];
    if (tid == 0 && has_smpl != 0.f) rot_aa3(io.pose + n * 72, it.aa_cs[0], it.aa_cs[1], root);
    __syncthreads();

    for (int i = tid; i < 49; i += 128) {                          // keypoints, keypoints_world (base_dataset.py:326-342)
        const double* k = io.keypoints + (n * 49 + (flip ? perm49(i, it.is_smpl) : i)) * 3;
        double nx, ny;
        j2d_point(it.T, k[0], k[1], nx, ny);
        const float kx = (float)(flip ? -nx : nx), ky = (float)ny, kc = (float)k[2];
        float* o = io.o_keypoints + ((int64_t)b * 49 + i) * 3;
        o[0] = kx; o[1] = ky; o[2] = kc;
        float wx = (0.5f * res_x) * (kx + 1.f) + (float)ul_x, wy = (0.5f * res_y) * (ky + 1.f) + (float)ul_y;
        wx = __fdiv_rn(2.f * wx, (float)it.W) - 1.f;
        wy = __fdiv_rn(2.f * wy, (float)it.H) - 1.f;
        float* w = io.o_keypoints_world + ((int64_t)b * 49 + i) * 3;
        w[0] = wx; w[1] = wy; w[2] = kc;
    }
    for (int i = tid; i < 24; i += 128) {                          // smpl_2dkps (:307-317), pose_3d (:319-324)
        float* o = io.o_smpl_2dkps + ((int64_t)b * 24 + i) * 3;
        o[0] = o[1] = o[2] = 0.f;
        if (io.smpl_2dkps) {
            const double* k = io.smpl_2dkps + (n * 24 + (flip ? PERM_SMPL24[i] : i)) * 3;
            double nx, ny;
            j2d_point(it.T, k[0], k[1], nx, ny);
            float kx = (float)nx, ky = (float)ny;
            const float kc = (float)k[2];
            if (kc == 0.f) kx = ky = 0.f;
            o[0] = flip ? -kx : kx; o[1] = ky; o[2] = kc;
        }
        float* p = io.o_pose_3d + ((int64_t)b * 24 + i) * 4;
        p[0] = p[1] = p[2] = p[3] = 0.f;
        if (io.S) {
            const double* s = io.S + (n * 24 + (flip ? perm24(i, it.is_smpl) : i)) * 4;
            double x = s[0], y = s[1];
            if (it.rot != 0.0) {
                const double cs = it.j3d_cs[0], sn = it.j3d_cs[1];
                x = cs * s[0] - sn * s[1];
                y = sn * s[0] + cs * s[1];
            }
            p[0] = (float)(flip ? -x : x); p[1] = (float)y; p[2] = (float)s[2]; p[3] = (float)s[3];
        }
    }
    for (int i = tid; i < 72; i += 128) {                          // pose (:238-247, 294-303)
        float v = 0.f;
        if (has_smpl != 0.f) {
            const int src = flip ? 3 * PERM_SMPL24[i / 3] + i % 3 : i;
            double d = src < 3 ? root[src] : io.pose[n * 72 + src];
            if (flip && i % 3 != 0) d = -d;
            v = (float)d;
        }
        io.o_pose[(int64_t)b * 72 + i] = v;
    }
    for (int i = tid; i < 10; i += 128) io.o_betas[(int64_t)b * 10 + i] = has_smpl != 0.f ? (float)io.betas[n * 10 + i] : 0.f;
    for (int i = tid; i < 431; i += 128) io.o_meta_mask[(int64_t)b * 431 + i] = io.mask[(int64_t)b * 431 + i] ? 1.f : 0.f;
    if (tid == 64) {                                                // scalars (:355-373)
        io.o_has_smpl[b] = has_smpl;
        io.o_has_pose_3d[b] = io.S ? 1 : 0;
        io.o_scale[b] = it.scale;
        io.o_center[2 * b] = __fdiv_rn((float)(ul_x + br_x), 2.f);
        io.o_center[2 * b + 1] = __fdiv_rn((float)(ul_y + br_y), 2.f);
        io.o_orig_shape[2 * b] = it.H; io.o_orig_shape[2 * b + 1] = it.W;
        io.o_is_flipped[b] = flip;
        io.o_rot_angle[b] = (float)it.rot;
        io.o_gender[b] = io.gender[n];
        io.o_sample_index[b] = n;
        io.o_bbox_height[b] = res_y; io.o_bbox_width[b] = res_x;
        const float focal = (float)sqrt((double)((int64_t)it.H * it.H + (int64_t)it.W * it.W));
        io.o_focal[b] = focal;
        const double f = (double)focal;
        float* bi = io.o_bbox_info + 5 * (int64_t)b;
        bi[0] = (float)((it.center[0] - (double)it.W / 2.0) / f);
        bi[1] = (float)((it.center[1] - (double)it.H / 2.0) / f);
        bi[2] = (float)((double)res_y / f);
        bi[3] = (float)((double)it.W / f);
        bi[4] = (float)((double)it.H / f);
    }
}

extern "C" int whmr_augment_labels(const void* items, int B, const whmr_augment_labels_io* io, void* stream) {
    if (B <= 0 || !io || !io->keypoints || !io->has_smpl || !io->gender || !io->mask) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(augment_labels_kernel, dim3(B), dim3(128), 0, (hipStream_t)stream, (const whmr_augment_item*)items, *io);
    WHMR_CHECK_LAUNCH();
    return 0;
}

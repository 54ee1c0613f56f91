// IUV ground-truth rasteriser of the training step: replaces pytorch3d's MeshRasterizer(faces_per_pixel=1, blur_radius=0) +
// HardFlatShader(TexturesVertex, AmbientLights) as utils/renderer.py:296-446 (IUV_Renderer.verts2iuvimg) drives it from core/trainer.py:442-464.
// pytorch3d is a third-party dependency absent from the reference tree: its NAIVE rasterisation path is restated (parity unpinned) --
//   * pixel (j, i) samples its centre (i + 0.5, j + 0.5); a face covers it iff all three barycentric coordinates are STRICTLY positive
//     (blur_radius 0: a centre exactly on an edge belongs to no face), faces with |area| <= kEpsilon are skipped, both windings render;
//   * perspective-correct barycentrics  b_i = (w_i / z_i) / sum_j (w_j / z_j),  pixel depth pz = sum_i b_i z_i,  pz < 0 is skipped;
//   * the nearest face wins (ties: the smaller face index -- deterministic: a packed 64-bit atomic-min z-buffer);
//   * the shaded value is the barycentric interpolation of the per-vertex texture (I / 24, U, V), background 0.
// Camera (renderer.py:362-433): R = diag(-1, -1, 1), t = (-cam_1, -cam_2, 2 f / (orig_h cam_0 + 1e-9)), K = [[fx, 0, px], [0, fy, py]] in
// the pixels of the orig_size image; with pytorch3d's screen <-> NDC conventions the two sign flips cancel and a vertex lands at
//   u = W/2 + (W / orig_w) (fx (x + cam_1) / z' + px - orig_w / 2),   v = H/2 + (H / orig_h) (fy (y + cam_2) / z' + py - orig_h / 2),   z' = z + t_z
// (pixel units of the W x H output).  Three launches: clear, one thread per (image, face), one thread per pixel.
//
// Depth target of the training step (cfg.MODEL.PyMAF.DEPTH_SUPV_ON): utils/renderer.py:449-533 (Depth_Renderer.verts2depthimg, driven from
// core/trainer.py:456-460) = MeshRasterizer(blur_radius = ln(1e4) 1e-7, faces_per_pixel = 30) on the same camera, the image being 1 / zbuf[..., 0].
// Same three launches and the same z-buffer key; what differs from the IUV image (pytorch3d's naive path restated again, parity unpinned):
//   * coverage: strictly inside, OR the squared distance of the centre to the nearest of the three edge SEGMENTS, in NDC units (1 px = 2 / W of a
//     square image), is below blur_radius -- a band of sqrt(blur_radius) W / 2 pixels (0.0614 at 128) outside every edge;
//   * depth: blur_radius > 0 switches pytorch3d's clip_barycentric_coords on -- the perspective-correct barycentrics (from the UNclipped screen
//     ones) are clamped to [0, 1] and divided by their sum (floored at 1e-5) before pz = sum_i b_i z_i; pz < 0 is skipped;
//   * output: 1 / (nearest pz), 0 where no face accepts (the reference's where(1 / zbuf == -1, 0): zbuf is -1 on the background).
#include "common.h"

struct raster_cam { float fx, fy, px, py, focal; int orig_h, orig_w, H, W; };

__global__ __launch_bounds__(256) void raster_project_kernel(const float* __restrict__ verts, const int64_t* __restrict__ vmap, const float* __restrict__ cam,
                                                             float* __restrict__ scr, unsigned long long* __restrict__ zbuf, int B, int V, int Vsrc,
                                                             raster_cam c) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long npix = (long)B * c.H * c.W;
    if (idx < npix) zbuf[idx] = ~0ull;
    if (idx >= (long)B * V) return;
    const int b = (int)(idx / V), v = (int)(idx - (long)b * V);
    const int src = vmap ? (int)vmap[v] : v;
    const float* p = verts + ((size_t)b * Vsrc + src) * 3;
    const float s = cam[b * 3], tx = cam[b * 3 + 1], ty = cam[b * 3 + 2];
    const float tz = 2.0f * c.focal / ((float)c.orig_h * s + 1e-9f);
    const float z = p[2] + tz;
    const float u = 0.5f * c.W + ((float)c.W / (float)c.orig_w) * (c.fx * (p[0] + tx) / z + c.px - 0.5f * c.orig_w);
    const float w = 0.5f * c.H + ((float)c.H / (float)c.orig_h) * (c.fy * (p[1] + ty) / z + c.py - 0.5f * c.orig_h);
    scr[idx * 3] = u; scr[idx * 3 + 1] = w; scr[idx * 3 + 2] = z;
}

__device__ __forceinline__ float edge_fn(float ax, float ay, float bx, float by, float px, float py) {
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax);
}

// Per-face setup + per-pixel test.  raster_setup: signed doubled area (|area| <= eps: degenerate, skipped; eps = pytorch3d's kEpsilon = 1e-8 NDC
// units^2 in pixels^2) and the four reciprocals the barycentrics need (1 / area, 1 / z_i: v_rcp_f32, 1 ulp -- the float64 oracle comparison is
// gated at 1e-3).  raster_bary: the coverage test compares the SIGNS of the three edge functions with the sign of the area (w_i = e_i / area > 0:
// most centres of a face's pixel box lie outside); covered pixels cost one more reciprocal.  Both kernels (z-buffer pass and resolve pass)
// run this one code path, so coverage and depth agree bit for bit between them.
struct raster_tri { float v[9]; float area, ra, rz0, rz1, rz2; };
__device__ __forceinline__ bool raster_setup(raster_tri& t, float eps) {
    t.area = edge_fn(t.v[0], t.v[1], t.v[3], t.v[4], t.v[6], t.v[7]);
    t.ra = __builtin_amdgcn_rcpf(t.area);
    t.rz0 = __builtin_amdgcn_rcpf(t.v[2]); t.rz1 = __builtin_amdgcn_rcpf(t.v[5]); t.rz2 = __builtin_amdgcn_rcpf(t.v[8]);
    return !(t.area <= eps && t.area >= -eps);
}
__device__ __forceinline__ bool raster_bary(const raster_tri& t, float px, float py, float& b0, float& b1, float& b2, float& pz) {
    const float e0 = edge_fn(t.v[3], t.v[4], t.v[6], t.v[7], px, py);
    const float e1 = edge_fn(t.v[6], t.v[7], t.v[0], t.v[1], px, py);
    const float e2 = edge_fn(t.v[0], t.v[1], t.v[3], t.v[4], px, py);
    const bool in = t.area > 0.f ? (e0 > 0.f && e1 > 0.f && e2 > 0.f) : (e0 < 0.f && e1 < 0.f && e2 < 0.f);
    if (!in) return false;
    const float q0 = (e0 * t.ra) * t.rz0, q1 = (e1 * t.ra) * t.rz1, q2 = (e2 * t.ra) * t.rz2;
    const float rden = __builtin_amdgcn_rcpf((q0 + q1) + q2);
    b0 = q0 * rden; b1 = q1 * rden; b2 = q2 * rden;
    pz = (b0 * t.v[2] + b1 * t.v[5]) + b2 * t.v[8];
    return pz >= 0.f;
}

// Depth target: coverage with the blur band, depth from the clipped and renormalised perspective-correct barycentrics (see the head of the file).
__device__ __forceinline__ float raster_seg_dist2(float ax, float ay, float bx, float by, float px, float py) {
    const float dx = bx - ax, dy = by - ay;
    const float l2 = dx * dx + dy * dy;
    float s = l2 > 0.f ? ((px - ax) * dx + (py - ay) * dy) / l2 : 0.f;
    s = fminf(fmaxf(s, 0.f), 1.f);
    const float qx = px - (ax + s * dx), qy = py - (ay + s * dy);
    return qx * qx + qy * qy;
}
__device__ __forceinline__ bool raster_bary_blur(const raster_tri& t, float px, float py, float band2, float& pz) {
    const float e0 = edge_fn(t.v[3], t.v[4], t.v[6], t.v[7], px, py);
    const float e1 = edge_fn(t.v[6], t.v[7], t.v[0], t.v[1], px, py);
    const float e2 = edge_fn(t.v[0], t.v[1], t.v[3], t.v[4], px, py);
    const bool in = t.area > 0.f ? (e0 > 0.f && e1 > 0.f && e2 > 0.f) : (e0 < 0.f && e1 < 0.f && e2 < 0.f);
    if (!in) {
        const float d2 = fminf(raster_seg_dist2(t.v[0], t.v[1], t.v[3], t.v[4], px, py),
                               fminf(raster_seg_dist2(t.v[3], t.v[4], t.v[6], t.v[7], px, py), raster_seg_dist2(t.v[6], t.v[7], t.v[0], t.v[1], px, py)));
        if (!(d2 < band2)) return false;
    }
    const float q0 = (e0 * t.ra) * t.rz0, q1 = (e1 * t.ra) * t.rz1, q2 = (e2 * t.ra) * t.rz2;
    const float rden = __builtin_amdgcn_rcpf((q0 + q1) + q2);
    float b0 = fminf(fmaxf(q0 * rden, 0.f), 1.f), b1 = fminf(fmaxf(q1 * rden, 0.f), 1.f), b2 = fminf(fmaxf(q2 * rden, 0.f), 1.f);
    const float sum = fmaxf((b0 + b1) + b2, 1e-5f);
    b0 /= sum; b1 /= sum; b2 /= sum;
    pz = (b0 * t.v[2] + b1 * t.v[5]) + b2 * t.v[8];
    return pz >= 0.f;                                                                      // false for NaN too
}

// One lane per (image, face) finds the face's pixel box; boxes of at most RASTER_SMALL pixels (a real SMPL mesh at 128 x 128: 1-4 pixels per
// face) are walked by that lane, larger ones by the WHOLE wave, 64 pixels at a time (the face's setup is broadcast with readlane): a mesh with
// a few large triangles -- or the synthetic benchmark mesh, whose random skinning weights stretch every face over a good part of the image --
// costs sum(box) / 64 per wave instead of max(box).  Same per-pixel arithmetic on both paths (bit-identical coverage).
#define RASTER_SMALL 16
template <bool BLUR>
__device__ __forceinline__ void raster_pixel(const raster_tri& t, int x, int y, int f, unsigned long long* __restrict__ zrow0, int W, float band2) {
    float b0, b1, b2, pz;
    if constexpr (BLUR) {
        if (!raster_bary_blur(t, x + 0.5f, y + 0.5f, band2, pz)) return;
    } else {
        if (!raster_bary(t, x + 0.5f, y + 0.5f, b0, b1, b2, pz)) return;
    }
    const unsigned long long key = ((unsigned long long)__float_as_uint(pz) << 32) | (unsigned)f;
    // the z-buffer only ever decreases: a plain (L2-scope) look first drops the faces that are already hidden -- with n faces over a pixel in
    // random depth order ~ln(n) of them still need the atomic
    unsigned long long* z = zrow0 + (size_t)y * W + x;
    if (__hip_atomic_load(z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(z, key);
}

// BLUR (the depth target): the pixel box grows by the band (``band`` pixels, ``band2`` = its square) and the per-pixel test is raster_bary_blur
template <bool BLUR>
__global__ __launch_bounds__(256) void raster_faces_kernel(const float* __restrict__ scr, const int32_t* __restrict__ faces, unsigned long long* __restrict__ zbuf,
                                                           int B, int V, int F, int H, int W, float band, float band2) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const float eps = 1e-8f * 0.25f * H * W;
    raster_tri t;
    int x0 = 0, x1 = -1, y0 = 0, y1 = -1, f = 0, b = 0;
    if (idx < (long)B * F) {
        b = (int)(idx / F); f = (int)(idx - (long)b * F);
        const float* s = scr + (size_t)b * V * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float* vp = s + faces[f * 3 + k] * 3;
            t.v[3 * k] = vp[0]; t.v[3 * k + 1] = vp[1]; t.v[3 * k + 2] = vp[2];
        }
        const float xmin = fminf(t.v[0], fminf(t.v[3], t.v[6])), xmax = fmaxf(t.v[0], fmaxf(t.v[3], t.v[6]));
        const float ymin = fminf(t.v[1], fminf(t.v[4], t.v[7])), ymax = fmaxf(t.v[1], fmaxf(t.v[4], t.v[7]));
        const float grow = BLUR ? band : 0.f;
        if (xmax + grow >= 0.f && ymax + grow >= 0.f && xmin - grow <= (float)W && ymin - grow <= (float)H) {        // also drops NaN vertices
            x0 = (int)floorf(xmin - grow - 0.5f); x1 = (int)ceilf(xmax + grow - 0.5f);
            y0 = (int)floorf(ymin - grow - 0.5f); y1 = (int)ceilf(ymax + grow - 0.5f);
            x0 = x0 < 0 ? 0 : x0; y0 = y0 < 0 ? 0 : y0; x1 = x1 > W - 1 ? W - 1 : x1; y1 = y1 > H - 1 ? H - 1 : y1;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) t.v[k] = 1.f;
    }
    const bool ok = raster_setup(t, eps);
    const int bw = x1 - x0 + 1, bh = y1 - y0 + 1;
    const int npx = (bw > 0 && bh > 0 && ok) ? bw * bh : 0;
    if (npx > 0 && npx <= RASTER_SMALL) {
        unsigned long long* z0 = zbuf + (size_t)b * H * W;
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x) raster_pixel<BLUR>(t, x, y, f, z0, W, band2);
    }
    unsigned long long big = __ballot(npx > RASTER_SMALL);
    while (big) {
        const int L = __ffsll((long long)big) - 1;
        big &= big - 1;
        raster_tri u;
#pragma unroll
        for (int k = 0; k < 9; ++k) u.v[k] = __shfl(t.v[k], L, 64);
        u.area = __shfl(t.area, L, 64); u.ra = __shfl(t.ra, L, 64);
        u.rz0 = __shfl(t.rz0, L, 64); u.rz1 = __shfl(t.rz1, L, 64); u.rz2 = __shfl(t.rz2, L, 64);
        const int ux0 = __shfl(x0, L, 64), uy0 = __shfl(y0, L, 64), ux1 = __shfl(x1, L, 64), uy1 = __shfl(y1, L, 64);
        const int uf = __shfl(f, L, 64), ub = __shfl(b, L, 64);
        unsigned long long* z0 = zbuf + (size_t)ub * H * W;
        // the box in 64-pixel tiles shaped after its height (64 x 1 ... 8 x 8), lane = pixel of the tile: no per-pixel index division
        const int uh = uy1 - uy0 + 1;
        const int lw = uh <= 1 ? 6 : uh <= 2 ? 5 : uh <= 4 ? 4 : 3;               // log2 of the tile width
        const int tw = 1 << lw, th = 64 >> lw;
        const int lx = lane & (tw - 1), ly = lane >> lw;
        for (int ty = uy0; ty <= uy1; ty += th)
            for (int tx = ux0; tx <= ux1; tx += tw) {
                const int x = tx + lx, y = ty + ly;
                if (x <= ux1 && y <= uy1) raster_pixel<BLUR>(u, x, y, uf, z0, W, band2);
            }
    }
}

__global__ __launch_bounds__(256) void raster_resolve_kernel(const float* __restrict__ scr, const int32_t* __restrict__ faces, const float* __restrict__ tex,
                                                             const unsigned long long* __restrict__ zbuf, float* __restrict__ out, int32_t* __restrict__ face_out,
                                                             int B, int V, int H, int W) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * H * W) return;
    const int b = (int)(idx / ((long)H * W)), r = (int)(idx - (long)b * H * W);
    const int y = r / W, x = r - y * W;
    const unsigned long long key = zbuf[idx];
    float o0 = 0.f, o1 = 0.f, o2 = 0.f;
    int fid = -1;
    if (key != ~0ull) {
        fid = (int)(key & 0xffffffffu);
        const float* s = scr + (size_t)b * V * 3;
        const int i0 = faces[fid * 3], i1 = faces[fid * 3 + 1], i2 = faces[fid * 3 + 2];
        raster_tri t;
#pragma unroll
        for (int k = 0; k < 3; ++k) { t.v[k] = s[i0 * 3 + k]; t.v[3 + k] = s[i1 * 3 + k]; t.v[6 + k] = s[i2 * 3 + k]; }
        raster_setup(t, 0.f);
        float b0, b1, b2, pz;
        if (raster_bary(t, x + 0.5f, y + 0.5f, b0, b1, b2, pz)) {
            o0 = (b0 * tex[i0 * 3] + b1 * tex[i1 * 3]) + b2 * tex[i2 * 3];
            o1 = (b0 * tex[i0 * 3 + 1] + b1 * tex[i1 * 3 + 1]) + b2 * tex[i2 * 3 + 1];
            o2 = (b0 * tex[i0 * 3 + 2] + b1 * tex[i1 * 3 + 2]) + b2 * tex[i2 * 3 + 2];
        }
    }
    const size_t plane = (size_t)H * W;
    float* o = out + (size_t)b * 3 * plane + r;
    o[0] = o0; o[plane] = o1; o[2 * plane] = o2;
    if (face_out) face_out[idx] = fid;
}

// verts [B, Vsrc, 3] fp32; vmap [V] int64 or null (DensePose vertex duplication, renderer.py:303-304,419-422); faces [F, 3] int32 into the V
// mapped vertices; tex [V, 3]; cam [B, 3] = (s, tx, ty); scratch: scr [B, V, 3] fp32, zbuf [B, H, W] uint64; out [B, 3, H, W]; face_out
// [B, H, W] int32 or null (covering face, -1 = background).
extern "C" int whmr_iuv_rasterize(const float* verts, int B, int Vsrc, const int64_t* vmap, int V, const int32_t* faces, int F, const float* tex,
                                  const float* cam, float fx, float fy, float px, float py, float focal, int orig_h, int orig_w, int H, int W, float* scr,
                                  void* zbuf, float* out, int32_t* face_out, void* stream) {
    if (B <= 0 || V <= 0 || F <= 0 || H <= 0 || W <= 0 || orig_h <= 0 || orig_w <= 0) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    raster_cam c{fx, fy, px, py, focal, orig_h, orig_w, H, W};
    const long n0 = (long)B * V > (long)B * H * W ? (long)B * V : (long)B * H * W;
    hipLaunchKernelGGL(raster_project_kernel, dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0, st, verts, vmap, cam, scr, (unsigned long long*)zbuf, B, V, Vsrc, c);
    WHMR_CHECK_LAUNCH();
    hipLaunchKernelGGL(raster_faces_kernel<false>, dim3((unsigned)(((long)B * F + 255) / 256)), dim3(256), 0, st, scr, faces, (unsigned long long*)zbuf, B, V, F,
                       H, W, 0.f, 0.f);
    WHMR_CHECK_LAUNCH();
    hipLaunchKernelGGL(raster_resolve_kernel, dim3((unsigned)(((long)B * H * W + 255) / 256)), dim3(256), 0, st, scr, faces, tex,
                       (const unsigned long long*)zbuf, out, face_out, B, V, H, W);
    WHMR_CHECK_LAUNCH();
    return 0;
}

// the z-buffer key already holds the nearest accepted pz (its high word): nothing is recomputed
__global__ __launch_bounds__(256) void depth_resolve_kernel(const unsigned long long* __restrict__ zbuf, float* __restrict__ out, int32_t* __restrict__ face_out,
                                                            long npix) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= npix) return;
    const unsigned long long key = zbuf[idx];
    const bool hit = key != ~0ull;
    out[idx] = hit ? 1.0f / __uint_as_float((unsigned)(key >> 32)) : 0.f;
    if (face_out) face_out[idx] = hit ? (int)(key & 0xffffffffu) : -1;
}

// Inverse-depth image of the meshes (see the head of the file): verts [B, V, 3] fp32 (no vertex duplication, no texture); faces [F, 3] int32;
// cam [B, 3]; scratch as whmr_iuv_rasterize; out [B, 1, H, W]; face_out [B, H, W] int32 or null.  H == W (pytorch3d scales the NDC of a
// non-square image differently; the reference's DP_HEATMAP_SIZE is square).
extern "C" int whmr_depth_rasterize(const float* verts, int B, int V, const int32_t* faces, int F, const float* cam, float fx, float fy, float px, float py,
                                    float focal, int orig_h, int orig_w, int H, int W, float* scr, void* zbuf, float* out, int32_t* face_out, void* stream) {
    if (B <= 0 || V <= 0 || F <= 0 || H <= 0 || W != H || orig_h <= 0 || orig_w <= 0) return (int)hipErrorInvalidValue;
    if (!verts || !faces || !cam || !scr || !zbuf || !out) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    raster_cam c{fx, fy, px, py, focal, orig_h, orig_w, H, W};
    const double blur = 9.210340371976182e-7;                                              // ln(1 / 1e-4) * 1e-7, renderer.py:494
    const float band2 = (float)(blur * 0.25 * (double)W * (double)W), band = sqrtf(band2);
    const long npix = (long)B * H * W;
    const long n0 = (long)B * V > npix ? (long)B * V : npix;
    hipLaunchKernelGGL(raster_project_kernel, dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0, st, verts, (const int64_t*)nullptr, cam, scr,
                       (unsigned long long*)zbuf, B, V, V, c);
    WHMR_CHECK_LAUNCH();
    hipLaunchKernelGGL(raster_faces_kernel<true>, dim3((unsigned)(((long)B * F + 255) / 256)), dim3(256), 0, st, scr, faces, (unsigned long long*)zbuf, B, V, F,
                       H, W, band, band2);
    WHMR_CHECK_LAUNCH();
    hipLaunchKernelGGL(depth_resolve_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, (const unsigned long long*)zbuf, out, face_out, npix);
    WHMR_CHECK_LAUNCH();
    return 0;
}

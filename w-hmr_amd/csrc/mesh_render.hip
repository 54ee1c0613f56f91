// Mesh overlay renderer of the demo (replaces utils/renderer_cam.py:41-141 render_overlay_image -- pyrender on an OpenGL / EGL context -- as
// demo/tester.py:176-214 drives it through render_image_group): all persons of a frame drawn over the uint8 frame, on the device, in three launches.
// pyrender and trimesh are third-party and absent from the reference tree, so the scene is restated from the call site and the shader is DEFINED here.
//
// Camera (renderer_cam.py:71-114).  With t' = (-t_x, t_y, t_z) (``camera_translation[0] *= -1``), D = diag(1, -1, -1) (the 180 degree turn about X),
// S = R_y(sideview_angle) and the camera pose [R | R t'], a mesh vertex p stands at  q = S D p  in the world and at  p_c = R^T q - t'  in the camera's
// frame.  IntrinsicsCamera(fx, fy, cx, cy) looks down -z with y up: from its projection matrix a point lands at  u = cx + fx x_c / (-z_c),
// v = cy - fy y_c / (-z_c)  (v counted from the top row) with depth -z_c.  In the computer-vision frame  (X, Y, Z) = D p_c = D R^T S D p + (t_x, t_y, t_z):
//     u = cx + fx X / Z,    v = cy + fy Y / Z,    depth Z,    pixel (j, i) samples its centre (i + 0.5, j + 0.5).
// R = I, no side view:  u = cx + fx (x + t_x) / (z + t_z),  v = cy + fy (y + t_y) / (z + t_z),  depth z + t_z -- perspective_projection (geometry.hip).
//
// Normals: smooth per-vertex normals, the sum of (v1 - v0) x (v2 - v0) (= 2 area x unit normal: area weighting) over the faces around a vertex,
// normalised.  The sum walks a vertex -> face CSR in its stored order: no float atomics, the same bits every run.  trimesh's own weighting (it
// blends by corner angle in some versions) is unpinned.  The normal is kept in the WORLD frame, n_w = S D n, where the lights are.
//
// Coverage: top-left fill rule.  Every edge function is evaluated from the edge's lexicographically smaller end point whatever face asks, and negated
// for the face that walks the edge the other way (exact in floating point), so the two faces of a shared edge see the same number with opposite signs:
// a pixel centre exactly on the edge goes to exactly one of them (the one for which it is a left edge, or a top edge if horizontal).  Both windings
// render.  A face with any vertex at depth <= znear (pyrender's IntrinsicsCamera default 0.05, from memory, unverified: a parameter), a NaN vertex or
// an empty pixel box is dropped whole.  z-buffer key = depth bits << 32 | global face id (person * F + face), 64-bit atomic min: nearest face, ties to
// the smaller id, bit-reproducible (as rasterize.hip).  The IUV kernel's strict-interior rule is pytorch3d's and stays there.
//
// Shading (DEFINED here, a stated deviation):  rgb = clamp(base * (ambient + k_d * max(n . l, 0)), 0, 1).  Every light of renderer_cam.py:116-128 is a
// DirectionalLight whose pose sets a translation only -- a directional light ignores it -- so all four shine along world -z: l = (0, 0, 1) is the
// direction TO the light, k_d = n_lights (1 - metallic) (1 - 0.04) / pi with metallic 0.2, n_lights 4: the diffuse term of the glTF metallic-roughness
// model.  The specular lobe (default roughness 1.0) is left out.  alphaMode 'OPAQUE': alpha does nothing in the reference and is no parameter.
// Background pixels keep the frame's bytes (the valid mask of :138-140, not a blend); uint8 = round-half-even(255 * rgb) of the fp32 colour.
//
// Ground plane (renderer_cam.py:53,95-104: add_ground_plane, on in both side views of render_image_group; whmr_mesh_render_scene below).  The reference
// adds get_checkerboard_plane() -- a PARE helper that is not in the reference tree -- lifted to the mesh's lowest point mesh.bounds[0, 1]; the mesh is
// turned by S, the plane is not (:79-82 against :100-104).  The plane is therefore DEFINED here: the horizontal square |q_x| <= half, |q_z| <= half at
// q_y = h in the world frame (y up), n x n tiles of side 2 half / n, no thickness, seen from both sides, flat UNLIT greys (pyrender would light the
// tiles: a stated deviation): tile (ix, iz) is `dark` where ix + iz is even, else `light`.  h = the lowest world-frame y of the owning draw's mesh:
// S turns about y and D negates y, so h = -max_v p_y over the mesh-frame vertices (NaN vertices skipped), or a height the caller gives.  A plane
// belongs to ONE draw: its camera is that draw's row (cam_t, focal), its image's centre and the call's rot -- the reference moves the camera by t' and
// leaves mesh and plane at the origin, so the floor is centred under that person's root.  It is never triangulated: the resolve pass intersects the
// pixel's ray with it.  From  (X, Y, Z) = D R^T q + t  follows  q = R D ((X, Y, Z) - t);  pixel (j, i) looks along (a, b, 1) Z with
// a = (i + 0.5 - cx) / fx, b = (j + 0.5 - cy) / fy, hence  q = Z w + o,  w = R D (a, b, 1),  o = -R D t,  and the plane is met at depth
// Z_g = (h - o_y) / w_y.  It covers the pixel iff Z_g is finite, Z_g > znear and 0 <= ix, iz < n with ix = floor((q_x + half) / tile),
// iz = floor((q_z + half) / tile); it owns the pixel iff it covers it and no face does or Z_g < the winning face's depth (a tie goes to the mesh).
// A plane pixel counts as covered (the rend_depth > 0 mask of :138): colour = the tile's grey, depth = Z_g, face id -1, `ground` = ix n + iz.
#include "common.h"

struct mesh_cam { float cx, cy, sc, ss; int has_rot; float r[9]; };

// The vertex transform of launch 1, one code path for both entry points: vertex v of the mesh at vp (mesh frame) under camera c with translation t and
// focal lengths fo -> its screen position (u, v, depth) and its world-frame smooth normal.
__device__ __forceinline__ void mesh_vertex(const float* __restrict__ vp, int v, const int32_t* __restrict__ faces, const int32_t* __restrict__ vf_ptr,
                                            const int32_t* __restrict__ vf_idx, const float* __restrict__ t, const float* __restrict__ fo, const mesh_cam& c,
                                            float* __restrict__ scr, float* __restrict__ nrm) {
    // world: q = S D p,  S = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    const float x = vp[v * 3], y = -vp[v * 3 + 1], z = -vp[v * 3 + 2];
    const float qx = c.sc * x + c.ss * z, qy = y, qz = c.sc * z - c.ss * x;
    float px = qx, py = qy, pz = qz;
    if (c.has_rot) {                                                              // p_c = R^T q
        px = (c.r[0] * qx + c.r[3] * qy) + c.r[6] * qz;
        py = (c.r[1] * qx + c.r[4] * qy) + c.r[7] * qz;
        pz = (c.r[2] * qx + c.r[5] * qy) + c.r[8] * qz;
    }
    const float X = px + t[0], Y = t[1] - py, Z = t[2] - pz;
    scr[0] = c.cx + fo[0] * X / Z;
    scr[1] = c.cy + fo[1] * Y / Z;
    scr[2] = Z;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    for (int k = vf_ptr[v]; k < vf_ptr[v + 1]; ++k) {
        const int32_t* f = faces + (size_t)vf_idx[k] * 3;
        const float* a = vp + (size_t)f[0] * 3;
        const float* b = vp + (size_t)f[1] * 3;
        const float* d = vp + (size_t)f[2] * 3;
        const float e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2], e2x = d[0] - a[0], e2y = d[1] - a[1], e2z = d[2] - a[2];
        nx += e1y * e2z - e1z * e2y; ny += e1z * e2x - e1x * e2z; nz += e1x * e2y - e1y * e2x;
    }
    const float inv = __builtin_amdgcn_rsqf(fmaxf((nx * nx + ny * ny) + nz * nz, 1e-30f));
    nx *= inv; ny = -ny * inv; nz = -nz * inv;                                    // D n
    nrm[0] = c.sc * nx + c.ss * nz; nrm[1] = ny; nrm[2] = c.sc * nz - c.ss * nx;
}

// Launch 1: z-buffer clear + one thread per (person, vertex): camera transform, projection, vertex normal.
__global__ __launch_bounds__(256) void mesh_vertex_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, const int32_t* __restrict__ vf_ptr,
                                                          const int32_t* __restrict__ vf_idx, const float* __restrict__ cam_t, const float* __restrict__ focal,
                                                          float* __restrict__ scr, float* __restrict__ nrm, unsigned long long* __restrict__ zbuf, long npix,
                                                          int P, int V, mesh_cam c) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < npix) zbuf[idx] = ~0ull;
    if (idx >= (long)P * V) return;
    const int p = (int)(idx / V), v = (int)(idx - (long)p * V);
    mesh_vertex(verts + (size_t)p * V * 3, v, faces, vf_ptr, vf_idx, cam_t + p * 3, focal + p * 2, c, scr + idx * 3, nrm + idx * 3);
}

// Edge function of the oriented edge a -> b at p, evaluated from the lexicographically smaller end point (see the header): the explicit fma keeps
// the rounding the same at every call site.
__device__ __forceinline__ float mesh_edge(float ax, float ay, float bx, float by, float px, float py) {
    const bool sw = bx < ax || (bx == ax && by < ay);
    const float lx = sw ? bx : ax, ly = sw ? by : ay, hx = sw ? ax : bx, hy = sw ? ay : by;
    const float e = __fmaf_rn(px - lx, hy - ly, -((py - ly) * (hx - lx)));
    return sw ? -e : e;
}
// a -> b is a left edge (the interior, e > 0, lies towards +x) or a top edge (horizontal, interior towards +y: rows grow downwards)
__device__ __forceinline__ bool mesh_top_left(float ax, float ay, float bx, float by) { return by > ay || (by == ay && bx < ax); }

// Per-face setup + per-pixel test, one code path for the z-buffer pass and the resolve pass: coverage and depth agree bit for bit between them.
// The face is taken in the winding that makes its doubled area positive; tl_i: edge i (opposite vertex i) owns the centres lying exactly on it.
struct mesh_tri { float v[9]; float area, ra, rz0, rz1, rz2; bool tl0, tl1, tl2; };
__device__ __forceinline__ bool mesh_setup(mesh_tri& t) {
    t.area = mesh_edge(t.v[0], t.v[1], t.v[3], t.v[4], t.v[6], t.v[7]);
    t.ra = __builtin_amdgcn_rcpf(t.area);
    t.rz0 = __builtin_amdgcn_rcpf(t.v[2]); t.rz1 = __builtin_amdgcn_rcpf(t.v[5]); t.rz2 = __builtin_amdgcn_rcpf(t.v[8]);
    const bool pos = t.area > 0.f;
    t.tl0 = pos ? mesh_top_left(t.v[3], t.v[4], t.v[6], t.v[7]) : mesh_top_left(t.v[6], t.v[7], t.v[3], t.v[4]);
    t.tl1 = pos ? mesh_top_left(t.v[6], t.v[7], t.v[0], t.v[1]) : mesh_top_left(t.v[0], t.v[1], t.v[6], t.v[7]);
    t.tl2 = pos ? mesh_top_left(t.v[0], t.v[1], t.v[3], t.v[4]) : mesh_top_left(t.v[3], t.v[4], t.v[0], t.v[1]);
    return t.area != 0.f && t.area == t.area;
}
__device__ __forceinline__ bool mesh_bary(const mesh_tri& t, float px, float py, float& b0, float& b1, float& b2, float& pz) {
    const float e0 = mesh_edge(t.v[3], t.v[4], t.v[6], t.v[7], px, py);
    const float e1 = mesh_edge(t.v[6], t.v[7], t.v[0], t.v[1], px, py);
    const float e2 = mesh_edge(t.v[0], t.v[1], t.v[3], t.v[4], px, py);
    const float s0 = t.area > 0.f ? e0 : -e0, s1 = t.area > 0.f ? e1 : -e1, s2 = t.area > 0.f ? e2 : -e2;
    const bool in = (s0 > 0.f || (s0 == 0.f && t.tl0)) && (s1 > 0.f || (s1 == 0.f && t.tl1)) && (s2 > 0.f || (s2 == 0.f && t.tl2));
    if (!in) return false;
    const float q0 = (e0 * t.ra) * t.rz0, q1 = (e1 * t.ra) * t.rz1, q2 = (e2 * t.ra) * t.rz2;      // perspective-correct: b_i ~ w_i / z_i
    const float rden = __builtin_amdgcn_rcpf((q0 + q1) + q2);
    b0 = q0 * rden; b1 = q1 * rden; b2 = q2 * rden;
    pz = (b0 * t.v[2] + b1 * t.v[5]) + b2 * t.v[8];
    return pz > 0.f;
}

// Launch 2: one lane per (person, face) finds the face's pixel box; boxes of at most MESH_SMALL pixels are walked by that lane, larger ones by the WHOLE
// wave, 64 pixels at a time (the walk of rasterize.hip: a close-up person at frame resolution has faces of tens to thousands of pixels, a distant one
// of one or two).  Same per-pixel arithmetic on both paths.
#define MESH_SMALL 16
__device__ __forceinline__ void mesh_pixel(const mesh_tri& t, int x, int y, unsigned gid, unsigned long long* __restrict__ z0, int W) {
    float b0, b1, b2, pz;
    if (!mesh_bary(t, x + 0.5f, y + 0.5f, b0, b1, b2, pz)) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(pz) << 32) | gid;
    unsigned long long* z = z0 + (size_t)y * W + x;
    // the z-buffer only ever decreases: a plain look first drops the faces that are already hidden (the far side of every closed mesh)
    if (__hip_atomic_load(z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(z, key);
}

// The face pass, one code path for both entry points.  ``tg`` names the targets: tg.image(p) = the image that mesh instance p is drawn into (negative:
// not drawn), tg.target(img) = that image's size and its first element of the z-buffer.  The wave walk asks for the target of the OWNER lane's image:
// one wave can hold faces of instances whose images differ in size and z-buffer base.
struct mesh_target { int H, W; long off; };
template <class Targets>
__device__ __forceinline__ void mesh_faces(const float* __restrict__ scr, const int32_t* __restrict__ faces, unsigned long long* __restrict__ zbuf, long idx,
                                           long n_faces, int V, int F, float znear, const Targets& tg) {
    const int lane = threadIdx.x & 63;
    mesh_tri t;
    int x0 = 0, x1 = -1, y0 = 0, y1 = -1, img = 0;
    unsigned gid = 0;
    bool ok = false;
    if (idx < n_faces) {
        const int p = (int)(idx / F), f = (int)(idx - (long)p * F);
        gid = (unsigned)idx; img = tg.image(p);
        if (img >= 0) {
            const mesh_target g = tg.target(img);
            const int H = g.H, W = g.W;
            const float* s = scr + (size_t)p * V * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float* vp = s + (size_t)faces[f * 3 + k] * 3;
                t.v[3 * k] = vp[0]; t.v[3 * k + 1] = vp[1]; t.v[3 * k + 2] = vp[2];
            }
            const float xmin = fminf(t.v[0], fminf(t.v[3], t.v[6])), xmax = fmaxf(t.v[0], fmaxf(t.v[3], t.v[6]));
            const float ymin = fminf(t.v[1], fminf(t.v[4], t.v[7])), ymax = fmaxf(t.v[1], fmaxf(t.v[4], t.v[7]));
            // every comparison is false for a NaN, but fminf / fmaxf skip one: the sum of the screen coordinates is looked at as well (inf - inf: dropped too)
            const float any = ((t.v[0] + t.v[1]) + (t.v[3] + t.v[4])) + (t.v[6] + t.v[7]);
            ok = t.v[2] > znear && t.v[5] > znear && t.v[8] > znear && any == any && xmax >= 0.5f && ymax >= 0.5f && xmin <= (float)W - 0.5f &&
                 ymin <= (float)H - 0.5f;
            if (ok) {                                                             // centres i + 0.5 in [min, max]; clamped as floats, so the casts are in range
                x0 = (int)fmaxf(ceilf(xmin - 0.5f), 0.f); x1 = (int)fminf(floorf(xmax - 0.5f), (float)(W - 1));
                y0 = (int)fmaxf(ceilf(ymin - 0.5f), 0.f); y1 = (int)fminf(floorf(ymax - 0.5f), (float)(H - 1));
            }
        } else {
            img = 0;
        }
    }
    if (!ok) {
#pragma unroll
        for (int k = 0; k < 9; ++k) t.v[k] = 1.f;
    }
    ok = mesh_setup(t) && ok;
    const int bw = x1 - x0 + 1, bh = y1 - y0 + 1;
    const int npx = (bw > 0 && bh > 0 && ok) ? bw * bh : 0;
    if (npx > 0 && npx <= MESH_SMALL) {
        const mesh_target g = tg.target(img);
        unsigned long long* z0 = zbuf + g.off;
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x) mesh_pixel(t, x, y, gid, z0, g.W);
    }
    unsigned long long big = __ballot(npx > MESH_SMALL);
    while (big) {
        const int L = __ffsll((long long)big) - 1;
        big &= big - 1;
        mesh_tri u;
#pragma unroll
        for (int k = 0; k < 9; ++k) u.v[k] = __shfl(t.v[k], L, 64);
        mesh_setup(u);                                                            // the same arithmetic on the same inputs: the owner lane's bits
        const int ux0 = __shfl(x0, L, 64), uy0 = __shfl(y0, L, 64), ux1 = __shfl(x1, L, 64), uy1 = __shfl(y1, L, 64);
        const unsigned ug = (unsigned)__shfl((int)gid, L, 64);
        const mesh_target g = tg.target(__shfl(img, L, 64));                      // the owner's image: its width and its z-buffer
        unsigned long long* z0 = zbuf + g.off;
        // the box in 64-pixel tiles shaped after its height (64 x 1 ... 8 x 8), lane = pixel of the tile: no per-pixel index division
        const int uh = uy1 - uy0 + 1;
        const int lw = uh <= 1 ? 6 : uh <= 2 ? 5 : uh <= 4 ? 4 : 3;
        const int tw = 1 << lw, th = 64 >> lw;
        const int lx = lane & (tw - 1), ly = lane >> lw;
        for (int ty = uy0; ty <= uy1; ty += th)
            for (int tx = ux0; tx <= ux1; tx += tw) {
                const int x = tx + lx, y = ty + ly;
                if (x <= ux1 && y <= uy1) mesh_pixel(u, x, y, ug, z0, g.W);
            }
    }
}

struct mesh_frame_targets {                                                       // whmr_mesh_render: images of one size, one for all persons or one each
    int H, W, per_person;
    __device__ __forceinline__ int image(int p) const { return per_person ? p : 0; }
    __device__ __forceinline__ mesh_target target(int img) const { return mesh_target{H, W, (long)img * H * W}; }
};

__global__ __launch_bounds__(256) void mesh_faces_kernel(const float* __restrict__ scr, const int32_t* __restrict__ faces, unsigned long long* __restrict__ zbuf,
                                                         int P, int V, int F, int H, int W, int per_person, float znear) {
    mesh_faces(scr, faces, zbuf, (long)blockIdx.x * 256 + threadIdx.x, (long)P * F, V, F, znear, mesh_frame_targets{H, W, per_person});
}

struct mesh_shade { float r, g, b, ambient, kd, lx, ly, lz; };
struct mesh_sample { int gid; float c0, c1, c2, depth; bool hit; };

// The resolve of one pixel, one code path for both entry points: the z-buffer's winner at pixel (x, y) -> global face id, shaded colour and depth.
__device__ __forceinline__ mesh_sample mesh_resolve(unsigned long long key, int x, int y, const float* __restrict__ scr, const float* __restrict__ nrm,
                                                    const int32_t* __restrict__ faces, int V, int F, const mesh_shade& m) {
    mesh_sample o{-1, 0.f, 0.f, 0.f, 0.f, false};
    if (key == ~0ull) return o;
    o.gid = (int)(key & 0xffffffffu);
    const int p = o.gid / F, f = o.gid - p * F;
    const float* s = scr + (size_t)p * V * 3;
    const float* n = nrm + (size_t)p * V * 3;
    const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    mesh_tri t;
#pragma unroll
    for (int k = 0; k < 3; ++k) { t.v[k] = s[(size_t)i0 * 3 + k]; t.v[3 + k] = s[(size_t)i1 * 3 + k]; t.v[6 + k] = s[(size_t)i2 * 3 + k]; }
    mesh_setup(t);
    float b0, b1, b2;
    o.hit = mesh_bary(t, x + 0.5f, y + 0.5f, b0, b1, b2, o.depth);                // true: the face pass took the same path
    if (o.hit) {
        const float nx = (b0 * n[(size_t)i0 * 3] + b1 * n[(size_t)i1 * 3]) + b2 * n[(size_t)i2 * 3];
        const float ny = (b0 * n[(size_t)i0 * 3 + 1] + b1 * n[(size_t)i1 * 3 + 1]) + b2 * n[(size_t)i2 * 3 + 1];
        const float nz = (b0 * n[(size_t)i0 * 3 + 2] + b1 * n[(size_t)i1 * 3 + 2]) + b2 * n[(size_t)i2 * 3 + 2];
        const float inv = __builtin_amdgcn_rsqf(fmaxf((nx * nx + ny * ny) + nz * nz, 1e-30f));
        const float ndl = fmaxf(((nx * m.lx + ny * m.ly) + nz * m.lz) * inv, 0.f);
        const float lum = m.ambient + m.kd * ndl;
        o.c0 = __builtin_amdgcn_fmed3f(m.r * lum, 0.f, 1.f); o.c1 = __builtin_amdgcn_fmed3f(m.g * lum, 0.f, 1.f); o.c2 = __builtin_amdgcn_fmed3f(m.b * lum, 0.f, 1.f);
    } else {
        o.gid = -1; o.depth = 0.f;
    }
    return o;
}
// the pixel's bytes (o: the output pixel, fr: the background pixel or null = black) and its entries `at` of the optional planes
__device__ __forceinline__ void mesh_store(const mesh_sample& s, uint8_t* __restrict__ o, const uint8_t* __restrict__ fr, long at, float* __restrict__ color_out,
                                           int32_t* __restrict__ face_out, float* __restrict__ depth_out) {
    if (s.hit) {
        o[0] = (uint8_t)rintf(255.f * s.c0); o[1] = (uint8_t)rintf(255.f * s.c1); o[2] = (uint8_t)rintf(255.f * s.c2);
    } else if (fr) {
        o[0] = fr[0]; o[1] = fr[1]; o[2] = fr[2];
    } else {
        o[0] = 0; o[1] = 0; o[2] = 0;
    }
    if (color_out) { color_out[at * 3] = s.c0; color_out[at * 3 + 1] = s.c1; color_out[at * 3 + 2] = s.c2; }
    if (face_out) face_out[at] = s.gid;
    if (depth_out) depth_out[at] = s.depth;
}

// Launch 3: one thread per pixel of every output image.
__global__ __launch_bounds__(256) void mesh_resolve_kernel(const float* __restrict__ scr, const float* __restrict__ nrm, const int32_t* __restrict__ faces,
                                                           const unsigned long long* __restrict__ zbuf, const uint8_t* __restrict__ frame,
                                                           uint8_t* __restrict__ out, float* __restrict__ color_out, int32_t* __restrict__ face_out,
                                                           float* __restrict__ depth_out, int NI, int V, int F, int H, int W, mesh_shade m) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long plane = (long)H * W;
    if (idx >= NI * plane) return;
    const long r = idx % plane;
    const int y = (int)(r / W), x = (int)(r - (long)y * W);
    mesh_store(mesh_resolve(zbuf[idx], x, y, scr, nrm, faces, V, F, m), out + idx * 3, frame ? frame + r * 3 : nullptr, idx, color_out, face_out, depth_out);
}

// verts [P, V, 3] fp32 (mesh frame, as WHMR.forward returns them); faces [F, 3] int32 with every index in [0, V) (the caller checks); vf_ptr [V + 1],
// vf_idx [3 F] int32: vertex -> face CSR; cam_t [P, 3]; focal [P, 2] = (fx, fy); rot [9] HOST floats (camera_rotation, row-major) or null = identity;
// side_cos / side_sin of sideview_angle; frame [H, W, 3] uint8 or null (black); per_person: one image per person instead of one shared depth buffer;
// base colour, ambient, k_d, (lx, ly, lz) = unit direction TO the light in the world frame.  Scratch: scr, nrm [P, V, 3] fp32 (scr = (u, v, depth) of
// every vertex on return), zbuf [NI, H, W] uint64, NI = per_person ? P : 1.  out [NI, H, W, 3] uint8; optional (or null) color_out [NI, H, W, 3] fp32
// (0 on the background), face_out [NI, H, W] int32 (global face id person * F + face, -1 = background), depth_out [NI, H, W] fp32 (0 = background).
extern "C" int whmr_mesh_render(const float* verts, int P, int V, const int32_t* faces, int F, const int32_t* vf_ptr, const int32_t* vf_idx,
                                const float* cam_t, const float* focal, float cx, float cy, const float* rot, float side_cos, float side_sin, float znear,
                                const uint8_t* frame, int H, int W, int per_person, float base_r, float base_g, float base_b, float ambient, float k_d,
                                float lx, float ly, float lz, float* scr, float* nrm, void* zbuf, uint8_t* out, float* color_out, int32_t* face_out,
                                float* depth_out, void* stream) {
    if (P <= 0 || V <= 0 || F <= 0 || H <= 0 || W <= 0 || (long)P * F > 0x7fffffffL) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const int NI = per_person ? P : 1;
    const long npix = (long)NI * H * W;
    mesh_cam c{cx, cy, side_cos, side_sin, rot != nullptr, {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}};
    if (rot)
        for (int k = 0; k < 9; ++k) c.r[k] = rot[k];
    mesh_shade m{base_r, base_g, base_b, ambient, k_d, lx, ly, lz};
    const long n0 = (long)P * V > npix ? (long)P * V : npix;
    hipLaunchKernelGGL(mesh_vertex_kernel, dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0, st, verts, faces, vf_ptr, vf_idx, cam_t, focal, scr, nrm,
                       (unsigned long long*)zbuf, npix, P, V, c);
    WHMR_CHECK_LAUNCH();
    hipLaunchKernelGGL(mesh_faces_kernel, dim3((unsigned)(((long)P * F + 255) / 256)), dim3(256), 0, st, scr, faces, (unsigned long long*)zbuf, P, V, F, H, W,
                       per_person, znear);
    WHMR_CHECK_LAUNCH();
    hipLaunchKernelGGL(mesh_resolve_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, scr, nrm, faces, (const unsigned long long*)zbuf, frame,
                       out, color_out, face_out, depth_out, NI, V, F, H, W, m);
    WHMR_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------
// Draw-list form: any number of mesh instances ("draws") into any number of target images in the same three launches -- the overlays of a whole clip,
// its per-person images, or the frame | overlay | side view | side view strips of render_image_group.  The host packs two device tables (rows of
// fixed size, little-endian, no implicit padding: whmr_amd._lib.RENDER_IMAGE_DTYPE / RENDER_DRAW_DTYPE restate them, tests/test_mesh_render_clip_cpu.py
// holds the two sides together through the static_asserts below).  The arithmetic per vertex, per face and per pixel is the device code above.
struct whmr_render_image {
    const uint8_t* frame;                       // background, null = black; row y at frame + y * frame_row_stride
    uint8_t* out;                               // row y at out + y * out_row_stride: a whole tensor or one panel of a strip
    int64_t frame_row_stride, out_row_stride;   // bytes
    int64_t pix_off;                            // this image's first element of the packed per-pixel planes (zbuf, color_out, face_out, depth_out)
    int32_t H, W;
    float cx, cy;
};
struct whmr_render_draw {
    int32_t row;                                // row of cam_t, focal and the vertex set
    int32_t verts_set;                          // 0: verts0, 1: verts1
    int32_t image;                              // target image; draws of one image share its depth buffer
    float side_cos, side_sin;
    int32_t reserved[3];
};
static_assert(sizeof(whmr_render_image) == 56, "table layout");
static_assert(offsetof(whmr_render_image, frame) == 0, "table layout");
static_assert(offsetof(whmr_render_image, out) == 8, "table layout");
static_assert(offsetof(whmr_render_image, frame_row_stride) == 16, "table layout");
static_assert(offsetof(whmr_render_image, out_row_stride) == 24, "table layout");
static_assert(offsetof(whmr_render_image, pix_off) == 32, "table layout");
static_assert(offsetof(whmr_render_image, H) == 40, "table layout");
static_assert(offsetof(whmr_render_image, W) == 44, "table layout");
static_assert(offsetof(whmr_render_image, cx) == 48, "table layout");
static_assert(offsetof(whmr_render_image, cy) == 52, "table layout");
static_assert(sizeof(whmr_render_draw) == 32, "table layout");
static_assert(offsetof(whmr_render_draw, row) == 0, "table layout");
static_assert(offsetof(whmr_render_draw, verts_set) == 4, "table layout");
static_assert(offsetof(whmr_render_draw, image) == 8, "table layout");
static_assert(offsetof(whmr_render_draw, side_cos) == 12, "table layout");
static_assert(offsetof(whmr_render_draw, side_sin) == 16, "table layout");
static_assert(offsetof(whmr_render_draw, reserved) == 20, "table layout");

// The targets of a draw list.  The host checks the tables before it uploads them; a row that is out of range all the same is not drawn (nothing is
// read or written through it).
struct mesh_draw_targets {
    const whmr_render_draw* draws; const whmr_render_image* images;
    int R, NI, has_verts1; long total;
    __device__ __forceinline__ bool image_ok(int img) const {
        if ((unsigned)img >= (unsigned)NI) return false;
        const whmr_render_image& im = images[img];
        return im.H > 0 && im.W > 0 && im.pix_off >= 0 && im.pix_off + (long)im.H * im.W <= total;
    }
    __device__ __forceinline__ int image(int d) const {
        const whmr_render_draw& dr = draws[d];
        const bool ok = (unsigned)dr.row < (unsigned)R && (dr.verts_set == 0 || (dr.verts_set == 1 && has_verts1)) && image_ok(dr.image);
        return ok ? dr.image : -1;
    }
    __device__ __forceinline__ mesh_target target(int img) const { return mesh_target{images[img].H, images[img].W, (long)images[img].pix_off}; }
};

// One (draw, vertex) of launch 1, one code path for the draw list and the scene: the centre comes from the draw's image, the angle from the draw.
__device__ __forceinline__ void mesh_draw_vertex(const float* __restrict__ verts0, const float* __restrict__ verts1, const int32_t* __restrict__ faces,
                                                 const int32_t* __restrict__ vf_ptr, const int32_t* __restrict__ vf_idx, const float* __restrict__ cam_t,
                                                 const float* __restrict__ focal, float* __restrict__ scr, float* __restrict__ nrm, long idx, int D, int V,
                                                 const mesh_draw_targets& tg, mesh_cam c) {
    if (idx >= (long)D * V) return;
    const int d = (int)(idx / V), v = (int)(idx - (long)d * V);
    const int img = tg.image(d);
    if (img < 0) return;
    const whmr_render_draw& dr = tg.draws[d];
    c.cx = tg.images[img].cx; c.cy = tg.images[img].cy; c.sc = dr.side_cos; c.ss = dr.side_sin;
    mesh_vertex((dr.verts_set ? verts1 : verts0) + (size_t)dr.row * V * 3, v, faces, vf_ptr, vf_idx, cam_t + (size_t)dr.row * 3, focal + (size_t)dr.row * 2, c,
                scr + idx * 3, nrm + idx * 3);
}

// Launch 1: z-buffer clear of all images + one thread per (draw, vertex).
__global__ __launch_bounds__(256) void mesh_draw_vertex_kernel(const float* __restrict__ verts0, const float* __restrict__ verts1, const int32_t* __restrict__ faces,
                                                               const int32_t* __restrict__ vf_ptr, const int32_t* __restrict__ vf_idx,
                                                               const float* __restrict__ cam_t, const float* __restrict__ focal, float* __restrict__ scr,
                                                               float* __restrict__ nrm, unsigned long long* __restrict__ zbuf, int D, int V, mesh_draw_targets tg,
                                                               mesh_cam c) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < tg.total) zbuf[idx] = ~0ull;
    mesh_draw_vertex(verts0, verts1, faces, vf_ptr, vf_idx, cam_t, focal, scr, nrm, idx, D, V, tg, c);
}

// Launch 2: one lane per (draw, face).
__global__ __launch_bounds__(256) void mesh_draw_faces_kernel(const float* __restrict__ scr, const int32_t* __restrict__ faces, unsigned long long* __restrict__ zbuf,
                                                              int D, int V, int F, float znear, mesh_draw_targets tg) {
    mesh_faces(scr, faces, zbuf, (long)blockIdx.x * 256 + threadIdx.x, (long)D * F, V, F, znear, tg);
}

// Launch 3: blockIdx.y = image, the x dimension strides over its pixels (it is sized for the mean plane: one step when all images have one size).
__global__ __launch_bounds__(256) void mesh_draw_resolve_kernel(const float* __restrict__ scr, const float* __restrict__ nrm, const int32_t* __restrict__ faces,
                                                                const unsigned long long* __restrict__ zbuf, float* __restrict__ color_out,
                                                                int32_t* __restrict__ face_out, float* __restrict__ depth_out, int V, int F, mesh_draw_targets tg,
                                                                mesh_shade m) {
    if (!tg.image_ok((int)blockIdx.y)) return;
    const whmr_render_image im = tg.images[blockIdx.y];
    const long plane = (long)im.H * im.W;
    for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < plane; r += (long)gridDim.x * 256) {
        const int y = (int)(r / im.W), x = (int)(r - (long)y * im.W);
        const long at = im.pix_off + r;
        mesh_store(mesh_resolve(zbuf[at], x, y, scr, nrm, faces, V, F, m), im.out + y * im.out_row_stride + (long)x * 3,
                   im.frame ? im.frame + y * im.frame_row_stride + (long)x * 3 : nullptr, at, color_out, face_out, depth_out);
    }
}

// verts0, verts1 (nullable) [R, V, 3]; cam_t [R, 3]; focal [R, 2]; faces, vf_ptr, vf_idx, rot, znear and the shading constants as whmr_mesh_render;
// draws: DEVICE table of D whmr_render_draw, images: DEVICE table of NI whmr_render_image, total_pixels = the sum of H * W over the images.  Scratch:
// scr, nrm [D, V, 3] fp32, zbuf [total_pixels] uint64.  Optional packed planes (or null): color_out [total_pixels, 3], face_out [total_pixels] (global
// face id draw * F + face, -1 = background), depth_out [total_pixels].  The nearest face wins a pixel, ties go to the smaller id = the earlier draw.
extern "C" int whmr_mesh_render_draws(const float* verts0, const float* verts1, int R, int V, const int32_t* faces, int F, const int32_t* vf_ptr,
                                      const int32_t* vf_idx, const float* cam_t, const float* focal, const void* draws, int D, const void* images, int NI,
                                      long total_pixels, const float* rot, float znear, float base_r, float base_g, float base_b, float ambient, float k_d,
                                      float lx, float ly, float lz, float* scr, float* nrm, void* zbuf, float* color_out, int32_t* face_out, float* depth_out,
                                      void* stream) {
    if (R <= 0 || V <= 0 || F <= 0 || D < 0 || NI <= 0 || NI > 65535 || total_pixels <= 0 || (long)D * F > 0x7fffffffL) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    mesh_cam c{0.f, 0.f, 1.f, 0.f, rot != nullptr, {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}};
    if (rot)
        for (int k = 0; k < 9; ++k) c.r[k] = rot[k];
    mesh_shade m{base_r, base_g, base_b, ambient, k_d, lx, ly, lz};
    mesh_draw_targets tg{(const whmr_render_draw*)draws, (const whmr_render_image*)images, R, NI, verts1 != nullptr, total_pixels};
    const long n0 = (long)D * V > total_pixels ? (long)D * V : total_pixels;
    hipLaunchKernelGGL(mesh_draw_vertex_kernel, dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0, st, verts0, verts1, faces, vf_ptr, vf_idx, cam_t, focal, scr, nrm,
                       (unsigned long long*)zbuf, D, V, tg, c);
    WHMR_CHECK_LAUNCH();
    if (D > 0) {
        hipLaunchKernelGGL(mesh_draw_faces_kernel, dim3((unsigned)(((long)D * F + 255) / 256)), dim3(256), 0, st, scr, faces, (unsigned long long*)zbuf, D, V, F,
                           znear, tg);
        WHMR_CHECK_LAUNCH();
    }
    const long mean_plane = (total_pixels + NI - 1) / NI;
    hipLaunchKernelGGL(mesh_draw_resolve_kernel, dim3((unsigned)((mean_plane + 255) / 256), (unsigned)NI), dim3(256), 0, st, scr, nrm, faces,
                       (const unsigned long long*)zbuf, color_out, face_out, depth_out, V, F, tg, m);
    WHMR_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------
// Scene form: the draw list plus at most one checkerboard ground plane per image (see the header).  A third device table has one row per image
// (whmr_amd._lib.RENDER_GROUND_DTYPE restates it, tests/test_mesh_ground_cpu.py holds the two sides together through the static_asserts below).
struct whmr_ground_row {
    int32_t draw;                               // the draw that owns the plane: its row is the camera, its mesh gives the height; -1 = no plane
    int32_t given;                              // 0: y = the lowest world-frame point of the owning draw's mesh, found on the device; 1: y below
    float y;                                    // the plane's height in the world frame (y up), read when given
    float half;                                 // half the side of the square, > 0
    int32_t n;                                  // tiles per side, >= 1
    float dark, light;                          // grey of the tiles with ix + iz even / odd, 0..1
    int32_t reserved;
};
static_assert(sizeof(whmr_ground_row) == 32, "table layout");
static_assert(offsetof(whmr_ground_row, draw) == 0, "table layout");
static_assert(offsetof(whmr_ground_row, given) == 4, "table layout");
static_assert(offsetof(whmr_ground_row, y) == 8, "table layout");
static_assert(offsetof(whmr_ground_row, half) == 12, "table layout");
static_assert(offsetof(whmr_ground_row, n) == 16, "table layout");
static_assert(offsetof(whmr_ground_row, dark) == 20, "table layout");
static_assert(offsetof(whmr_ground_row, light) == 24, "table layout");
static_assert(offsetof(whmr_ground_row, reserved) == 28, "table layout");

// max_v p_y of a draw as an integer maximum: the key grows with the float (negative floats with their magnitude bits flipped), so an atomic max
// of keys is the exact maximum whatever order the lanes arrive in.  MESH_NO_HEIGHT is below every key of a number and decodes to a NaN.
#define MESH_NO_HEIGHT ((int32_t)0x80000000)
__device__ __forceinline__ int32_t mesh_height_key(float f) { const int32_t i = __float_as_int(f); return i >= 0 ? i : i ^ 0x7fffffff; }
__device__ __forceinline__ float mesh_height_of(int32_t k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }

struct mesh_scene {
    const whmr_ground_row* grounds;             // [NI]
    int32_t* heights;                           // [D] scratch: key of max_v p_y of every draw whose plane asks for it
    int32_t* ground_out;                        // [total_pixels] or null
    float* ground_y;                            // [NI]
    int D;
    // the plane of image img: its owning draw, or -1 (no plane, or a row the host would have refused: nothing is read through it)
    __device__ __forceinline__ int owner(int img, const mesh_draw_targets& tg) const {
        const whmr_ground_row& g = grounds[img];
        const bool ok = (unsigned)g.draw < (unsigned)D && g.n >= 1 && g.half > 0.f && tg.image(g.draw) == img;
        return ok ? g.draw : -1;
    }
};

// Launch 1 of the scene: as the draw list's, and the height slots are cleared beside the z-buffer.
__global__ __launch_bounds__(256) void mesh_scene_vertex_kernel(const float* __restrict__ verts0, const float* __restrict__ verts1, const int32_t* __restrict__ faces,
                                                                const int32_t* __restrict__ vf_ptr, const int32_t* __restrict__ vf_idx,
                                                                const float* __restrict__ cam_t, const float* __restrict__ focal, float* __restrict__ scr,
                                                                float* __restrict__ nrm, unsigned long long* __restrict__ zbuf, int D, int V, mesh_draw_targets tg,
                                                                mesh_cam c, int32_t* __restrict__ heights) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < tg.total) zbuf[idx] = ~0ull;
    if (idx < D) heights[idx] = MESH_NO_HEIGHT;
    mesh_draw_vertex(verts0, verts1, faces, vf_ptr, vf_idx, cam_t, focal, scr, nrm, idx, D, V, tg, c);
}

// Launch 2 of the scene: lane idx < D * V also looks at vertex idx: if its draw owns a plane without a given height, p_y enters the draw's maximum --
// reduced over the wave first (the lanes of a wave nearly always share the draw), one atomic per wave and draw.  Every lane of the wave comes here.
__device__ __forceinline__ void mesh_heights(const float* __restrict__ verts0, const float* __restrict__ verts1, long idx, int V, const mesh_draw_targets& tg,
                                             const mesh_scene& sc) {
    int d = -1;
    int32_t key = MESH_NO_HEIGHT;
    if (idx < (long)sc.D * V) {
        const int dd = (int)(idx / V), v = (int)(idx - (long)dd * V);
        const int img = tg.image(dd);
        if (img >= 0 && !sc.grounds[img].given && sc.owner(img, tg) == dd) {
            d = dd;
            const whmr_render_draw& dr = tg.draws[dd];
            const float py = ((dr.verts_set ? verts1 : verts0) + (size_t)dr.row * V * 3)[(size_t)v * 3 + 1];
            if (py == py) key = mesh_height_key(py);                              // a NaN vertex is skipped
        }
    }
    const unsigned long long any = __ballot(d >= 0);
    if (!any) return;                                                             // wave-uniform: no lane of this wave feeds a plane
    const int d0 = __shfl(d, __ffsll((long long)any) - 1, 64);
    int32_t k = d == d0 ? key : MESH_NO_HEIGHT;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int32_t other = __shfl_xor(k, off, 64);
        k = other > k ? other : k;
    }
    if ((threadIdx.x & 63) == 0 && k != MESH_NO_HEIGHT) atomicMax(sc.heights + d0, k);
    if (d >= 0 && d != d0 && key != MESH_NO_HEIGHT) atomicMax(sc.heights + d, key);   // the few lanes of a wave that straddles two draws
}
__global__ __launch_bounds__(256) void mesh_scene_faces_kernel(const float* __restrict__ verts0, const float* __restrict__ verts1, const float* __restrict__ scr,
                                                               const int32_t* __restrict__ faces, unsigned long long* __restrict__ zbuf, int V, int F, float znear,
                                                               mesh_draw_targets tg, mesh_scene sc) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    mesh_heights(verts0, verts1, idx, V, tg, sc);
    mesh_faces(scr, faces, zbuf, idx, (long)sc.D * F, V, F, znear, tg);
}

// The plane of one image as the resolve pass needs it (see the header): q = Z w + o with w = R D (a, b, 1), o = -R D t.
struct mesh_plane { bool on; float h, half, tile, n, dark, light, fx, fy, ox, oy, oz; };
__device__ __forceinline__ mesh_plane mesh_plane_setup(int img, const mesh_draw_targets& tg, const mesh_scene& sc, const float* __restrict__ cam_t,
                                                       const float* __restrict__ focal, const mesh_cam& c) {
    mesh_plane p{};
    const int d = sc.owner(img, tg);
    if (d < 0) return p;
    const whmr_ground_row g = sc.grounds[img];
    p.h = g.given ? g.y : -mesh_height_of(sc.heights[d]);
    if (!(p.h == p.h)) return p;                                                  // no finite vertex (or a NaN given): no plane
    const int row = tg.draws[d].row;
    const float tx = -cam_t[(size_t)row * 3], ty = cam_t[(size_t)row * 3 + 1], tz = cam_t[(size_t)row * 3 + 2];      // -D t
    p.ox = tx; p.oy = ty; p.oz = tz;
    if (c.has_rot) {
        p.ox = (c.r[0] * tx + c.r[1] * ty) + c.r[2] * tz;
        p.oy = (c.r[3] * tx + c.r[4] * ty) + c.r[5] * tz;
        p.oz = (c.r[6] * tx + c.r[7] * ty) + c.r[8] * tz;
    }
    p.fx = focal[(size_t)row * 2]; p.fy = focal[(size_t)row * 2 + 1];
    p.half = g.half; p.n = (float)g.n; p.tile = 2.f * g.half / (float)g.n; p.dark = g.dark; p.light = g.light;
    p.on = true;
    return p;
}
// pixel (x, y) against the plane: true = the plane covers it, at depth Z in tile (ix, iz)
__device__ __forceinline__ bool mesh_plane_hit(const mesh_plane& p, const mesh_cam& c, float cx, float cy, int x, int y, float znear, float& Z, int& ix, int& iz) {
    const float a = ((float)x + 0.5f - cx) / p.fx, b = -(((float)y + 0.5f - cy) / p.fy);
    float wx = a, wy = b, wz = -1.f;
    if (c.has_rot) {
        wx = (c.r[0] * a + c.r[1] * b) - c.r[2];
        wy = (c.r[3] * a + c.r[4] * b) - c.r[5];
        wz = (c.r[6] * a + c.r[7] * b) - c.r[8];
    }
    Z = (p.h - p.oy) / wy;
    const float fi = floorf((__fmaf_rn(Z, wx, p.ox) + p.half) / p.tile), fk = floorf((__fmaf_rn(Z, wz, p.oz) + p.half) / p.tile);
    const bool hit = fabsf(Z) < __builtin_inff() && Z > znear && fi >= 0.f && fi < p.n && fk >= 0.f && fk < p.n;     // every comparison is false for a NaN
    ix = hit ? (int)fi : 0; iz = hit ? (int)fk : 0;
    return hit;
}

// Launch 3 of the scene: the draw list's resolve; an image with a plane (one block-uniform branch) also intersects the pixel's ray with it.
__global__ __launch_bounds__(256) void mesh_scene_resolve_kernel(const float* __restrict__ scr, const float* __restrict__ nrm, const int32_t* __restrict__ faces,
                                                                 const unsigned long long* __restrict__ zbuf, float* __restrict__ color_out,
                                                                 int32_t* __restrict__ face_out, float* __restrict__ depth_out, const float* __restrict__ cam_t,
                                                                 const float* __restrict__ focal, int V, int F, float znear, mesh_draw_targets tg, mesh_shade m,
                                                                 mesh_cam c, mesh_scene sc) {
    const int img = (int)blockIdx.y;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (!tg.image_ok(img)) {
        if (first) sc.ground_y[img] = __builtin_nanf("");
        return;
    }
    const whmr_render_image im = tg.images[img];
    const mesh_plane pl = mesh_plane_setup(img, tg, sc, cam_t, focal, c);
    if (first) sc.ground_y[img] = pl.on ? pl.h : __builtin_nanf("");
    const long plane = (long)im.H * im.W;
    for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < plane; r += (long)gridDim.x * 256) {
        const int y = (int)(r / im.W), x = (int)(r - (long)y * im.W);
        const long at = im.pix_off + r;
        mesh_sample s = mesh_resolve(zbuf[at], x, y, scr, nrm, faces, V, F, m);
        int tile = -1;
        if (pl.on) {
            float Z;
            int ix, iz;
            if (mesh_plane_hit(pl, c, im.cx, im.cy, x, y, znear, Z, ix, iz) && (!s.hit || Z < s.depth)) {
                const float grey = ((ix + iz) & 1) ? pl.light : pl.dark;
                s = mesh_sample{-1, grey, grey, grey, Z, true};
                tile = ix * (int)pl.n + iz;
            }
        }
        mesh_store(s, im.out + y * im.out_row_stride + (long)x * 3, im.frame ? im.frame + y * im.frame_row_stride + (long)x * 3 : nullptr, at, color_out,
                   face_out, depth_out);
        if (sc.ground_out) sc.ground_out[at] = tile;
    }
}

// The arguments of whmr_mesh_render_draws, and: grounds: DEVICE table of NI whmr_ground_row; heights [max(D, 1)] int32 scratch; ground_out
// [total_pixels] int32 (ix * n + iz of the plane's tile, -1 elsewhere) or null; ground_y [NI] fp32: the height of every image's plane, NaN = none.
// A table without a plane gives the bytes of whmr_mesh_render_draws.  Three launches, no allocation, no synchronisation; bit-reproducible.
extern "C" int whmr_mesh_render_scene(const float* verts0, const float* verts1, int R, int V, const int32_t* faces, int F, const int32_t* vf_ptr,
                                      const int32_t* vf_idx, const float* cam_t, const float* focal, const void* draws, int D, const void* images, int NI,
                                      long total_pixels, const void* grounds, const float* rot, float znear, float base_r, float base_g, float base_b,
                                      float ambient, float k_d, float lx, float ly, float lz, float* scr, float* nrm, void* zbuf, int32_t* heights,
                                      float* color_out, int32_t* face_out, float* depth_out, int32_t* ground_out, float* ground_y, void* stream) {
    if (R <= 0 || V <= 0 || F <= 0 || D < 0 || NI <= 0 || NI > 65535 || total_pixels <= 0 || (long)D * F > 0x7fffffffL || !grounds || !heights || !ground_y)
        return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    mesh_cam c{0.f, 0.f, 1.f, 0.f, rot != nullptr, {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}};
    if (rot)
        for (int k = 0; k < 9; ++k) c.r[k] = rot[k];
    mesh_shade m{base_r, base_g, base_b, ambient, k_d, lx, ly, lz};
    mesh_draw_targets tg{(const whmr_render_draw*)draws, (const whmr_render_image*)images, R, NI, verts1 != nullptr, total_pixels};
    mesh_scene sc{(const whmr_ground_row*)grounds, heights, ground_out, ground_y, D};
    const long n0 = (long)D * V > total_pixels ? (long)D * V : total_pixels;                // >= D: the height slots are cleared by the same grid
    hipLaunchKernelGGL(mesh_scene_vertex_kernel, dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0, st, verts0, verts1, faces, vf_ptr, vf_idx, cam_t, focal, scr,
                       nrm, (unsigned long long*)zbuf, D, V, tg, c, heights);
    WHMR_CHECK_LAUNCH();
    if (D > 0) {
        const long n1 = (long)D * (F > V ? F : V);
        hipLaunchKernelGGL(mesh_scene_faces_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, st, verts0, verts1, scr, faces, (unsigned long long*)zbuf,
                           V, F, znear, tg, sc);
        WHMR_CHECK_LAUNCH();
    }
    const long mean_plane = (total_pixels + NI - 1) / NI;
    hipLaunchKernelGGL(mesh_scene_resolve_kernel, dim3((unsigned)((mean_plane + 255) / 256), (unsigned)NI), dim3(256), 0, st, scr, nrm, faces,
                       (const unsigned long long*)zbuf, color_out, face_out, depth_out, cam_t, focal, V, F, znear, tg, m, c, sc);
    WHMR_CHECK_LAUNCH();
    return 0;
}

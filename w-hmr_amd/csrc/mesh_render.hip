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

// The camera of launch 1, one code path for vertices and skeleton joints: the point p (mesh frame) under camera c with translation t and focal
// lengths fo -> its screen position (u, v, depth).
__device__ __forceinline__ void mesh_camera(const float* __restrict__ p, const float* __restrict__ t, const float* __restrict__ fo, const mesh_cam& c,
                                            float* __restrict__ scr) {
    // world: q = S D p,  S = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    const float x = p[0], y = -p[1], z = -p[2];
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
}

// The vertex transform of launch 1, one code path for both entry points: vertex v of the mesh at vp (mesh frame) under camera c with translation t and
// focal lengths fo -> its screen position (u, v, depth) and its world-frame smooth normal.
__device__ __forceinline__ void mesh_vertex(const float* __restrict__ vp, int v, const int32_t* __restrict__ faces, const int32_t* __restrict__ vf_ptr,
                                            const int32_t* __restrict__ vf_idx, const float* __restrict__ t, const float* __restrict__ fo, const mesh_cam& c,
                                            float* __restrict__ scr, float* __restrict__ nrm) {
    mesh_camera(vp + v * 3, t, fo, c, scr);
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

// ---------------------------------------------------------------------------------------------------------------------------------------------------
// Marked form: the scene plus keypoint skeletons (--draw_keypoints, demo/whmr_demo.py:158; the keypoints_2d of render_image_group,
// utils/renderer_cam.py:157,165-166) and hidden-line wireframe (--wireframe, :152).  The reference draws the skeleton with PARE's draw_skeleton on cv2
// lines and circles; neither is in the reference tree, so the drawing is DEFINED here and pixel parity with cv2 is unpinned.  Pixel (j, i) has the
// centre c = (i + 0.5, j + 0.5).
//   Keypoints of a skeleton row: source 0 sends the row's 3-D joints (mesh frame) through mesh_camera with the row's cam_t / focal, the target image's
//   centre, the call's rot and the row's side rotation: (u, v, Z), valid with w = Z if u, v, Z are finite and Z > znear, else w = 0.  Source 1 takes the
//   row's 2-D keypoints (x, y, conf): w = conf, or 0 if one of the three is not finite.  (u, v, w) of every row goes to kp [S, J, 3].
//   Coverage: a bone (n0, n1) is drawn iff both w > 0 and covers c by a = clamp(half_width + 0.5 - d, 0, 1), d the distance from c to the segment (the
//   foot parameter clamped to [0, 1]; a bone of no length is a point).  A joint with w > 0 covers by a = clamp(radius + 0.5 - |c - k|, 0, 1).  A bone
//   naming a joint outside [0, J) is not drawn.
//   A layer at a pixel: from a colour C, the skeletons of this image and this layer in table order, in each the bones in table order and then the
//   joints in index order; each with a > 0 blends C <- C + a (rgb - C).
//   The pixel: C0 = frame / 255 (0 without a frame); C1 = the under layer over C0; the scene's sample (z-buffer winner or plane) as today, with alpha 1
//   for a solid draw and the plane and, for a wireframe draw, alpha = clamp(half_width + 0.5 - d_e, 0, 1), d_e = the smallest of |edge function at c| /
//   the edge's screen length over the winner's three edges -- the winner is still the nearest face, so hidden lines stay hidden; an inner edge is
//   drawn by both its faces (2 half_width wide), a silhouette edge by one.  C2 = the shaded colour exactly where alpha = 1, C1 where alpha = 0 or
//   nothing won, else C1 + alpha (shade - C1); C3 = the over layer over C2.  Bytes: the frame's where nothing touched the pixel, today's where alpha = 1
//   and no over mark touched it, rint(255 C3) elsewhere.  color / face / depth / ground keep the winner's sample whatever its alpha.
// The resolve does not test every pixel against every bone: a workgroup lists the skeletons of its own image once (wave 0, ballots, table order),
// and for each span of 256 pixels marks in LDS bit masks -- one bit per (listed skeleton, bone or joint), one mask per layer -- the ones whose box,
// padded by half-width or radius + 0.5, meets the span's box.  A pixel walks the set bits in order.  The list holds MESH_BIN_SKELETONS skeletons (and
// no more than fit MESH_BIN_WORDS mask words); the skeletons of the image beyond it come later in table order and are tested pixel by pixel after it.
struct whmr_style_row {
    int32_t mode;                               // 0 solid, 1 wireframe
    float half_width;                           // of a wireframe line, pixels
    int32_t reserved[2];
};
struct whmr_skeleton_row {
    int32_t row;                                // row of joints / keypoints, cam_t and focal
    int32_t image;                              // target image
    int32_t source;                             // 0: project the 3-D joints of the row, 1: the 2-D keypoints of the row
    int32_t layer;                              // 0 under the meshes, 1 over everything
    float side_cos, side_sin;                   // of the side rotation (source 0)
    float half_width, radius;                   // of a bone / a joint dot, pixels
};
static_assert(sizeof(whmr_style_row) == 16, "table layout");
static_assert(offsetof(whmr_style_row, mode) == 0, "table layout");
static_assert(offsetof(whmr_style_row, half_width) == 4, "table layout");
static_assert(offsetof(whmr_style_row, reserved) == 8, "table layout");
static_assert(sizeof(whmr_skeleton_row) == 32, "table layout");
static_assert(offsetof(whmr_skeleton_row, row) == 0, "table layout");
static_assert(offsetof(whmr_skeleton_row, image) == 4, "table layout");
static_assert(offsetof(whmr_skeleton_row, source) == 8, "table layout");
static_assert(offsetof(whmr_skeleton_row, layer) == 12, "table layout");
static_assert(offsetof(whmr_skeleton_row, side_cos) == 16, "table layout");
static_assert(offsetof(whmr_skeleton_row, side_sin) == 20, "table layout");
static_assert(offsetof(whmr_skeleton_row, half_width) == 24, "table layout");
static_assert(offsetof(whmr_skeleton_row, radius) == 28, "table layout");

#define MESH_BIN_SKELETONS 16                   // include/whmr_hip.h: WHMR_MESH_BIN_SKELETONS, whmr_amd._lib.MESH_BIN_SKELETONS
#define MESH_BIN_WORDS 32                       // 2048 (skeleton, bone or joint) bits per layer

struct mesh_marks {
    const whmr_style_row* styles;            // [D]
    const whmr_skeleton_row* skels;          // [S]
    const int32_t* bones;                       // [NB, 2]
    const float *bone_rgb, *joint_rgb;          // [NB, 3], [J, 3]
    const float *joints, *keypoints;            // [R, J, 3] each, or null
    float* kp;                                  // [S, J, 3]: (u, v, w)
    float* overlay;                             // [total_pixels, 3] or null
    int S, NB, J, R;
    // the image of skeleton s, or -1 (a row the host would have refused: nothing is read through it, nothing of it is drawn)
    __device__ __forceinline__ int image(int s, const mesh_draw_targets& tg) const {
        const whmr_skeleton_row& k = skels[s];
        const bool ok = (unsigned)k.row < (unsigned)R && (unsigned)k.layer < 2u && ((k.source == 0 && joints) || (k.source == 1 && keypoints)) &&
                        tg.image_ok(k.image);
        return ok ? k.image : -1;
    }
};

// The scene's sample of one pixel as mesh_scene_resolve_kernel takes it (that kernel keeps its own text, and with it its code object, as it was): the
// z-buffer's winner, or the plane where it is nearer (tile >= 0).
__device__ __forceinline__ mesh_sample mesh_scene_sample(unsigned long long key, int x, int y, const float* __restrict__ scr, const float* __restrict__ nrm,
                                                         const int32_t* __restrict__ faces, int V, int F, const mesh_shade& m, const mesh_plane& pl,
                                                         const mesh_cam& c, float cx, float cy, float znear, int& tile) {
    mesh_sample s = mesh_resolve(key, x, y, scr, nrm, faces, V, F, m);
    tile = -1;
    if (pl.on) {
        float Z;
        int ix, iz;
        if (mesh_plane_hit(pl, c, cx, cy, x, y, znear, Z, ix, iz) && (!s.hit || Z < s.depth)) {
            const float grey = ((ix + iz) & 1) ? pl.light : pl.dark;
            s = mesh_sample{-1, grey, grey, grey, Z, true};
            tile = ix * (int)pl.n + iz;
        }
    }
    return s;
}

__device__ __forceinline__ bool mesh_finite(float f) { return fabsf(f) < __builtin_inff(); }                      // false for a NaN

// Launch 1 of the marked form: as the scene's, and thread idx < S * J writes (u, v, w) of joint idx % J of skeleton row idx / J.
__global__ __launch_bounds__(256) void mesh_marked_vertex_kernel(const float* __restrict__ verts0, const float* __restrict__ verts1, const int32_t* __restrict__ faces,
                                                                 const int32_t* __restrict__ vf_ptr, const int32_t* __restrict__ vf_idx,
                                                                 const float* __restrict__ cam_t, const float* __restrict__ focal, float* __restrict__ scr,
                                                                 float* __restrict__ nrm, unsigned long long* __restrict__ zbuf, int D, int V, mesh_draw_targets tg,
                                                                 mesh_cam c, int32_t* __restrict__ heights, mesh_marks mk, float znear) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < tg.total) zbuf[idx] = ~0ull;
    if (idx < D) heights[idx] = MESH_NO_HEIGHT;
    if (idx < (long)mk.S * mk.J) {
        const int s = (int)(idx / mk.J), j = (int)(idx - (long)s * mk.J);
        float u = 0.f, v = 0.f, w = 0.f;
        const int img = mk.image(s, tg);
        if (img >= 0) {
            const whmr_skeleton_row k = mk.skels[s];
            if (k.source == 0) {
                mesh_cam cj = c;
                cj.cx = tg.images[img].cx; cj.cy = tg.images[img].cy; cj.sc = k.side_cos; cj.ss = k.side_sin;
                float o[3];
                mesh_camera(mk.joints + ((size_t)k.row * mk.J + j) * 3, cam_t + (size_t)k.row * 3, focal + (size_t)k.row * 2, cj, o);
                u = o[0]; v = o[1];
                w = (mesh_finite(u) && mesh_finite(v) && mesh_finite(o[2]) && o[2] > znear) ? o[2] : 0.f;
            } else {
                const float* q = mk.keypoints + ((size_t)k.row * mk.J + j) * 3;
                u = q[0]; v = q[1];
                w = (mesh_finite(u) && mesh_finite(v) && mesh_finite(q[2])) ? q[2] : 0.f;
            }
        }
        mk.kp[idx * 3] = u; mk.kp[idx * 3 + 1] = v; mk.kp[idx * 3 + 2] = w;
    }
    mesh_draw_vertex(verts0, verts1, faces, vf_ptr, vf_idx, cam_t, focal, scr, nrm, idx, D, V, tg, c);
}

// coverage of the centre (px, py) by the segment a -> b of reach = half-width + 0.5 (a == b: a dot)
__device__ __forceinline__ float mesh_cover(float px, float py, float ax, float ay, float bx, float by, float reach) {
    const float dx = bx - ax, dy = by - ay, len2 = dx * dx + dy * dy;
    float t = 0.f;
    if (len2 > 0.f) t = fminf(fmaxf(((px - ax) * dx + (py - ay) * dy) / len2, 0.f), 1.f);
    const float ex = px - (ax + t * dx), ey = py - (ay + t * dy);
    return fminf(fmaxf(reach - sqrtf(ex * ex + ey * ey), 0.f), 1.f);              // fmaxf drops a NaN: not covered
}

// Element e of skeleton row s (e < NB: bone e, else joint e - NB): false = not drawn; else its end points, reach and colour.
struct mesh_mark_geom { float ax, ay, bx, by, reach; const float* rgb; };
__device__ __forceinline__ bool mesh_mark_of(const mesh_marks& mk, int s, int e, mesh_mark_geom& g) {
    const whmr_skeleton_row& sk = mk.skels[s];
    const float* k = mk.kp + (size_t)s * mk.J * 3;
    if (e < mk.NB) {
        const int n0 = mk.bones[2 * e], n1 = mk.bones[2 * e + 1];
        if ((unsigned)n0 >= (unsigned)mk.J || (unsigned)n1 >= (unsigned)mk.J) return false;
        const float *k0 = k + n0 * 3, *k1 = k + n1 * 3;
        if (!(k0[2] > 0.f && k1[2] > 0.f)) return false;
        g = mesh_mark_geom{k0[0], k0[1], k1[0], k1[1], sk.half_width + 0.5f, mk.bone_rgb + 3 * e};
        return true;
    }
    const int j = e - mk.NB;
    const float* k0 = k + j * 3;
    if (!(k0[2] > 0.f)) return false;
    g = mesh_mark_geom{k0[0], k0[1], k0[0], k0[1], sk.radius + 0.5f, mk.joint_rgb + 3 * j};
    return true;
}
// one mark over the colour (c0, c1, c2) at the centre (px, py)
__device__ __forceinline__ void mesh_mark(const mesh_marks& mk, int s, int e, float px, float py, float& c0, float& c1, float& c2, bool& touched) {
    mesh_mark_geom g;
    if (!mesh_mark_of(mk, s, e, g)) return;
    const float a = mesh_cover(px, py, g.ax, g.ay, g.bx, g.by, g.reach);
    if (a > 0.f) {
        c0 = __fmaf_rn(a, g.rgb[0] - c0, c0); c1 = __fmaf_rn(a, g.rgb[1] - c1, c1); c2 = __fmaf_rn(a, g.rgb[2] - c2, c2);
        touched = true;
    }
}
// can the mark reach a centre inside the box [x0, x1] x [y0, y1]?  Its own box, padded by the reach and a little more than rounding can lose:
// a superset of the covered centres is all the binning needs, the pixel decides.
__device__ __forceinline__ bool mesh_mark_meets(const mesh_marks& mk, int s, int e, float x0, float y0, float x1, float y1) {
    mesh_mark_geom g;
    if (!mesh_mark_of(mk, s, e, g)) return false;
    const float pad = g.reach + 0.0625f;
    return fminf(g.ax, g.bx) - pad <= x1 && fmaxf(g.ax, g.bx) + pad >= x0 && fminf(g.ay, g.by) - pad <= y1 && fmaxf(g.ay, g.by) + pad >= y0;
}

// one layer at one pixel: the binned marks in bit order (= table order), then the skeletons that did not fit the list, element by element
__device__ __forceinline__ void mesh_layer(const mesh_marks& mk, const mesh_draw_targets& tg, int img, int layer, const unsigned long long* words, int nwords,
                                           const int* list, int E, int s_over, float px, float py, float& c0, float& c1, float& c2, bool& touched) {
    for (int w = 0; w < nwords; ++w) {
        const unsigned long long word = words[w];
        // the same word in every lane: the walk is wave-uniform
        unsigned long long m = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(word >> 32)) << 32) |
                               (unsigned)__builtin_amdgcn_readfirstlane((int)(word & 0xffffffffu));
        while (m) {
            const int i = w * 64 + __ffsll((long long)m) - 1;
            m &= m - 1;
            const int k = i / E;
            mesh_mark(mk, __builtin_amdgcn_readfirstlane(list[k]), i - k * E, px, py, c0, c1, c2, touched);
        }
    }
    for (int s = s_over; s < mk.S; ++s) {
        if (mk.image(s, tg) != img || mk.skels[s].layer != layer) continue;
        for (int e = 0; e < E; ++e) mesh_mark(mk, s, e, px, py, c0, c1, c2, touched);
    }
}

// alpha of a wireframe draw's winning face gid at pixel (x, y)
__device__ __forceinline__ float mesh_wire_alpha(int gid, int x, int y, const float* __restrict__ scr, const int32_t* __restrict__ faces, int V, int F,
                                                 float half_width) {
    const int p = gid / F, f = gid - p * F;
    const float* s = scr + (size_t)p * V * 3;
    const float *a = s + (size_t)faces[f * 3] * 3, *b = s + (size_t)faces[f * 3 + 1] * 3, *d = s + (size_t)faces[f * 3 + 2] * 3;
    const float px = x + 0.5f, py = y + 0.5f;
    const float d0 = fabsf(mesh_edge(b[0], b[1], d[0], d[1], px, py)) / sqrtf((d[0] - b[0]) * (d[0] - b[0]) + (d[1] - b[1]) * (d[1] - b[1]));
    const float d1 = fabsf(mesh_edge(d[0], d[1], a[0], a[1], px, py)) / sqrtf((a[0] - d[0]) * (a[0] - d[0]) + (a[1] - d[1]) * (a[1] - d[1]));
    const float d2 = fabsf(mesh_edge(a[0], a[1], b[0], b[1], px, py)) / sqrtf((b[0] - a[0]) * (b[0] - a[0]) + (b[1] - a[1]) * (b[1] - a[1]));
    return fminf(fmaxf(half_width + 0.5f - fminf(d0, fminf(d1, d2)), 0.f), 1.f);                // fminf skips the 0 / 0 of an edge without length
}

__device__ __forceinline__ uint8_t mesh_byte(float c) { return (uint8_t)rintf(255.f * __builtin_amdgcn_fmed3f(c, 0.f, 1.f)); }

// Launch 3 of the marked form: the scene's resolve with the two mark layers and the wire alpha (see the header of this section).
__global__ __launch_bounds__(256) void mesh_marked_resolve_kernel(const float* __restrict__ scr, const float* __restrict__ nrm, const int32_t* __restrict__ faces,
                                                                  const unsigned long long* __restrict__ zbuf, float* __restrict__ color_out,
                                                                  int32_t* __restrict__ face_out, float* __restrict__ depth_out, const float* __restrict__ cam_t,
                                                                  const float* __restrict__ focal, int V, int F, float znear, mesh_draw_targets tg, mesh_shade m,
                                                                  mesh_cam c, mesh_scene sc, mesh_marks mk) {
    __shared__ unsigned long long s_words[2][MESH_BIN_WORDS];
    __shared__ int s_list[MESH_BIN_SKELETONS];
    __shared__ int s_n, s_over;
    const int img = (int)blockIdx.y, tid = (int)threadIdx.x, lane = tid & 63;
    const bool first = blockIdx.x == 0 && tid == 0;
    if (!tg.image_ok(img)) {                                                      // block-uniform
        if (first) sc.ground_y[img] = __builtin_nanf("");
        return;
    }
    const whmr_render_image im = tg.images[img];
    const mesh_plane pl = mesh_plane_setup(img, tg, sc, cam_t, focal, c);
    if (first) sc.ground_y[img] = pl.on ? pl.h : __builtin_nanf("");
    const long plane = (long)im.H * im.W;
    // the skeletons of this image, in table order: the first `fit` into the list, the first one beyond it into s_over
    const int E = mk.NB + mk.J;
    int n_bin = 0, over = mk.S;
    if (mk.S > 0) {                                                               // kernel-uniform
        const int room = MESH_BIN_WORDS * 64 / E, fit = room < MESH_BIN_SKELETONS ? room : MESH_BIN_SKELETONS;
        if (tid < 64) {
            int count = 0;
            if (lane == 0) s_over = mk.S;
            for (int s0 = 0; s0 < mk.S; s0 += 64) {
                const int s = s0 + lane;
                const bool mine = s < mk.S && mk.image(s, tg) == img;
                const unsigned long long b = __ballot(mine);
                const int pos = count + __popcll(b & ((1ull << lane) - 1ull));
                if (mine && pos < fit) s_list[pos] = s;
                if (mine && pos == fit) s_over = s;
                count += __popcll(b);
            }
            if (lane == 0) s_n = count < fit ? count : fit;
        }
        __syncthreads();
        n_bin = s_n; over = s_over;
    }
    const bool marks = n_bin > 0 || over < mk.S;                                   // block-uniform
    const int n_items = n_bin * E, nwords = (n_items + 63) >> 6;                  // <= MESH_BIN_WORDS
    for (long r0 = (long)blockIdx.x * 256; r0 < plane; r0 += (long)gridDim.x * 256) {          // block-uniform bounds: every thread meets the barriers
        if (nwords > 0) {
            __syncthreads();                                                      // the previous span has been read
            const long r1 = r0 + 255 < plane ? r0 + 255 : plane - 1;
            const int ya = (int)(r0 / im.W), yb = (int)(r1 / im.W);
            const float x0 = ya == yb ? (float)(r0 - (long)ya * im.W) + 0.5f : 0.5f, x1 = ya == yb ? (float)(r1 - (long)yb * im.W) + 0.5f : (float)im.W - 0.5f;
            const float y0 = (float)ya + 0.5f, y1 = (float)yb + 0.5f;
            for (int i0 = 0; i0 < nwords * 64; i0 += 256) {
                const int i = i0 + tid;
                int layer = -1;
                if (i < n_items) {
                    const int k = i / E, s = s_list[k];
                    if (mesh_mark_meets(mk, s, i - k * E, x0, y0, x1, y1)) layer = mk.skels[s].layer;
                }
                const unsigned long long under = __ballot(layer == 0), above = __ballot(layer == 1);
                if (lane == 0 && (i >> 6) < nwords) { s_words[0][i >> 6] = under; s_words[1][i >> 6] = above; }
            }
            __syncthreads();
        }
        const long r = r0 + tid;
        if (r < plane) {
            const int y = (int)(r / im.W), x = (int)(r - (long)y * im.W);
            const long at = im.pix_off + r;
            const float px = (float)x + 0.5f, py = (float)y + 0.5f;
            const uint8_t* fr = im.frame ? im.frame + y * im.frame_row_stride + (long)x * 3 : nullptr;
            uint8_t* o = im.out + y * im.out_row_stride + (long)x * 3;
            float c0 = 0.f, c1 = 0.f, c2 = 0.f;
            if (fr) { c0 = (float)fr[0] / 255.f; c1 = (float)fr[1] / 255.f; c2 = (float)fr[2] / 255.f; }
            bool under = false, above = false;
            if (marks) mesh_layer(mk, tg, img, 0, s_words[0], nwords, s_list, E, over, px, py, c0, c1, c2, under);
            int tile;
            const mesh_sample s = mesh_scene_sample(zbuf[at], x, y, scr, nrm, faces, V, F, m, pl, c, im.cx, im.cy, znear, tile);
            float alpha = s.hit ? 1.f : 0.f;
            if (s.hit && s.gid >= 0) {
                const whmr_style_row st = mk.styles[s.gid / F];
                if (st.mode == 1) alpha = mesh_wire_alpha(s.gid, x, y, scr, faces, V, F, st.half_width);
            }
            if (alpha == 1.f) {
                c0 = s.c0; c1 = s.c1; c2 = s.c2;
            } else if (alpha > 0.f) {
                c0 = __fmaf_rn(alpha, s.c0 - c0, c0); c1 = __fmaf_rn(alpha, s.c1 - c1, c1); c2 = __fmaf_rn(alpha, s.c2 - c2, c2);
            }
            if (marks) mesh_layer(mk, tg, img, 1, s_words[1], nwords, s_list, E, over, px, py, c0, c1, c2, above);
            mesh_store(s, o, fr, at, color_out, face_out, depth_out);            // today's bytes and planes
            const bool today = !above && (s.hit ? alpha == 1.f : !under);
            if (!today) {
                if (!under && !above && alpha == 0.f) {                           // a wireframe face away from its edges: nothing touched the pixel
                    o[0] = fr ? fr[0] : 0; o[1] = fr ? fr[1] : 0; o[2] = fr ? fr[2] : 0;
                } else {
                    o[0] = mesh_byte(c0); o[1] = mesh_byte(c1); o[2] = mesh_byte(c2);
                }
            }
            if (sc.ground_out) sc.ground_out[at] = tile;
            if (mk.overlay) { mk.overlay[at * 3] = c0; mk.overlay[at * 3 + 1] = c1; mk.overlay[at * 3 + 2] = c2; }
        }
    }
}

// The arguments of whmr_mesh_render_scene, and: styles: DEVICE table of D whmr_style_row; skeletons: DEVICE table of S whmr_skeleton_row (S may
// be 0); bones [NB, 2] int32, bone_rgb [NB, 3], joint_rgb [J, 3], joints / keypoints [R, J, 3] (either may be null when no row uses it): device;
// kp_out [max(S, 1), J, 3] fp32: (u, v, w) of every skeleton row; overlay_out [total_pixels, 3] fp32 or null: the blended colour C3 of every pixel.
// Launch 2 is the scene's own kernel.  Three launches, no allocation, no synchronisation, no float atomics; bit-reproducible.
extern "C" int whmr_mesh_render_marked(const float* verts0, const float* verts1, int R, int V, const int32_t* faces, int F, const int32_t* vf_ptr,
                                       const int32_t* vf_idx, const float* cam_t, const float* focal, const void* draws, int D, const void* images, int NI,
                                       long total_pixels, const void* grounds, const void* styles, const void* skeletons, int S, const int32_t* bones, int NB,
                                       const float* bone_rgb, const float* joint_rgb, int J, const float* joints, const float* keypoints, const float* rot,
                                       float znear, float base_r, float base_g, float base_b, float ambient, float k_d, float lx, float ly, float lz,
                                       float* scr, float* nrm, void* zbuf, int32_t* heights, float* kp_out, float* color_out, int32_t* face_out,
                                       float* depth_out, int32_t* ground_out, float* ground_y, float* overlay_out, void* stream) {
    if (R <= 0 || V <= 0 || F <= 0 || D < 0 || NI <= 0 || NI > 65535 || total_pixels <= 0 || (long)D * F > 0x7fffffffL || !grounds || !heights || !ground_y)
        return (int)hipErrorInvalidValue;
    if (S < 0 || NB < 0 || J < 0 || (D > 0 && !styles) || (NB > 0 && (!bones || !bone_rgb)) || (long)S * J > 0x7fffffffL) return (int)hipErrorInvalidValue;
    if (S > 0 && (!skeletons || J < 1 || !joint_rgb || !kp_out || (!joints && !keypoints))) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    mesh_cam c{0.f, 0.f, 1.f, 0.f, rot != nullptr, {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}};
    if (rot)
        for (int k = 0; k < 9; ++k) c.r[k] = rot[k];
    mesh_shade m{base_r, base_g, base_b, ambient, k_d, lx, ly, lz};
    mesh_draw_targets tg{(const whmr_render_draw*)draws, (const whmr_render_image*)images, R, NI, verts1 != nullptr, total_pixels};
    mesh_scene sc{(const whmr_ground_row*)grounds, heights, ground_out, ground_y, D};
    mesh_marks mk{(const whmr_style_row*)styles, (const whmr_skeleton_row*)skeletons, bones, bone_rgb, joint_rgb, joints, keypoints, kp_out, overlay_out,
                  S, NB, J, R};
    long n0 = (long)D * V > total_pixels ? (long)D * V : total_pixels;                      // >= D
    if ((long)S * J > n0) n0 = (long)S * J;
    hipLaunchKernelGGL(mesh_marked_vertex_kernel, dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0, st, verts0, verts1, faces, vf_ptr, vf_idx, cam_t, focal, scr,
                       nrm, (unsigned long long*)zbuf, D, V, tg, c, heights, mk, znear);
    WHMR_CHECK_LAUNCH();
    if (D > 0) {
        const long n1 = (long)D * (F > V ? F : V);
        hipLaunchKernelGGL(mesh_scene_faces_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, st, verts0, verts1, scr, faces, (unsigned long long*)zbuf,
                           V, F, znear, tg, sc);
        WHMR_CHECK_LAUNCH();
    }
    const long mean_plane = (total_pixels + NI - 1) / NI;
    hipLaunchKernelGGL(mesh_marked_resolve_kernel, dim3((unsigned)((mean_plane + 255) / 256), (unsigned)NI), dim3(256), 0, st, scr, nrm, faces,
                       (const unsigned long long*)zbuf, color_out, face_out, depth_out, cam_t, focal, V, F, znear, tg, m, c, sc, mk);
    WHMR_CHECK_LAUNCH();
    return 0;
}

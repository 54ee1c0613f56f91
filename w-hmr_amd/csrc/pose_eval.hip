// Evaluation metrics on the device: MPJPE, PA-MPJPE and PVE of evaluate/eval.py:193-228 / core/trainer.py:754-907, and the
// Procrustes alignment of utils/pose_utils.py:10-76 (compute_similarity_transform / reconstruction_error) that the reference runs as a Python
// loop of np.linalg.svd calls behind two .cpu().numpy() syncs per batch.
//
// Procrustes: one wave per sample, lane i holds point i (N <= 64).  Everything after the fp32 loads is fp64.  The rotation maximising
// trace(R K), K = X1 X2^T, is found with Horn's quaternion method: the eigenvector of the largest eigenvalue of the symmetric 4x4 matrix built
// from K, by a fixed number of cyclic Jacobi sweeps (5 reach fp64 resolution on random, mirrored and collinear point sets; 8 are run).  A unit
// quaternion is always a proper rotation -- what the reference's Z[-1,-1] = sign(det(U V^T)) correction of the SVD achieves.  All lanes
// hold the same sums (the xor butterfly adds the same two values on both sides), so the 4x4 solve runs redundantly in every lane.
//
// pose_metrics: pass 1 = grid (B, chunks of PE_VC vertices; neighbouring workgroups share a J_reg chunk in L2): the chunk of both meshes
// is staged in LDS once; the PVE partial and the (1 + nj) regressed rows (pelvis row 0, then the joint_map rows) are reduced inside the
// workgroup in a fixed order and stored as fp64 partials.  Pass 2 = one wave per sample: the partials summed in chunk order (no atomics: repeated runs are bit-identical), pelvis
// subtraction, MPJPE, Procrustes, PA-MPJPE.  Both passes allocate nothing (the caller owns the workspace): graph-capturable.
#include "common.h"

#define PE_VC 512            // vertices per workgroup of pass 1 (2 per thread)
#define PE_SWEEPS 8          // cyclic Jacobi sweeps of the 4x4 eigenproblem

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one Jacobi rotation in the (p, q) plane that zeroes A[p][q] (Golub & Van Loan, sym.schur2); Vm accumulates the eigenvectors as columns
template <int p, int q>
__device__ __forceinline__ void jacobi_rot(double (&A)[4][4], double (&Vm)[4][4]) {
    const double apq = A[p][q];
    if (apq == 0.0) return;
    const double tau = (A[q][q] - A[p][p]) / (2.0 * apq);
    const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
    const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
#pragma unroll
    for (int k = 0; k < 4; ++k) { const double x = A[k][p], y = A[k][q]; A[k][p] = c * x - s * y; A[k][q] = s * x + c * y; }
#pragma unroll
    for (int k = 0; k < 4; ++k) { const double x = A[p][k], y = A[q][k]; A[p][k] = c * x - s * y; A[q][k] = s * x + c * y; }
#pragma unroll
    for (int k = 0; k < 4; ++k) { const double x = Vm[k][p], y = Vm[k][q]; Vm[k][p] = c * x - s * y; Vm[k][q] = s * x + c * y; }
}

// Similarity transform (s, R, t) taking the N points s1 closest to s2 (pose_utils.py:10-56), one wave, lane i = point i (valid = i < N).
// hat = s R s1 + t for this lane's point; returns the mean over the N points of |hat - s2| (pose_utils.py:69).  var1 = 0 gives NaN, as numpy.
__device__ double procrustes_wave(const double (&s1)[3], const double (&s2)[3], bool valid, int N, double (&hat)[3]) {
    double mu1[3], mu2[3], x1[3], x2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        mu1[k] = wave_sum_f64(valid ? s1[k] : 0.0) / N;
        mu2[k] = wave_sum_f64(valid ? s2[k] : 0.0) / N;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        x1[k] = valid ? s1[k] - mu1[k] : 0.0;
        x2[k] = valid ? s2[k] - mu2[k] : 0.0;
    }
    const double var1 = wave_sum_f64(x1[0] * x1[0] + x1[1] * x1[1] + x1[2] * x1[2]);
    double K[3][3];                                                     // K = X1 . X2^T
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) K[a][b] = wave_sum_f64(x1[a] * x2[b]);
    // Horn (1987): the unit quaternion of the rotation maximising sum_i (R x1_i) . x2_i is the top eigenvector of this matrix
    const double xx = K[0][0], xy = K[0][1], xz = K[0][2], yx = K[1][0], yy = K[1][1], yz = K[1][2], zx = K[2][0], zy = K[2][1], zz = K[2][2];
    double A[4][4] = {{xx + yy + zz, yz - zy, zx - xz, xy - yx},
                      {yz - zy, xx - yy - zz, xy + yx, zx + xz},
                      {zx - xz, xy + yx, -xx + yy - zz, yz + zy},
                      {xy - yx, zx + xz, yz + zy, -xx - yy + zz}};
    double Vm[4][4] = {{1.0, 0.0, 0.0, 0.0}, {0.0, 1.0, 0.0, 0.0}, {0.0, 0.0, 1.0, 0.0}, {0.0, 0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < PE_SWEEPS; ++sweep) {
        jacobi_rot<0, 1>(A, Vm); jacobi_rot<0, 2>(A, Vm); jacobi_rot<0, 3>(A, Vm);
        jacobi_rot<1, 2>(A, Vm); jacobi_rot<1, 3>(A, Vm); jacobi_rot<2, 3>(A, Vm);
    }
    double best = A[0][0], w = Vm[0][0], x = Vm[1][0], y = Vm[2][0], z = Vm[3][0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (A[i][i] > best) { best = A[i][i]; w = Vm[0][i]; x = Vm[1][i]; y = Vm[2][i]; z = Vm[3][i]; }
    const double R[3][3] = {{w * w + x * x - y * y - z * z, 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)},
                            {2.0 * (y * x + w * z), w * w - x * x + y * y - z * z, 2.0 * (y * z - w * x)},
                            {2.0 * (z * x - w * y), 2.0 * (z * y + w * x), w * w - x * x - y * y + z * z}};
    double tr = 0.0;                                                    // trace(R K)
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) tr += R[a][b] * K[b][a];
    const double scale = tr / var1;
    double d2 = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double t = mu2[a] - scale * (R[a][0] * mu1[0] + R[a][1] * mu1[1] + R[a][2] * mu1[2]);
        hat[a] = scale * (R[a][0] * s1[0] + R[a][1] * s1[1] + R[a][2] * s1[2]) + t;
        const double d = hat[a] - s2[a];
        d2 += d * d;
    }
    return wave_sum_f64(valid ? sqrt(d2) : 0.0) / N;
}

// S1, S2, S1_hat: [B, N, 3]; err: [B].  One wave per sample, 4 per workgroup.
__global__ __launch_bounds__(256) void similarity_transform_kernel(const float* __restrict__ S1, const float* __restrict__ S2, int B, int N,
                                                                   float* __restrict__ S1_hat, float* __restrict__ err) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;                                                 // wave-uniform
    const bool valid = lane < N;
    const size_t o = ((size_t)b * N + (valid ? lane : 0)) * 3;
    double s1[3], s2[3], hat[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s1[k] = valid ? (double)S1[o + k] : 0.0;
        s2[k] = valid ? (double)S2[o + k] : 0.0;
    }
    const double e = procrustes_wave(s1, s2, valid, N, hat);
    if (S1_hat && valid)
#pragma unroll
        for (int k = 0; k < 3; ++k) S1_hat[o + k] = (float)hat[k];
    if (err && lane == 0) err[b] = (float)e;
}

// Pass 1.  Rows r = 0..nj of a sample's partial: J_reg row 0 (the pelvis, taken before the mapping: eval.py:201,213), then J_reg row
// joint_map[r - 1]; 6 doubles each (pred xyz, gt xyz).  ws_rows[((b * C + c) * (nj + 1) + r) * 6 + k], ws_pve[b * C + c].
__global__ __launch_bounds__(256) void pose_vertex_pass_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int V,
                                                               const float* __restrict__ J_reg, int nJ, const int* __restrict__ joint_map,
                                                               int nj, int C, double* __restrict__ ws_rows, double* __restrict__ ws_pve) {
    __shared__ float sp[PE_VC * 3], sg[PE_VC * 3];
    __shared__ double spve[4];
    const int b = blockIdx.x, c = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int v0 = c * PE_VC, nv = min(PE_VC, V - v0);
    const size_t base = ((size_t)b * V + v0) * 3;
    for (int i = tid; i < nv * 3; i += 256) {
        sp[i] = pred[base + i];
        sg[i] = gt[base + i];
    }
    __syncthreads();
    // PVE over the raw vertices (eval.py:195-197): sum of |pred - gt| of this chunk
    double e = 0.0;
    for (int v = tid; v < nv; v += 256) {
        const double dx = (double)sp[3 * v] - sg[3 * v], dy = (double)sp[3 * v + 1] - sg[3 * v + 1], dz = (double)sp[3 * v + 2] - sg[3 * v + 2];
        e += sqrt(dx * dx + dy * dy + dz * dz);
    }
    e = wave_sum_f64(e);
    if (lane == 0) spve[wv] = e;
    // joint regression (eval.py:199,210): wave wv takes rows wv, wv + 4, ...; fp32 x fp32 products are exact in fp64
    const int R = nj + 1;
    const size_t slot = (size_t)b * C + c;
    for (int r = wv; r < R; r += 4) {
        const int row = r == 0 ? 0 : joint_map[r - 1];
        double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if ((unsigned)row < (unsigned)nJ) {                             // an out-of-range map entry is flagged by pass 2
            const float* J = J_reg + (size_t)row * V + v0;
            for (int v = lane; v < nv; v += 64) {
                const double j = J[v];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    a[k] += j * (double)sp[3 * v + k];
                    a[3 + k] += j * (double)sg[3 * v + k];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) a[k] = wave_sum_f64(a[k]);
        if (lane < 6) {
            double out = a[0];
#pragma unroll
            for (int k = 1; k < 6; ++k) out = lane == k ? a[k] : out;
            ws_rows[(slot * R + r) * 6 + lane] = out;
        }
    }
    __syncthreads();
    if (tid == 0) ws_pve[slot] = ((spve[0] + spve[1]) + spve[2]) + spve[3];
}

// Pass 2.  One wave per sample: lane r sums row r over the C chunks in chunk order; lane i < nj then holds joint i (row i + 1) minus the pelvis.
__global__ __launch_bounds__(256) void pose_finalize_kernel(const double* __restrict__ ws_rows, const double* __restrict__ ws_pve, int B, int V,
                                                            int nJ, const int* __restrict__ joint_map, int nj, int C, float* __restrict__ mpjpe,
                                                            float* __restrict__ pa_mpjpe, float* __restrict__ pve, float* __restrict__ pred_j,
                                                            float* __restrict__ pred_j_pa) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;                                                 // wave-uniform
    const int R = nj + 1;
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, pv = 0.0;
    if (lane < R)
        for (int c = 0; c < C; ++c) {
            const double* p = ws_rows + (((size_t)b * C + c) * R + lane) * 6;
#pragma unroll
            for (int k = 0; k < 6; ++k) a[k] += p[k];
        }
    if (lane == 0)
        for (int c = 0; c < C; ++c) pv += ws_pve[(size_t)b * C + c];
    const bool valid = lane < nj;
    const bool bad = __any(valid && (unsigned)joint_map[valid ? lane : 0] >= (unsigned)nJ);
    double p[3], g[3], hat[3], d2 = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double pp = __shfl(a[k], 0, 64), gp = __shfl(a[3 + k], 0, 64);          // pelvis (eval.py:201,213)
        const double pj = __shfl(a[k], lane + 1, 64), gj = __shfl(a[3 + k], lane + 1, 64);
        p[k] = valid ? pj - pp : 0.0;                                                   // eval.py:202-203,214-215
        g[k] = valid ? gj - gp : 0.0;
        d2 += (p[k] - g[k]) * (p[k] - g[k]);
    }
    const double mp = wave_sum_f64(valid ? sqrt(d2) : 0.0) / nj;                        // eval.py:218
    const double pa = procrustes_wave(p, g, valid, nj, hat);                            // eval.py:222-223
    const double nan = __builtin_nan("");
    if (lane == 0) {
        mpjpe[b] = (float)(bad ? nan : mp);
        pa_mpjpe[b] = (float)(bad ? nan : pa);
        pve[b] = (float)(bad ? nan : pv / V);
    }
    if (valid) {
        const size_t o = ((size_t)b * nj + lane) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (pred_j) pred_j[o + k] = (float)(bad ? nan : p[k]);
            if (pred_j_pa) pred_j_pa[o + k] = (float)(bad ? nan : hat[k]);
        }
    }
}

static inline int C_of(int V) { return (V + PE_VC - 1) / PE_VC; }

static inline long pose_metrics_ws_bytes(int B, int V, int nj) {
    const long C = C_of(V);
    return (long)B * C * (6L * (nj + 1) + 1) * (long)sizeof(double);
}

extern "C" int whmr_similarity_transform(const float* S1, const float* S2, int B, int N, float* S1_hat, float* err, void* stream) {
    if (B <= 0 || N <= 0 || N > 64 || !S1 || !S2) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(similarity_transform_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, S1, S2, B, N, S1_hat, err);
    WHMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int whmr_pose_metrics_workspace(int B, int V, int nj, long* bytes) {
    if (B <= 0 || V <= 0 || nj <= 0 || nj > 63 || !bytes) return (int)hipErrorInvalidValue;
    *bytes = pose_metrics_ws_bytes(B, V, nj);
    return 0;
}

extern "C" int whmr_pose_metrics(const float* pred_verts, const float* gt_verts, int B, int V, const float* J_reg, int nJ, const int* joint_map,
                                 int nj, float* mpjpe, float* pa_mpjpe, float* pve, float* pred_j, float* pred_j_pa, void* workspace,
                                 long workspace_bytes, void* stream) {
    if (B <= 0 || V <= 0 || nJ <= 0 || nj <= 0 || nj > 63 || C_of(V) > 65535 || !pred_verts || !gt_verts || !J_reg || !joint_map || !mpjpe ||
        !pa_mpjpe || !pve || !workspace || workspace_bytes < pose_metrics_ws_bytes(B, V, nj))
        return (int)hipErrorInvalidValue;
    const int C = C_of(V);
    double* ws_rows = (double*)workspace;
    double* ws_pve = ws_rows + (size_t)B * C * (nj + 1) * 6;
    hipLaunchKernelGGL(pose_vertex_pass_kernel, dim3(B, C), dim3(256), 0, (hipStream_t)stream, pred_verts, gt_verts, V, J_reg, nJ, joint_map,
                       nj, C, ws_rows, ws_pve);
    WHMR_CHECK_LAUNCH();
    hipLaunchKernelGGL(pose_finalize_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, ws_rows, ws_pve, B, V, nJ, joint_map, nj, C,
                       mpjpe, pa_mpjpe, pve, pred_j, pred_j_pa);
    WHMR_CHECK_LAUNCH();
    return 0;
}

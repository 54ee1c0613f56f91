// The W-HMR training objective on preds_dict['smpl_out'][1..3], forward and backward (gfx950, wave64).
//
// Reference: core/trainer.py:498-609.  Per supervised stage l = 1..3 (entry 0, the mean-pose mesh, is skipped: :511-513) up to ten scalar terms --
// smpl_losses (:242-253), keypoint_3d_loss (:214-231), shape_loss on the three mesh resolutions (:233-240, l > 2 only: :576-582), the camera term
// (:586), keypoint_loss on the crop and world projections (:203-212, :544-564) and the focal-length MSE (:566-569).  The reference gathers the
// supervised samples with boolean masks (x[has_smpl]) and branches on len(...) > 0: every one of those reads the mask on the host.  Here a masked
// sample contributes an exact zero, the valid count is summed on the device and enters as the normaliser, and "no valid sample" selects 0.0 for the
// value and for every gradient -- nothing is read back, so the three launches can be captured into a graph.
//
// Forward, launch 1 (loss_partial_kernel): every enabled (stage, term) pair is cut into chunks of LOSS_CHUNK units (a unit = the smallest piece
// that shares work: a joint's 3 x 3 block for the pose term -- one batch_rodrigues per joint --, a joint for the keypoint terms, a sample for the
// camera / focal terms, an element elsewhere); one workgroup per chunk adds its units in a fixed order (4 per thread, wave64 butterfly, the four
// wave sums through LDS) and writes ONE partial.  Launch 2 (loss_finish_kernel, one workgroup): the valid counts, then per term the partials
// lane-strided in index order + the butterfly, times weight / normaliser -> losses[30].  No atomics: two calls give the same bits.
// Backward (loss_bwd_kernel): one elementwise launch over the same chunks writes d(sum_k g[k] losses[k]) / d(input) for every input of every stage.
//
// The node is launch-bound, not bandwidth-bound (the three vertex terms of the last stage are ~5 MB each way at batch 64): plain coalesced 4-byte
// accesses, four in flight per thread.
#include "../../include/whmr_hip.h"
#include "geometry_dev.h"

namespace {

constexpr int LOSS_THREADS = 256, LOSS_PER_THREAD = 4, LOSS_CHUNK = LOSS_THREADS * LOSS_PER_THREAD;
constexpr int NT = WHMR_LOSS_STAGES * WHMR_LOSS_TERMS;
enum { T_POSE, T_BETAS, T_KP3D, T_VERTS, T_SUB, T_TEMP, T_CAM, T_KP2D, T_KP2DW, T_FOCAL };

struct loss_plan { int begin[NT + 1]; };        // first workgroup of every (stage, term); begin[NT] = the grid

__host__ __device__ inline float* field(const whmr_loss_stage& s, int term) {
    switch (term) {
        case T_POSE: return s.rotmat;
        case T_BETAS: return s.shape;
        case T_KP3D: return s.kp_3d;
        case T_VERTS: return s.verts;
        case T_SUB: return s.sub_verts;
        case T_TEMP: return s.temp_verts;
        case T_CAM: return s.cam;
        case T_KP2D: return s.kp_2d;
        case T_KP2DW: return s.kp_2d_w;
        default: return s.focal;
    }
}

__host__ __device__ inline long mesh_size(const whmr_loss_args& a, int term) { return term == T_VERTS ? a.V : term == T_SUB ? a.V_sub : a.V_temp; }

// units of a term's forward sum; the backward walks the same units except for kp_3d, whose gradient covers all 49 rows element by element
__host__ __device__ inline long units(const whmr_loss_args& a, int term, bool bwd) {
    const long B = a.B;
    switch (term) {
        case T_POSE: return B * 24;
        case T_BETAS: return B * 10;
        case T_KP3D: return bwd ? B * 147 : B * 24;
        case T_VERTS: case T_SUB: case T_TEMP: return B * mesh_size(a, term) * 3;
        case T_KP2D: case T_KP2DW: return B * 49;
        default: return B;                       // T_CAM, T_FOCAL
    }
}

// weight / normaliser of a term (the reference's .mean() / nn.MSELoss / nn.L1Loss over the gathered samples), 0 when no sample is valid
__device__ __forceinline__ float term_scale(const whmr_loss_args& a, int term, float n_smpl, float n_3d) {
    const float B = (float)a.B;
    switch (term) {
        case T_POSE: return n_smpl > 0.f ? a.w_pose / (n_smpl * 216.f) : 0.f;
        case T_BETAS: return n_smpl > 0.f ? a.w_shape / (n_smpl * 10.f) : 0.f;
        case T_KP3D: return n_3d > 0.f ? a.w_kp3d / (n_3d * 72.f) : 0.f;
        case T_VERTS: case T_SUB: case T_TEMP: return n_smpl > 0.f ? a.w_vert / (n_smpl * 3.f * (float)mesh_size(a, term)) : 0.f;
        case T_CAM: return 1.f / B;
        case T_KP2D: case T_KP2DW: return a.w_kp2d / (B * 98.f);
        default: return a.w_focal / B;
    }
}

// trainer.py:225-228: coordinate c of joint j of sample b, prediction minus target, each centred on the mean of its joints 2 and 3
__device__ __forceinline__ float kp3d_diff(const float* P /* kp_3d row 25 of the sample */, const float* G /* pose_3d of the sample */, int j, int c) {
    const float pp = (P[6 + c] + P[9 + c]) / 2.f, pg = (G[8 + c] + G[12 + c]) / 2.f;
    return (P[3 * j + c] - pp) - (G[4 * j + c] - pg);
}

// trainer.py:208-210, :501-506: confidence of keypoint row r and, for the world term, the per-sample scale of coordinate c
__device__ __forceinline__ float kp2d_conf(const whmr_loss_args& a, const float* gt, long u) {
    return gt[3 * u + 2] * ((int)(u % 49) < 25 ? a.w_openpose : a.w_gt);
}
__device__ __forceinline__ float world_scale(const whmr_loss_args& a, long b, int c) {
    return c == 0 ? a.orig_shape[2 * b + 1] / a.bbox_width[b] : a.orig_shape[2 * b] / a.bbox_height[b];
}

// one unit's contribution to the un-normalised sum of a term (an exact 0 for a masked sample)
__device__ __forceinline__ float unit_value(const whmr_loss_args& a, const whmr_loss_stage& p, int term, long u) {
    switch (term) {
        case T_POSE: {                          // trainer.py:244,248
            const long b = u / 24;
            if (a.has_smpl[b] == 0.f) return 0.f;
            float R[9], s = 0.f;
            rodrigues9(a.gt_pose + 3 * u, R);
            const float* x = p.rotmat + 9 * u;
#pragma unroll
            for (int i = 0; i < 9; ++i) { const float d = x[i] - R[i]; s += d * d; }
            return s;
        }
        case T_BETAS: {                         // trainer.py:249
            if (a.has_smpl[u / 10] == 0.f) return 0.f;
            const float d = p.shape[(u / 10) * p.shape_stride + u % 10] - a.gt_betas[u];
            return d * d;
        }
        case T_KP3D: {                          // trainer.py:218-229
            const long b = u / 24;
            const int j = (int)(u - b * 24);
            if (a.has_pose_3d[b] == 0.f) return 0.f;
            const float* P = p.kp_3d + b * 147 + 75;
            const float* G = a.pose_3d + b * 96;
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) { const float d = kp3d_diff(P, G, j, c); s += d * d; }
            return G[4 * j + 3] * s;
        }
        case T_VERTS: case T_SUB: case T_TEMP: {    // trainer.py:235-238
            if (a.has_smpl[u / (3 * mesh_size(a, term))] == 0.f) return 0.f;
            const float* gt = term == T_VERTS ? a.gt_verts : term == T_SUB ? a.gt_sub_verts : a.gt_temp_verts;
            return fabsf(field(p, term)[u] - gt[u]);
        }
        case T_CAM: {                           // trainer.py:586
            const float e = expf(-10.f * p.cam[u * p.cam_stride]);
            return e * e;
        }
        case T_KP2D: {                          // trainer.py:208-211
            const float d0 = p.kp_2d[2 * u] - a.gt_kp_2d[3 * u], d1 = p.kp_2d[2 * u + 1] - a.gt_kp_2d[3 * u + 1];
            return kp2d_conf(a, a.gt_kp_2d, u) * (d0 * d0 + d1 * d1);
        }
        case T_KP2DW: {                         // trainer.py:551-553
            const long b = u / 49;
            const float d0 = p.kp_2d_w[2 * u] - a.gt_kp_2d_w[3 * u], d1 = p.kp_2d_w[2 * u + 1] - a.gt_kp_2d_w[3 * u + 1];
            return kp2d_conf(a, a.gt_kp_2d_w, u) * (world_scale(a, b, 0) * d0 * d0 + world_scale(a, b, 1) * d1 * d1);
        }
        default: {                              // trainer.py:568
            const float d = p.focal[u] - a.gt_focal[u];
            return d * d;
        }
    }
}

// workgroup -> (stage * WHMR_LOSS_TERMS + term, chunk): the plan is a sorted table of 31 workgroup-uniform entries
__device__ __forceinline__ int find_term(const loss_plan& pl, int blk) {
    int t = 0;
    while (t < NT - 1 && blk >= pl.begin[t + 1]) ++t;
    return t;
}

__global__ __launch_bounds__(LOSS_THREADS) void loss_partial_kernel(whmr_loss_args a, loss_plan pl, float* partial) {
    __shared__ float red[LOSS_THREADS / 64];
    const int t = find_term(pl, blockIdx.x), term = t % WHMR_LOSS_TERMS;
    const whmr_loss_stage& p = a.pred[t / WHMR_LOSS_TERMS];
    const long n = units(a, term, false), u0 = (long)(blockIdx.x - pl.begin[t]) * LOSS_CHUNK + threadIdx.x;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < LOSS_PER_THREAD; ++k) {
        const long u = u0 + k * LOSS_THREADS;
        if (u < n) acc += unit_value(a, p, term, u);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// sum of x[0..n) by one wave: lane l adds x[l], x[l + 64], ... in index order, then the butterfly (every lane holds the result)
__device__ __forceinline__ float wave_strided_sum(const float* x, int n) {
    float acc = 0.f;
    for (int i = threadIdx.x & 63; i < n; i += 64) acc += x[i];
    return wave_sum(acc);
}

__global__ __launch_bounds__(LOSS_THREADS) void loss_finish_kernel(whmr_loss_args a, loss_plan pl, const float* partial, float* losses, float* counts) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // 0 / 1 flags: the sums are exact, and every wave finds the same two numbers
    const float n_smpl = wave_strided_sum(a.has_smpl, a.B), n_3d = wave_strided_sum(a.has_pose_3d, a.B);
    if (threadIdx.x == 0) { counts[0] = n_smpl; counts[1] = n_3d; }
    for (int t = wave; t < NT; t += LOSS_THREADS / 64) {
        const int nb = pl.begin[t + 1] - pl.begin[t];
        const float s = wave_strided_sum(partial + pl.begin[t], nb);
        const float scale = term_scale(a, t % WHMR_LOSS_TERMS, n_smpl, n_3d);
        if (lane == 0) losses[t] = (nb > 0 && scale != 0.f) ? s * scale : 0.f;
    }
}

__device__ __forceinline__ float sign0(float d) { return (float)((d > 0.f) - (d < 0.f)); }     // torch.sign: sign(0) = 0

// gradient of unit u of a term: k = g[term] * weight / normaliser (0 when the term has no valid sample)
__device__ __forceinline__ void unit_grad(const whmr_loss_args& a, const whmr_loss_stage& p, const whmr_loss_stage& o, int term, long u, float k) {
    switch (term) {
        case T_POSE: {
            const bool on = a.has_smpl[u / 24] != 0.f && k != 0.f;
            float R[9];
            rodrigues9(a.gt_pose + 3 * u, R);
#pragma unroll
            for (int i = 0; i < 9; ++i) o.rotmat[9 * u + i] = on ? 2.f * k * (p.rotmat[9 * u + i] - R[i]) : 0.f;
            break;
        }
        case T_BETAS:
            o.shape[u] = (a.has_smpl[u / 10] != 0.f && k != 0.f) ? 2.f * k * (p.shape[(u / 10) * p.shape_stride + u % 10] - a.gt_betas[u]) : 0.f;
            break;
        case T_KP3D: {                          // u = element of kp_3d [B, 49, 3]; rows 0..24 do not enter the loss (trainer.py:218)
            const long b = u / 147;
            const int rc = (int)(u - b * 147), r = rc / 3, c = rc - 3 * r, j = r - 25;
            float v = 0.f;
            if (j >= 0 && a.has_pose_3d[b] != 0.f && k != 0.f) {
                const float* P = p.kp_3d + b * 147 + 75;
                const float* G = a.pose_3d + b * 96;
                v = G[4 * j + 3] * kp3d_diff(P, G, j, c);
                if (j == 2 || j == 3) {         // the pelvis (trainer.py:227-228) takes minus half of every joint's gradient
                    float s = 0.f;
                    for (int q = 0; q < 24; ++q) s += G[4 * q + 3] * kp3d_diff(P, G, q, c);
                    v -= 0.5f * s;
                }
                v *= 2.f * k;
            }
            o.kp_3d[u] = v;
            break;
        }
        case T_VERTS: case T_SUB: case T_TEMP: {
            const float* gt = term == T_VERTS ? a.gt_verts : term == T_SUB ? a.gt_sub_verts : a.gt_temp_verts;
            const bool on = a.has_smpl[u / (3 * mesh_size(a, term))] != 0.f && k != 0.f;
            field(o, term)[u] = on ? k * sign0(field(p, term)[u] - gt[u]) : 0.f;
            break;
        }
        case T_CAM: {
            const float e = expf(-10.f * p.cam[u * p.cam_stride]);
            o.cam[3 * u] = -20.f * k * e * e;
            o.cam[3 * u + 1] = 0.f;
            o.cam[3 * u + 2] = 0.f;
            break;
        }
        case T_KP2D: {
            const float w = 2.f * k * kp2d_conf(a, a.gt_kp_2d, u);
            o.kp_2d[2 * u] = w * (p.kp_2d[2 * u] - a.gt_kp_2d[3 * u]);
            o.kp_2d[2 * u + 1] = w * (p.kp_2d[2 * u + 1] - a.gt_kp_2d[3 * u + 1]);
            break;
        }
        case T_KP2DW: {
            const long b = u / 49;
            const float w = 2.f * k * kp2d_conf(a, a.gt_kp_2d_w, u);
            o.kp_2d_w[2 * u] = w * world_scale(a, b, 0) * (p.kp_2d_w[2 * u] - a.gt_kp_2d_w[3 * u]);
            o.kp_2d_w[2 * u + 1] = w * world_scale(a, b, 1) * (p.kp_2d_w[2 * u + 1] - a.gt_kp_2d_w[3 * u + 1]);
            break;
        }
        default:
            o.focal[u] = 2.f * k * (p.focal[u] - a.gt_focal[u]);
            break;
    }
}

__global__ __launch_bounds__(LOSS_THREADS) void loss_bwd_kernel(whmr_loss_args a, loss_plan pl, const float* counts, const float* g) {
    const int t = find_term(pl, blockIdx.x), term = t % WHMR_LOSS_TERMS, stage = t / WHMR_LOSS_TERMS;
    const long n = units(a, term, true), u0 = (long)(blockIdx.x - pl.begin[t]) * LOSS_CHUNK + threadIdx.x;
    const float scale = term_scale(a, term, counts[0], counts[1]);
    const float k = scale != 0.f ? g[t] * scale : 0.f;
#pragma unroll
    for (int i = 0; i < LOSS_PER_THREAD; ++i) {
        const long u = u0 + i * LOSS_THREADS;
        if (u < n) unit_grad(a, a.pred[stage], a.grad[stage], term, u, k);
    }
}

// the grid: chunks of every enabled (stage, term); -1 when the arguments are outside the contract
long make_plan(const whmr_loss_args& a, bool bwd, loss_plan& pl) {
    if (a.B <= 0 || !a.gt_pose || !a.gt_betas || !a.pose_3d || !a.has_smpl || !a.has_pose_3d) return -1;
    long blocks = 0;
    for (int s = 0; s < WHMR_LOSS_STAGES; ++s)
        for (int term = 0; term < WHMR_LOSS_TERMS; ++term) {
            pl.begin[s * WHMR_LOSS_TERMS + term] = (int)blocks;
            if (!field(a.pred[s], term)) continue;
            if ((term == T_BETAS && a.pred[s].shape_stride < 10) || (term == T_CAM && a.pred[s].cam_stride < 1)) return -1;
            if (bwd && !field(a.grad[s], term)) return -1;
            if (term >= T_VERTS && term <= T_TEMP) {
                const float* gt = term == T_VERTS ? a.gt_verts : term == T_SUB ? a.gt_sub_verts : a.gt_temp_verts;
                if (!gt || mesh_size(a, term) <= 0) return -1;
            }
            if (term == T_KP2D && !a.gt_kp_2d) return -1;
            if (term == T_KP2DW && (!a.gt_kp_2d_w || !a.orig_shape || !a.bbox_width || !a.bbox_height)) return -1;
            if (term == T_FOCAL && !a.gt_focal) return -1;
            blocks += (units(a, term, bwd) + LOSS_CHUNK - 1) / LOSS_CHUNK;
            if (blocks > 0x7fffffffL) return -1;
        }
    pl.begin[NT] = (int)blocks;
    return blocks;
}

}  // namespace

extern "C" int whmr_train_losses_workspace(const whmr_loss_args* a, long* n_floats) {
    loss_plan pl;
    if (!a || !n_floats) return (int)hipErrorInvalidValue;
    const long blocks = make_plan(*a, false, pl);
    if (blocks < 0) return (int)hipErrorInvalidValue;
    *n_floats = blocks > 0 ? blocks : 1;
    return 0;
}

extern "C" int whmr_train_losses(const whmr_loss_args* a, float* partial, float* losses, float* counts, void* stream) {
    loss_plan pl;
    if (!a || !partial || !losses || !counts) return (int)hipErrorInvalidValue;
    const long blocks = make_plan(*a, false, pl);
    if (blocks < 0) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    if (blocks > 0) {
        hipLaunchKernelGGL(loss_partial_kernel, dim3((unsigned)blocks), dim3(LOSS_THREADS), 0, st, *a, pl, partial);
        WHMR_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(LOSS_THREADS), 0, st, *a, pl, (const float*)partial, losses, counts);
    WHMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int whmr_train_losses_bwd(const whmr_loss_args* a, const float* counts, const float* g, void* stream) {
    loss_plan pl;
    if (!a || !counts || !g) return (int)hipErrorInvalidValue;
    const long blocks = make_plan(*a, true, pl);
    if (blocks < 0) return (int)hipErrorInvalidValue;
    if (blocks > 0) {
        hipLaunchKernelGGL(loss_bwd_kernel, dim3((unsigned)blocks), dim3(LOSS_THREADS), 0, (hipStream_t)stream, *a, pl, counts, g);
        WHMR_CHECK_LAUNCH();
    }
    return 0;
}

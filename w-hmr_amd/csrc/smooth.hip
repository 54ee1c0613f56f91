// Temporal smoothing of tracked persons behind clip inference (the --smooth / --min_cutoff / --beta flags of demo/whmr_demo.py:135-144, which the
// reference parses and drops): a one-euro filter per track, with time counted in frames.
//
// whmr_track_smooth walks every track of a clip in ONE launch.  Work item = one wavefront (a workgroup of 64 threads):
//   items 0 .. T-1      one TRACK each: the rows rows[track_offsets[t] .. track_offsets[t+1]) of the clip in frame order, gap[k] frames after the
//                       track's previous sample (0: the track starts or restarts at this row), filter state kept in slot[t] of the state arrays;
//   items T .. T+U-1    one UNTRACKED row each (rows[n_tracked + i]): passed through, no state.
//   lane 0 .. 23        rotation channel of joint `lane` of local_pose        lane 24       rotation channel of joint 0 of global_pose
//   lane 25 .. 38       scalar channels: cam_t (3), focal (1), shape (10)     lane 39 .. 63 idle
// The filter is sequential in time and independent across tracks, joints and channels, so each lane keeps its channel's state in registers and walks
// the track's rows in order; nothing is exchanged between lanes, there is no LDS, no barrier and no atomic, and every output element is written by
// exactly one lane (`rows` names every row of the clip once) -- repeated runs are bit-identical.  The work is latency-bound (a few hundred dependent
// fp32 operations per row and channel); the point of the kernel is ONE launch and no host round trip.  A wavefront per workgroup spreads the tracks
// over the CUs: nothing would be shared inside a larger workgroup.
//
// Scalar channel, gap D >= 1, a(f, D) = r / (r + 1) with r = 2 pi f D:
//   dx = (x - xh) / D;  dxh = a(d_cutoff, D) dx + (1 - a(d_cutoff, D)) dxh;  f = min_cutoff + beta |dxh|;  xh = a(f, D) x + (1 - a(f, D)) xh
//   -- the recurrence of the reference tree's OneEuroFilter (models/ViTPose/mmpose/core/post_processing/one_euro_filter.py:59-102) built with
//   fps = d_cutoff and called with t_e = D.
// Rotation channel on SO(3) (this package's form: the reference defines no smoothing of rotations; an axis-angle filter would wrap at pi, where
// SMPL's root orientation in camera coordinates usually sits):
//   v = log(Rh^T R);  w = v / D;  wh = a(d_cutoff, D) w + (1 - a(d_cutoff, D)) wh;  f = min_cutoff + beta |wh|;  Rh = GramSchmidt(Rh exp(a(f, D) v))
//   log = rotmat_to_aa3, exp = rodrigues9, GramSchmidt = gram_schmidt9 (geometry_dev.h); the re-orthonormalisation keeps a streamed track of
//   thousands of frames on SO(3).
// First sample of a track (gap 0): xh = x, dxh = 0, Rh = R = exp(pose), wh = 0, and the row's poses and scalars leave as the bits they came in.
#include "common.h"
#include "geometry_dev.h"
#include "../../include/whmr_hip.h"

// one arithmetic for a row whether its predecessor came from this call or from the state arrays: no contraction into fused multiply-adds
#pragma clang fp contract(off)

#define SMOOTH_ROT 25          // rotation channels per track
#define SMOOTH_SCALAR 14       // scalar channels per track

struct smooth_args {
    const float *local_pose, *global_pose, *cam_t, *focal, *shape;
    const int32_t *track_offsets, *rows, *gap, *slot;
    float *state_R, *state_w, *state_x, *state_dx;
    float *o_local_rotmat, *o_global_rotmat, *o_local_pose, *o_global_pose, *o_cam_t, *o_focal, *o_shape;
    int P, T, n_tracked, n_slots;
    float min_cutoff, beta, two_pi_dcutoff;
};

__device__ __forceinline__ float smoothing_factor(float two_pi_cutoff, float gap) {
    const float r = two_pi_cutoff * gap;
    return r / (r + 1.0f);
}

// o = a^T b (row-major 3x3)
__device__ __forceinline__ void mul_tn9(const float* a, const float* b, float* o) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o[3 * i + j] = a[i] * b[j] + a[3 + i] * b[3 + j] + a[6 + i] * b[6 + j];
}

// o = a b
__device__ __forceinline__ void mul9(const float* a, const float* b, float* o) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

__global__ __launch_bounds__(64) void track_smooth_kernel(const smooth_args a) {
    const int item = blockIdx.x, lane = threadIdx.x;
    if (lane >= SMOOTH_ROT + SMOOTH_SCALAR) return;
    int k0, k1, slot = -1;
    if (item < a.T) {
        k0 = a.track_offsets[item];
        k1 = a.track_offsets[item + 1];
        slot = a.slot[item];
        if (slot < 0 || slot >= a.n_slots || k1 > a.n_tracked) return;      // a table the host did not build: touch nothing
    } else {
        k0 = a.n_tracked + (item - a.T);                        // an untracked row: one sample, no state
        k1 = k0 + 1;
    }
    if (k0 < 0 || k1 > a.P || k0 >= k1) return;
    const bool tracked = item < a.T;

    if (lane < SMOOTH_ROT) {
        const int joint = lane < 24 ? lane : 0;
        float Rh[9], wh[3];
        bool have = false;
        if (tracked && a.gap[k0] > 0) {                       // the track continues from an earlier call
#pragma unroll
            for (int i = 0; i < 9; ++i) Rh[i] = a.state_R[((long)slot * SMOOTH_ROT + lane) * 9 + i];
#pragma unroll
            for (int i = 0; i < 3; ++i) wh[i] = a.state_w[((long)slot * SMOOTH_ROT + lane) * 3 + i];
            have = true;
        }
        for (int k = k0; k < k1; ++k) {
            const int row = a.rows[k];
            if (row < 0 || row >= a.P) continue;
            const int g = tracked ? a.gap[k] : 0;
            const float* src = (lane < 24 ? a.local_pose : a.global_pose) + (long)row * 72 + 3 * joint;
            const float t[3] = {src[0], src[1], src[2]};
            float R[9], aa[3];
            rodrigues9(t, R);
            const bool first = g <= 0 || !have;
            if (first) {
#pragma unroll
                for (int i = 0; i < 9; ++i) Rh[i] = R[i];
                wh[0] = wh[1] = wh[2] = 0.f;
                aa[0] = t[0]; aa[1] = t[1]; aa[2] = t[2];
                have = true;
            } else {
                const float gap = (float)g;
                float M[9], v[3], E[9], N[9];
                mul_tn9(Rh, R, M);
                rotmat_to_aa3(M, v);
                const float ad = smoothing_factor(a.two_pi_dcutoff, gap);
#pragma unroll
                for (int i = 0; i < 3; ++i) wh[i] = ad * (v[i] / gap) + (1.0f - ad) * wh[i];
                const float f = a.min_cutoff + a.beta * sqrtf(wh[0] * wh[0] + wh[1] * wh[1] + wh[2] * wh[2]);
                const float al = smoothing_factor(6.283185307179586f * f, gap);
                const float step[3] = {al * v[0], al * v[1], al * v[2]};
                rodrigues9(step, E);
                mul9(Rh, E, N);
                gram_schmidt9(N, Rh);
                rotmat_to_aa3(Rh, aa);
            }
            if (lane < 24) {
#pragma unroll
                for (int i = 0; i < 9; ++i) a.o_local_rotmat[((long)row * 24 + lane) * 9 + i] = Rh[i];
#pragma unroll
                for (int i = 0; i < 3; ++i) a.o_local_pose[(long)row * 72 + 3 * lane + i] = aa[i];
            }
            if (lane >= 1) {                                  // global = [filtered global root | local joints 1 .. 23]
                const int gj = lane < 24 ? lane : 0;
                if (first && lane < 24) {                     // an unfiltered row keeps the bits of ITS global_pose
                    const float* gsrc = a.global_pose + (long)row * 72 + 3 * lane;
                    aa[0] = gsrc[0]; aa[1] = gsrc[1]; aa[2] = gsrc[2];
                }
#pragma unroll
                for (int i = 0; i < 9; ++i) a.o_global_rotmat[((long)row * 24 + gj) * 9 + i] = Rh[i];
#pragma unroll
                for (int i = 0; i < 3; ++i) a.o_global_pose[(long)row * 72 + 3 * gj + i] = aa[i];
            }
        }
        if (tracked && have) {
#pragma unroll
            for (int i = 0; i < 9; ++i) a.state_R[((long)slot * SMOOTH_ROT + lane) * 9 + i] = Rh[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) a.state_w[((long)slot * SMOOTH_ROT + lane) * 3 + i] = wh[i];
        }
        return;
    }

    const int c = lane - SMOOTH_ROT;                          // 0 .. 2 cam_t, 3 focal, 4 .. 13 shape
    const float* in = c < 3 ? a.cam_t + c : c == 3 ? a.focal : a.shape + (c - 4);
    float* out = c < 3 ? a.o_cam_t + c : c == 3 ? a.o_focal : a.o_shape + (c - 4);
    const int ld = c < 3 ? 3 : c == 3 ? 1 : 10;
    float xh = 0.f, dxh = 0.f;
    bool have = false;
    if (tracked && a.gap[k0] > 0) {
        xh = a.state_x[(long)slot * SMOOTH_SCALAR + c];
        dxh = a.state_dx[(long)slot * SMOOTH_SCALAR + c];
        have = true;
    }
    for (int k = k0; k < k1; ++k) {
        const int row = a.rows[k];
        if (row < 0 || row >= a.P) continue;
        const int g = tracked ? a.gap[k] : 0;
        const float x = in[(long)row * ld];
        if (g <= 0 || !have) {
            xh = x;
            dxh = 0.f;
            have = true;
        } else {
            const float gap = (float)g;
            const float ad = smoothing_factor(a.two_pi_dcutoff, gap);
            dxh = ad * ((x - xh) / gap) + (1.0f - ad) * dxh;
            const float al = smoothing_factor(6.283185307179586f * (a.min_cutoff + a.beta * fabsf(dxh)), gap);
            xh = al * x + (1.0f - al) * xh;
        }
        out[(long)row * ld] = xh;
    }
    if (tracked && have) {
        a.state_x[(long)slot * SMOOTH_SCALAR + c] = xh;
        a.state_dx[(long)slot * SMOOTH_SCALAR + c] = dxh;
    }
}

extern "C" int whmr_track_smooth(const float* local_pose, const float* global_pose, const float* cam_t, const float* focal, const float* shape, int P,
                                 const int32_t* track_offsets, const int32_t* rows, const int32_t* gap, const int32_t* slot, int T, int n_tracked,
                                 float* state_R, float* state_w, float* state_x, float* state_dx, int n_slots,
                                 double min_cutoff, double beta, double d_cutoff,
                                 float* local_rotmat, float* global_rotmat, float* local_pose_out, float* global_pose_out, float* cam_t_out,
                                 float* focal_out, float* shape_out, void* stream) {
    if (!local_pose || !global_pose || !cam_t || !focal || !shape || !track_offsets || !rows || !local_rotmat || !global_rotmat || !local_pose_out ||
        !global_pose_out || !cam_t_out || !focal_out || !shape_out)
        return (int)hipErrorInvalidValue;
    if (P <= 0 || T < 0 || n_tracked < 0 || n_tracked > P || T > n_tracked || n_slots < 0 || T > n_slots) return (int)hipErrorInvalidValue;
    if (T > 0 && (!gap || !slot || !state_R || !state_w || !state_x || !state_dx)) return (int)hipErrorInvalidValue;
    if (!(min_cutoff > 0.0) || !(beta >= 0.0) || !(d_cutoff > 0.0) || min_cutoff > 1e30 || beta > 1e30 || d_cutoff > 1e30) return (int)hipErrorInvalidValue;
    smooth_args a;
    a.local_pose = local_pose; a.global_pose = global_pose; a.cam_t = cam_t; a.focal = focal; a.shape = shape;
    a.track_offsets = track_offsets; a.rows = rows; a.gap = gap; a.slot = slot;
    a.state_R = state_R; a.state_w = state_w; a.state_x = state_x; a.state_dx = state_dx;
    a.o_local_rotmat = local_rotmat; a.o_global_rotmat = global_rotmat; a.o_local_pose = local_pose_out; a.o_global_pose = global_pose_out;
    a.o_cam_t = cam_t_out; a.o_focal = focal_out; a.o_shape = shape_out;
    a.P = P; a.T = T; a.n_tracked = n_tracked; a.n_slots = n_slots;
    a.min_cutoff = (float)min_cutoff; a.beta = (float)beta; a.two_pi_dcutoff = (float)(6.283185307179586 * d_cutoff);
    hipLaunchKernelGGL(track_smooth_kernel, dim3(T + (P - n_tracked)), dim3(64), 0, (hipStream_t)stream, a);
    WHMR_CHECK_LAUNCH();
    return 0;
}

// Adam step of a whole model in two launches over a device-resident table (reference: torch.optim.Adam as core/trainer.py:615 steps it --
// non-amsgrad, L2 weight decay), capturable in a HIP graph: the step counts, the bias corrections and the hyper-parameters all live in device
// memory, so a replayed graph advances them and follows a learning rate the host changed between two replays.
//   whmr_adam_advance   one thread per parameter: step += 1, bias corrections 1 - beta^step (double precision) into the table
//   whmr_adam_step      one workgroup per 4096-element chunk ("flat" item) or per 64x64 tile ("tile" item: the fp32 matrices whose bf16 W / W^T
//                       operand copies the ViT's GEMMs read -- the update writes both copies from the registers and the LDS tile it already holds,
//                       which is the pass whmr_weights_prepare (train_ops.hip) would otherwise make over the weights after the step)
// The gradient guard (optional; the three launches of a guarded step): global L2 norm of the gradients, clipping by it, skipping a non-finite step
//   whmr_adam_grad_sumsq     the step launch's grid and adam_find_item decomposition; workgroup b reads the 4096-element chunk b - block_begin of its
//                            item's gradient -- tile items too: their gradient is the same contiguous N x K floats, and ceil(N/64) ceil(K/64) tiles are
//                            never fewer than ceil(N K / 4096) chunks, so the spare workgroups of a tile item write 0.0 -- and writes ONE double to
//                            partials[b].  No atomics, no memset.  Each thread squares and accumulates its <= 16 elements in fp32 (16 squares and 15
//                            sums of non-negative terms: relative error of a thread's sum <= 16 x 2^-24 < 1.0e-6); from there on everything is summed
//                            in double in a fixed order (64 lanes by shuffles, 4 waves through LDS), so the norm carries <= ~5e-7 relative error plus
//                            its final rounding to fp32, and the same inputs give the same bits
//   whmr_adam_guard_advance  ONE workgroup: sums the partials (thread t takes t, t + 256, ...; LDS tree), writes norm / coefficient / decision / counters
//                            to struct whmr_adam_guard_state and, if the step is applied, does whmr_adam_advance's work.  A model has ~30 k workgroups
//                            = 240 KB of doubles: 120 loads per thread, a few microseconds, so a two-level tree would only buy back a launch it costs
//   whmr_adam_step_guarded   whmr_adam_step reading the decision: returns before touching anything when the step is skipped, else updates with
//                            fp32(g * coef) (coef == 1 multiplies exactly: a guarded step that does not clip has the unguarded step's bits)
// Memory-bound (28 B per parameter; the guard reads the gradients once more: 4 B): 16-byte accesses where the four pointers of an item allow them -- gradients may be views into GradReducer's
// flat buckets, which guarantee 4 bytes only -- and a dword path otherwise.  Built without packed-fp32 instructions (build.py: NO_PACKED_FP32).
#include "common.h"
#include "../../include/whmr_hip.h"

static_assert(sizeof(whmr_adam_item) == 104 && sizeof(whmr_adam_hyper) == 32, "layout of the device table (whmr_amd/_lib.py mirrors it)");
static_assert(sizeof(whmr_adam_guard_cfg) == 16 && sizeof(whmr_adam_guard_state) == 32, "layout of the guard rows (whmr_amd/_lib.py mirrors it)");
static_assert(WHMR_ADAM_CHUNK == 16 * 256, "whmr_adam_grad_sumsq: <= 16 fp32 squares per thread (its error bound, and the tests' gate, count on it)");

struct adam_coef { float wd, omb1, b2, omb2, step_size, sqrt_bc2, eps; };

__device__ __forceinline__ adam_coef adam_coefficients(const whmr_adam_item& it, const whmr_adam_hyper* __restrict__ hyper) {
    const whmr_adam_hyper h = hyper[it.group];
    adam_coef c;
    c.wd = h.weight_decay;
    c.omb1 = (float)(1.0 - h.beta1);                 // 1 - beta rounded ONCE, as torch does on the host: 1.f - 0.999f is 4.7e-5 off 0.001
    c.b2 = (float)h.beta2;
    c.omb2 = (float)(1.0 - h.beta2);
    c.step_size = (float)(h.lr / it.bc1);            // torch: step_size = lr / bias_correction1 and bias_correction2 ** 0.5 as Python floats (doubles),
    c.sqrt_bc2 = (float)sqrt(it.bc2);                // each rounded to fp32 once where it meets the tensors
    c.eps = h.eps;
    return c;
}

// ONE element, one fixed sequence of fp32 roundings (no contraction left to the compiler): the flat and the tile path, vector or dword, give the
// same bits for the same element
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, const adam_coef& c) {
#pragma clang fp contract(off)
    if (c.wd != 0.f) g = fmaf(c.wd, p, g);
    m = fmaf(g - m, c.omb1, m);
    v = fmaf(c.b2, v, (c.omb2 * g) * g);
    const float denom = sqrtf(v) / c.sqrt_bc2 + c.eps;
    p = p - c.step_size * (m / denom);
}

// the gradient the update sees: g itself, or fp32(g * coef) -- the value torch's clip_grad_norm_ leaves in p.grad with its in-place mul_ (p.grad is
// NOT rewritten here).  A statement of its own, never contracted into adam_update's first operation.
template <bool GUARD> __device__ __forceinline__ float adam_grad(float g, float coef) {
#pragma clang fp contract(off)
    if (GUARD) g = g * coef;
    return g;
}

__device__ __forceinline__ int adam_find_item(const whmr_adam_item* __restrict__ items, int n_items, int block) {
    int lo = 0, hi = n_items - 1;                    // last item whose block_begin <= block
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid].block_begin <= block) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ bool aligned16(const void* a, const void* b, const void* c, const void* d) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

template <bool GUARD> __device__ __forceinline__ void adam_flat(const whmr_adam_item& it, const adam_coef& c, int chunk, float coef) {
    const int64_t start = (int64_t)chunk * WHMR_ADAM_CHUNK;
    if (start >= it.numel) return;
    const int n = (int)(it.numel - start < WHMR_ADAM_CHUNK ? it.numel - start : WHMR_ADAM_CHUNK);
    float* p = it.p + start;
    const float* g = it.g + start;
    float* m = it.m + start;
    float* v = it.v + start;
    const int t = threadIdx.x;
    if (aligned16(p, g, m, v)) {                      // the chunk starts 16 KiB into the item: the item's own alignment decides
        const int n4 = n >> 2;
        for (int i = t; i < n4; i += 256) {
            float4 P = ((float4*)p)[i], M = ((float4*)m)[i], V = ((float4*)v)[i];
            const float4 G = ((const float4*)g)[i];
            adam_update(P.x, adam_grad<GUARD>(G.x, coef), M.x, V.x, c);
            adam_update(P.y, adam_grad<GUARD>(G.y, coef), M.y, V.y, c);
            adam_update(P.z, adam_grad<GUARD>(G.z, coef), M.z, V.z, c);
            adam_update(P.w, adam_grad<GUARD>(G.w, coef), M.w, V.w, c);
            ((float4*)p)[i] = P; ((float4*)m)[i] = M; ((float4*)v)[i] = V;
        }
        const int i = (n4 << 2) + t;                  // ragged tail: at most 3 elements
        if (i < n) {
            float P = p[i], M = m[i], V = v[i];
            adam_update(P, adam_grad<GUARD>(g[i], coef), M, V, c);
            p[i] = P; m[i] = M; v[i] = V;
        }
    } else {
        for (int i = t; i < n; i += 256) {
            float P = p[i], M = m[i], V = v[i];
            adam_update(P, adam_grad<GUARD>(g[i], coef), M, V, c);
            p[i] = P; m[i] = M; v[i] = V;
        }
    }
}

// 64x64 tile of p [N, K]: update, bf16(p_new) to w [N, K] from the registers and to wt [K, N] through the LDS tile.  Indexing and rounding of the
// copies are weights_prepare_kernel's (train_ops.hip).
template <bool GUARD> __device__ __forceinline__ void adam_tile(const whmr_adam_item& it, const adam_coef& c, int tile_index, float (*tile)[65], float coef) {
    const int n0 = (tile_index / it.tiles_k) * 64, k0 = (tile_index % it.tiles_k) * 64;
    if (n0 >= it.N) return;                           // a block past the item's tiles (a table that disagrees with the grid): uniform, before any barrier
    bf16_t* w = (bf16_t*)it.w;
    bf16_t* wt = (bf16_t*)it.wt;
    if (!(it.K & 3) && aligned16(it.p, it.g, it.m, it.v) && !((uintptr_t)w & 7)) {
        // rows of K % 4 == 0 floats from 16-byte aligned bases: 16 lanes x 16 B per row, 16 rows per pass
        const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll 2
        for (int i = 0; i < 4; ++i) {
            const int r = ty + 16 * i, n = n0 + r, k = k0 + 4 * tx;
            float4 P = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n < it.N && k < it.K) {               // K % 4 == 0: the four columns are inside or outside together
                const size_t off = (size_t)n * it.K + k;
                P = *(const float4*)(it.p + off);
                float4 M = *(const float4*)(it.m + off), V = *(const float4*)(it.v + off);
                const float4 G = *(const float4*)(it.g + off);
                adam_update(P.x, adam_grad<GUARD>(G.x, coef), M.x, V.x, c);
                adam_update(P.y, adam_grad<GUARD>(G.y, coef), M.y, V.y, c);
                adam_update(P.z, adam_grad<GUARD>(G.z, coef), M.z, V.z, c);
                adam_update(P.w, adam_grad<GUARD>(G.w, coef), M.w, V.w, c);
                *(float4*)(it.p + off) = P; *(float4*)(it.m + off) = M; *(float4*)(it.v + off) = V;
                if (w) *(uint2*)(w + off) = make_uint2(pack_bf16x2(P.x, P.y), pack_bf16x2(P.z, P.w));
            }
            tile[r][4 * tx] = P.x; tile[r][4 * tx + 1] = P.y; tile[r][4 * tx + 2] = P.z; tile[r][4 * tx + 3] = P.w;
        }
    } else {
        const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;      // 64 columns x 4 rows per pass
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {
            const int r = ty + 4 * i, n = n0 + r, k = k0 + tx;
            float P = 0.f;
            if (n < it.N && k < it.K) {
                const size_t off = (size_t)n * it.K + k;
                P = it.p[off];
                float M = it.m[off], V = it.v[off];
                adam_update(P, adam_grad<GUARD>(it.g[off], coef), M, V, c);
                it.p[off] = P; it.m[off] = M; it.v[off] = V;
                if (w) w[off] = f32_to_bf16(P);
            }
            tile[r][tx] = P;
        }
    }
    __syncthreads();
    if (!wt) return;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
        const int k = k0 + ty + 4 * i, n = n0 + tx;
        if (k < it.K && n < it.N) wt[(size_t)k * it.N + n] = f32_to_bf16(tile[tx][ty + 4 * i]);
    }
}

// GUARD = false is whmr_adam_step as it always was (state unused); GUARD = true reads the guard's decision first
template <bool GUARD> __global__ __launch_bounds__(256) void adam_step_kernel(const whmr_adam_item* __restrict__ items, int n_items,
                                                                              const whmr_adam_hyper* __restrict__ hyper,
                                                                              const whmr_adam_guard_state* __restrict__ state) {
    __shared__ float tile[64][65];
    float coef = 1.f;
    if (GUARD) {                                      // read once per workgroup, uniform: a skipped step leaves before any barrier
        if (!state->apply) return;
        coef = state->clip_coef;
    }
    const whmr_adam_item it = items[adam_find_item(items, n_items, (int)blockIdx.x)];
    const adam_coef c = adam_coefficients(it, hyper);
    const int local = (int)blockIdx.x - it.block_begin;
    if (it.tiles_k > 0) adam_tile<GUARD>(it, c, local, tile, coef);
    else adam_flat<GUARD>(it, c, local, coef);
}

// step += 1 and the bias corrections of item i: the advance launch and the guard's single workgroup share it
__device__ __forceinline__ void adam_advance_item(whmr_adam_item* __restrict__ items, int i, const whmr_adam_hyper* __restrict__ hyper) {
    const whmr_adam_hyper h = hyper[items[i].group];
    float* step = items[i].step;
    const float t = *step + 1.f;
    *step = t;
    items[i].bc1 = 1.0 - pow(h.beta1, (double)t);
    items[i].bc2 = 1.0 - pow(h.beta2, (double)t);
}

__global__ __launch_bounds__(64) void adam_advance_kernel(whmr_adam_item* __restrict__ items, int n_items, const whmr_adam_hyper* __restrict__ hyper) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_items) return;
    adam_advance_item(items, i, hyper);
}

// sum of g^2 over chunk (blockIdx.x - block_begin) of the item's gradient, one double per workgroup
__global__ __launch_bounds__(256) void adam_grad_sumsq_kernel(const whmr_adam_item* __restrict__ items, int n_items, double* __restrict__ partials) {
    __shared__ double wave_sum[4];
    const whmr_adam_item it = items[adam_find_item(items, n_items, (int)blockIdx.x)];
    const int64_t start = (int64_t)((int)blockIdx.x - it.block_begin) * WHMR_ADAM_CHUNK;
    const int t = threadIdx.x;
    float acc = 0.f;                                  // <= 16 elements per thread on either path
    if (start < it.numel) {                           // else: a spare workgroup of a tile item (or a table that disagrees with the grid) writes 0.0
        const int n = (int)(it.numel - start < WHMR_ADAM_CHUNK ? it.numel - start : WHMR_ADAM_CHUNK);
        const float* g = it.g + start;
        if (((uintptr_t)g & 15) == 0) {
            const int n4 = n >> 2;
            for (int i = t; i < n4; i += 256) {
                const float4 G = ((const float4*)g)[i];
                acc += G.x * G.x; acc += G.y * G.y; acc += G.z * G.z; acc += G.w * G.w;
            }
            // ragged tail, at most 3 elements, given to the LAST threads: n4 < 1024 then, so they hold at most 3 vectors (12 elements)
            const int i = (n4 << 2) + (255 - t);
            if (i < n) acc += g[i] * g[i];
        } else {
            for (int i = t; i < n; i += 256) acc += g[i] * g[i];
        }
    }
    double s = (double)acc;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((t & 63) == 0) wave_sum[t >> 6] = s;
    __syncthreads();
    if (t == 0) partials[blockIdx.x] = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
}

__global__ __launch_bounds__(256) void adam_guard_advance_kernel(whmr_adam_item* __restrict__ items, int n_items, const whmr_adam_hyper* __restrict__ hyper,
                                                                 const double* __restrict__ partials, int total_blocks,
                                                                 const whmr_adam_guard_cfg* __restrict__ cfg, whmr_adam_guard_state* __restrict__ state) {
    __shared__ double red[256];
    __shared__ int apply_shared;
    const int t = threadIdx.x;
    double s = 0.0;
    for (int i = t; i < total_blocks; i += 256) s += partials[i];
    red[t] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    if (t == 0) {
        const float norm = (float)sqrt(red[0]);       // Inf where the sum (or a thread's fp32 share of it) overflowed, NaN where an element was NaN
        const bool finite = isfinite(norm);
        const int apply = (cfg->skip_nonfinite && !finite) ? 0 : 1;
        float coef = 1.f;
        if (cfg->max_norm > 0.0) {                    // torch: clamp(max_norm / (total_norm + 1e-6), max=1.0); a NaN coefficient stays NaN
            const double c = cfg->max_norm / ((double)norm + 1e-6);
            coef = (c < 1.0 || c != c) ? (float)c : 1.f;
        }
        state->grad_norm = norm;
        state->clip_coef = apply ? coef : 0.f;        // a skipped step applied nothing
        state->apply = apply;
        state->steps_seen += 1;
        if (!apply) state->steps_skipped += 1;
        apply_shared = apply;
    }
    __syncthreads();
    if (!apply_shared) return;                        // skipped: step counts and bias corrections stay, the next applied step is number t + 1
    for (int i = t; i < n_items; i += 256) adam_advance_item(items, i, hyper);
}

extern "C" int whmr_adam_advance(void* items, int n_items, const void* hyper, void* stream) {
    if (!items || !hyper || n_items <= 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(adam_advance_kernel, dim3((n_items + 63) / 64), dim3(64), 0, (hipStream_t)stream, (whmr_adam_item*)items, n_items,
                       (const whmr_adam_hyper*)hyper);
    WHMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int whmr_adam_step(const void* items, int n_items, int total_blocks, const void* hyper, void* stream) {
    if (!items || !hyper || n_items <= 0 || total_blocks <= 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(adam_step_kernel<false>, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, (const whmr_adam_item*)items, n_items,
                       (const whmr_adam_hyper*)hyper, (const whmr_adam_guard_state*)nullptr);
    WHMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int whmr_adam_grad_sumsq(const void* items, int n_items, int total_blocks, void* partials, void* stream) {
    if (!items || !partials || n_items <= 0 || total_blocks <= 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(adam_grad_sumsq_kernel, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, (const whmr_adam_item*)items, n_items,
                       (double*)partials);
    WHMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int whmr_adam_guard_advance(void* items, int n_items, const void* hyper, const void* partials, int total_blocks, const void* cfg,
                                       void* state, void* stream) {
    if (!items || !hyper || !partials || !cfg || !state || n_items <= 0 || total_blocks <= 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(adam_guard_advance_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (whmr_adam_item*)items, n_items,
                       (const whmr_adam_hyper*)hyper, (const double*)partials, total_blocks, (const whmr_adam_guard_cfg*)cfg,
                       (whmr_adam_guard_state*)state);
    WHMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int whmr_adam_step_guarded(const void* items, int n_items, int total_blocks, const void* hyper, const void* state, void* stream) {
    if (!items || !hyper || !state || n_items <= 0 || total_blocks <= 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(adam_step_kernel<true>, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, (const whmr_adam_item*)items, n_items,
                       (const whmr_adam_hyper*)hyper, (const whmr_adam_guard_state*)state);
    WHMR_CHECK_LAUNCH();
    return 0;
}

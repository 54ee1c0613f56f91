// Adam step of a whole model in two launches over a device-resident table (reference: torch.optim.Adam as core/trainer.py:615 steps it --
// non-amsgrad, L2 weight decay), capturable in a HIP graph: the step counts, the bias corrections and the hyper-parameters all live in device
// memory, so a replayed graph advances them and follows a learning rate the host changed between two replays.
//   whmr_adam_advance   one thread per parameter: step += 1, bias corrections 1 - beta^step (double precision) into the table
//   whmr_adam_step      one workgroup per 4096-element chunk ("flat" item) or per 64x64 tile ("tile" item: the fp32 matrices whose bf16 W / W^T
//                       operand copies the ViT's GEMMs read -- the update writes both copies from the registers and the LDS tile it already holds,
//                       which is the pass whmr_weights_prepare (train_ops.hip) would otherwise make over the weights after the step)
// Memory-bound (28 B per parameter): 16-byte accesses where the four pointers of an item allow them -- gradients may be views into GradReducer's
// flat buckets, which guarantee 4 bytes only -- and a dword path otherwise.  Built without packed-fp32 instructions (build.py: NO_PACKED_FP32).
#include "common.h"
#include "../../include/whmr_hip.h"

static_assert(sizeof(whmr_adam_item) == 104 && sizeof(whmr_adam_hyper) == 32, "layout of the device table (whmr_amd/_lib.py mirrors it)");

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

__device__ __forceinline__ void adam_flat(const whmr_adam_item& it, const adam_coef& c, int chunk) {
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
            adam_update(P.x, G.x, M.x, V.x, c);
            adam_update(P.y, G.y, M.y, V.y, c);
            adam_update(P.z, G.z, M.z, V.z, c);
            adam_update(P.w, G.w, M.w, V.w, c);
            ((float4*)p)[i] = P; ((float4*)m)[i] = M; ((float4*)v)[i] = V;
        }
        const int i = (n4 << 2) + t;                  // ragged tail: at most 3 elements
        if (i < n) {
            float P = p[i], M = m[i], V = v[i];
            adam_update(P, g[i], M, V, c);
            p[i] = P; m[i] = M; v[i] = V;
        }
    } else {
        for (int i = t; i < n; i += 256) {
            float P = p[i], M = m[i], V = v[i];
            adam_update(P, g[i], M, V, c);
            p[i] = P; m[i] = M; v[i] = V;
        }
    }
}

// 64x64 tile of p [N, K]: update, bf16(p_new) to w [N, K] from the registers and to wt [K, N] through the LDS tile.  Indexing and rounding of the
// copies are weights_prepare_kernel's (train_ops.hip).
__device__ __forceinline__ void adam_tile(const whmr_adam_item& it, const adam_coef& c, int tile_index, float (*tile)[65]) {
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
                adam_update(P.x, G.x, M.x, V.x, c);
                adam_update(P.y, G.y, M.y, V.y, c);
                adam_update(P.z, G.z, M.z, V.z, c);
                adam_update(P.w, G.w, M.w, V.w, c);
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
                adam_update(P, it.g[off], M, V, c);
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

__global__ __launch_bounds__(256) void adam_step_kernel(const whmr_adam_item* __restrict__ items, int n_items,
                                                        const whmr_adam_hyper* __restrict__ hyper) {
    __shared__ float tile[64][65];
    const whmr_adam_item it = items[adam_find_item(items, n_items, (int)blockIdx.x)];
    const adam_coef c = adam_coefficients(it, hyper);
    const int local = (int)blockIdx.x - it.block_begin;
    if (it.tiles_k > 0) adam_tile(it, c, local, tile);
    else adam_flat(it, c, local);
}

__global__ __launch_bounds__(64) void adam_advance_kernel(whmr_adam_item* __restrict__ items, int n_items, const whmr_adam_hyper* __restrict__ hyper) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_items) return;
    const whmr_adam_hyper h = hyper[items[i].group];
    float* step = items[i].step;
    const float t = *step + 1.f;
    *step = t;
    items[i].bc1 = 1.0 - pow(h.beta1, (double)t);
    items[i].bc2 = 1.0 - pow(h.beta2, (double)t);
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
    hipLaunchKernelGGL(adam_step_kernel, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, (const whmr_adam_item*)items, n_items,
                       (const whmr_adam_hyper*)hyper);
    WHMR_CHECK_LAUNCH();
    return 0;
}

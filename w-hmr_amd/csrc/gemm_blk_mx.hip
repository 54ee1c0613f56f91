// MXFP8 GEMM of the MX pilot of the ViT inference path (ViT.mx_pilot, off by default): out = epi(deq(A) . deq(W)^T + bias [+ res]) on
// v_mfma_scale_f32_32x32x64_f8f6f4 with e4m3 operands and fp32 accumulation, plus the quantiser that makes its operands (whmr_quantize_mx).
// Number format and layouts: mx_common.h.
//
// Fragment maps of the scaled 32x32x64 MFMA with e4m3 operands (measured with exact integer data and one-hot operands, tests/test_mxfp8_gpu.py): lane
// l = (r = l & 31, h = l >> 5) holds 32 bytes of row r of an operand's 32-row block; bytes 16 v .. 16 v + 15 (VGPRs 4 v .. 4 v + 3) are k = 32 v + 16 h
// .. + 15 of the 64-deep sub-step, and the scale byte of lane (r, h) applies to the 32-block k = 32 h .. 32 h + 31 -- i.e. scale block b is bytes 16 b ..
// of BOTH lane halves, not the 32 bytes of one lane.  So lane h loads the 16-byte units 4 sub + h and 4 sub + 2 + h of the 128-deep K step (the first
// halves of MX blocks 2 sub and 2 sub + 1 for h = 0, the second halves for h = 1) and supplies the scale of block 2 sub + h.  W is the FIRST operand
// and A the second, so D[row = n][col = m]: a lane owns row m = r of its A block and the 16 columns n = 8 q + 4 h + t (register 4 q + t) of a
// 32-column W block -- the epilogues store straight from the accumulators.
//
// Tile: 4 waves (2 x 2), wave tile (32 MI) x (32 NI), one 128-deep K step per iteration through a double-buffered LDS image of the stage.  A stage of
// one 32-row block is 8 consecutive 512-B units = 4 KiB contiguous in global memory, so thread t copies 16 B of every row block of the stage (256
// threads x 16 B = 4 KiB) and the image is linear: the fragment reads (lanes 0-15 = 256 contiguous bytes) are conflict-free without a swizzle.
// Scales go straight from global memory to registers, one dword per lane and row block per K step, a step ahead.
#include <type_traits>
#include "mx_common.h"

struct whmr_gemm_blk_mx_desc {
    const void* A;        // e4m3 [ceil(M/32)][K/16][32][16]
    const void* A_scale;  // e8m0 [ceil(M/32)][K/128][32][4]
    const void* W;        // e4m3 [N/32][K/16][32][16]           (nn.Linear weight [N, K], quantised once)
    const void* W_scale;  // e8m0 [N/32][K/128][32][4]
    void* C;              // epi 0: bf16 [ceil(M/32)][N/8][32][8];  epi 1: e4m3 [ceil(M/32)][N/16][32][16];  epi 2: fp32 [ceil(M/32)][N/4][32][4]
    void* C_scale;        // epi 1: e8m0 [ceil(M/32)][N/128][32][4]
    const float* bias;    // [N] or null
    const float* res;     // epi 2: fp32 blocked like C (may alias C)
    int32_t M, N, K;      // N % 128 == 0, K % 128 == 0; buffers hold whole 32-row blocks
    int32_t epi;          // 0: bf16(acc + bias)   1: MX(gelu(acc + bias))   2: fp32(acc + bias + res)
    int32_t tile;         // 0 = chooser; 0x42: 256 x 128, 0x22: 128 x 128
    int32_t reserved;
};

typedef __attribute__((ext_vector_type(8))) int i32x8_t;
typedef __attribute__((ext_vector_type(4))) int i32x4_t;

template <int MI, int NI>
struct mx_cfg {
    static constexpr int MB = 2 * MI, NB = 2 * NI;        // A / W row blocks per tile
    static constexpr int BM = 32 * MB, BN = 32 * NB;
    static constexpr int STAGE = (MB + NB) * 4096;       // one 128-deep K step of every row block
    static constexpr int LDS = 2 * STAGE;
};

template <int MI, int NI, int EPI>
__global__ __launch_bounds__(256) void gemm_blk_mx_kernel(const whmr_gemm_blk_mx_desc p) {
    using cfg = mx_cfg<MI, NI>;
    constexpr int MB = cfg::MB, NB = cfg::NB, BM = cfg::BM, BN = cfg::BN, STAGE = cfg::STAGE;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int r = lane & 31, h = lane >> 5;
    const int tiles_n = p.N / BN, tiles_m = (p.M + BM - 1) / BM;
    const int lid = xcd_remap(blockIdx.x, tiles_m * tiles_n);
    const int tm = lid / tiles_n, tn = lid % tiles_n;
    const int rb0 = tm * MB, nb0 = tn * NB;               // first A / W row block of the tile
    const int rb_last = ((p.M + 31) >> 5) - 1;
    const int KS = p.K >> 7;                              // 128-deep K steps
    const size_t rbytes = (size_t)p.K * 32;               // operand bytes of one 32-row block

    const char* src[MB + NB];
#pragma unroll
    for (int i = 0; i < MB; ++i) {
        const int rb = rb0 + i > rb_last ? rb_last : rb0 + i;         // M tail: re-read the last block (its results are not stored)
        src[i] = (const char*)p.A + rb * rbytes + tid * 16;
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) src[MB + j] = (const char*)p.W + (nb0 + j) * rbytes + tid * 16;
    const uint32_t* sa_src[MI];
    const uint32_t* sw_src[NI];
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        int rb = rb0 + wm * MI + i;
        if (rb > rb_last) rb = rb_last;
        sa_src[i] = (const uint32_t*)p.A_scale + (size_t)rb * KS * 32 + r;
    }
#pragma unroll
    for (int j = 0; j < NI; ++j) sw_src[j] = (const uint32_t*)p.W_scale + (size_t)(nb0 + wn * NI + j) * KS * 32 + r;

    i32x4_t stg[MB + NB];
    uint32_t sa[MI], sw[NI], sa_n[MI], sw_n[NI];
    auto gload = [&](int ks) {
#pragma unroll
        for (int i = 0; i < MB + NB; ++i) stg[i] = *(const i32x4_t*)(src[i] + (size_t)ks * 4096);
#pragma unroll
        for (int i = 0; i < MI; ++i) sa_n[i] = sa_src[i][ks * 32];
#pragma unroll
        for (int j = 0; j < NI; ++j) sw_n[j] = sw_src[j][ks * 32];
    };
    auto sstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < MB + NB; ++i) *(i32x4_t*)(smem + buf * STAGE + i * 4096 + tid * 16) = stg[i];
#pragma unroll
        for (int i = 0; i < MI; ++i) sa[i] = sa_n[i] >> (8 * h);       // byte 2 sub + h of the step's dword -> byte 2 sub (op_sel below)
#pragma unroll
        for (int j = 0; j < NI; ++j) sw[j] = sw_n[j] >> (8 * h);
    };

    f32x16_t acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    gload(0);
    sstore(0);
    __syncthreads();
    for (int ks = 0; ks < KS; ++ks) {
        const int buf = ks & 1;
        uint32_t ca[MI], cw[NI];
#pragma unroll
        for (int i = 0; i < MI; ++i) ca[i] = sa[i];
#pragma unroll
        for (int j = 0; j < NI; ++j) cw[j] = sw[j];
        if (ks + 1 < KS) gload(ks + 1);
        const char* sb = smem + buf * STAGE + h * 512 + r * 16;
        auto step = [&](auto sub_tag) {
            constexpr int sub = decltype(sub_tag)::value;                 // 64-deep sub-step: MX blocks 2 sub and 2 sub + 1 of the K step
            i32x8_t fa[MI], fw[NI];
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                const char* q = sb + (wm * MI + i) * 4096 + sub * 2048;
                fa[i] = __builtin_shufflevector(*(const i32x4_t*)q, *(const i32x4_t*)(q + 1024), 0, 1, 2, 3, 4, 5, 6, 7);
            }
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                const char* q = sb + (MB + wn * NI + j) * 4096 + sub * 2048;
                fw[j] = __builtin_shufflevector(*(const i32x4_t*)q, *(const i32x4_t*)(q + 1024), 0, 1, 2, 3, 4, 5, 6, 7);
            }
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fw[j], fa[i], acc[i][j], 0, 0, 2 * sub, (int)cw[j], 2 * sub, (int)ca[i]);
        };
        step(std::integral_constant<int, 0>());
        step(std::integral_constant<int, 1>());
        if (ks + 1 < KS) sstore(buf ^ 1);
        __syncthreads();
    }

    // ---- epilogue: lane owns row r of A block rb and columns 32 nblk + 8 q + 4 h + t (accumulator register 4 q + t)
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        const int rb = rb0 + wm * MI + i;
        if (rb > rb_last) continue;
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int nblk = nb0 + wn * NI + j;
            float v[16];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 b = p.bias ? *(const float4*)(p.bias + 32 * nblk + 8 * q + 4 * h) : make_float4(0.f, 0.f, 0.f, 0.f);
                v[4 * q + 0] = acc[i][j][4 * q + 0] + b.x;
                v[4 * q + 1] = acc[i][j][4 * q + 1] + b.y;
                v[4 * q + 2] = acc[i][j][4 * q + 2] + b.z;
                v[4 * q + 3] = acc[i][j][4 * q + 3] + b.w;
            }
            if constexpr (EPI == 2) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const size_t off = (((size_t)rb * (p.N >> 2) + nblk * 8 + 2 * q + h) * 32 + r) * 4;
                    const float4 rs = *(const float4*)(p.res + off);
                    *(float4*)((float*)p.C + off) = make_float4(v[4 * q] + rs.x, v[4 * q + 1] + rs.y, v[4 * q + 2] + rs.z, v[4 * q + 3] + rs.w);
                }
            } else if constexpr (EPI == 0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    char* unitp = (char*)p.C + (((size_t)rb * (p.N >> 3) + nblk * 4 + q) * 32 + r) * 16 + 8 * h;
                    *(uint2*)unitp = make_uint2(pack_bf16x2(v[4 * q], v[4 * q + 1]), pack_bf16x2(v[4 * q + 2], v[4 * q + 3]));
                }
            } else {
                // GELU (the bf16 epilogue's form), then the row's 32-column block -> one MX block: the 16 values of this lane and the 16 of lane l ^ 32
                float amax = 0.f;
#pragma unroll
                for (int e = 0; e < 16; e += 2) {
                    const f32x2_t g = gelu_fast2(f32x2_t{v[e], v[e + 1]});
                    v[e] = g.x; v[e + 1] = g.y;
                    amax = fmaxf(amax, fmaxf(fabsf(g.x), fabsf(g.y)));
                }
                amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
                const int ex = mx_scale_exp(amax);
                const float inv = mx_inv_scale(ex);
                uint32_t w[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) w[q] = mx_pack4(v[4 * q] * inv, v[4 * q + 1] * inv, v[4 * q + 2] * inv, v[4 * q + 3] * inv);
                // 16-byte row c of the block holds columns 16 c .. 16 c + 15 = words q = 2 c (bytes 0-7) and 2 c + 1 (bytes 8-15), each split over the
                // lane pair (h = 0: its first 4 bytes, h = 1: the next 4).  Lane h stores bytes 8 h .. 8 h + 7 = word q = 2 c + h of both lanes.
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const uint32_t mine = w[2 * c + h], other = __shfl_xor(w[2 * c + 1 - h], 32, 64);
                    char* unitp = (char*)p.C + (((size_t)rb * (p.N >> 4) + nblk * 2 + c) * 32 + r) * 16 + 8 * h;
                    *(uint2*)unitp = h ? make_uint2(other, mine) : make_uint2(mine, other);
                }
                if (h == 0) ((uint8_t*)p.C_scale)[(((size_t)rb * (p.N >> 7) + (nblk >> 2)) * 32 + r) * 4 + (nblk & 3)] = (uint8_t)(ex + 127);
            }
        }
    }
}

template <int MI, int NI, int EPI>
static int launch_mx(const whmr_gemm_blk_mx_desc& p, hipStream_t st) {
    using cfg = mx_cfg<MI, NI>;
    auto kern = gemm_blk_mx_kernel<MI, NI, EPI>;
    static bool attr_done = false;
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, cfg::LDS);
        if (e != hipSuccess) return (int)e;
        attr_done = true;
    }
    const int tiles = ((p.M + cfg::BM - 1) / cfg::BM) * (p.N / cfg::BN);
    hipLaunchKernelGGL(kern, dim3(tiles), dim3(256), cfg::LDS, st, p);
    WHMR_CHECK_LAUNCH();
    return 0;
}

template <int MI, int NI>
static int launch_mx_epi(const whmr_gemm_blk_mx_desc& p, hipStream_t st) {
    switch (p.epi) {
        case 0: return launch_mx<MI, NI, 0>(p, st);
        case 1: return launch_mx<MI, NI, 1>(p, st);
        case 2: return launch_mx<MI, NI, 2>(p, st);
    }
    return (int)hipErrorInvalidValue;
}

extern "C" int whmr_gemm_blk_mx(const whmr_gemm_blk_mx_desc* pp, void* stream) {
    const whmr_gemm_blk_mx_desc& p = *pp;
    if (!p.A || !p.A_scale || !p.W || !p.W_scale || !p.C || p.M <= 0 || p.N <= 0 || (p.N % 128) || p.K <= 0 || (p.K % 128) || p.epi < 0 || p.epi > 2)
        return (int)hipErrorInvalidValue;
    if ((p.epi == 2 && !p.res) || (p.epi == 1 && !p.C_scale)) return (int)hipErrorInvalidValue;
    int tile = p.tile;
    if (!tile) {
        // 256 x 128 (one workgroup per CU: 96 KiB of LDS) once it fills two rounds of the 256 CUs; below that the 128 x 128 tile (two per CU) spreads
        // the work over more CUs (ViT-B 224^2 batch 64: proj / fc2 294 big tiles would leave most of a second round idle)
        const long big = (long)((p.M + 255) / 256) * (p.N / 128);
        tile = big >= 512 ? 0x42 : 0x22;
    }
    const hipStream_t st = (hipStream_t)stream;
    switch (tile) {
        case 0x42: return launch_mx_epi<4, 2>(p, st);     // 256 x 128
        case 0x22: return launch_mx_epi<2, 2>(p, st);     // 128 x 128
    }
    return (int)hipErrorInvalidValue;
}

// ---- quantiser: one thread per (row, 32-element block), threads of a row block consecutive in the row -> the 16-B stores of a unit are one 512-B run
__global__ __launch_bounds__(256) void quantize_mx_kernel(const void* __restrict__ src, int kind, uint8_t* __restrict__ q, uint8_t* __restrict__ s, int R,
                                                          int K, long total) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int r = (int)(t & 31);
    const long u = t >> 5;
    const int KB = K >> 5;
    const int kb = (int)(u % KB);
    const long rb = u / KB;
    const long row = rb * 32 + r;
    float x[32];
    if (row >= R) {
#pragma unroll
        for (int e = 0; e < 32; ++e) x[e] = 0.f;
    } else if (kind == 0) {
        const float4* p4 = (const float4*)((const float*)src + row * K + kb * 32);
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float4 v = p4[e]; x[4 * e] = v.x; x[4 * e + 1] = v.y; x[4 * e + 2] = v.z; x[4 * e + 3] = v.w; }
    } else {
        uint4 raw[4];
        if (kind == 1) {
            const uint4* p4 = (const uint4*)((const bf16_t*)src + row * K + kb * 32);
#pragma unroll
            for (int e = 0; e < 4; ++e) raw[e] = p4[e];
        } else {                                           // blocked bf16 [R/32][K/8][32][8]: units 4 kb .. 4 kb + 3 of row r
#pragma unroll
            for (int e = 0; e < 4; ++e) raw[e] = *(const uint4*)((const char*)src + ((rb * (K >> 3) + kb * 4 + e) * 32 + r) * 16);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t w[4] = {raw[e].x, raw[e].y, raw[e].z, raw[e].w};
#pragma unroll
            for (int f = 0; f < 4; ++f) { x[8 * e + 2 * f] = __uint_as_float(w[f] << 16); x[8 * e + 2 * f + 1] = __uint_as_float(w[f] & 0xffff0000u); }
        }
    }
    float amax = 0.f;
#pragma unroll
    for (int e = 0; e < 32; ++e) amax = fmaxf(amax, fabsf(x[e]));
    const int ex = mx_scale_exp(amax);
    const float inv = mx_inv_scale(ex);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        uint4 o;
        o.x = mx_pack4(x[16 * c] * inv, x[16 * c + 1] * inv, x[16 * c + 2] * inv, x[16 * c + 3] * inv);
        o.y = mx_pack4(x[16 * c + 4] * inv, x[16 * c + 5] * inv, x[16 * c + 6] * inv, x[16 * c + 7] * inv);
        o.z = mx_pack4(x[16 * c + 8] * inv, x[16 * c + 9] * inv, x[16 * c + 10] * inv, x[16 * c + 11] * inv);
        o.w = mx_pack4(x[16 * c + 12] * inv, x[16 * c + 13] * inv, x[16 * c + 14] * inv, x[16 * c + 15] * inv);
        *(uint4*)(q + ((rb * (K >> 4) + kb * 2 + c) * 32 + r) * 16) = o;
    }
    s[((rb * (K >> 7) + (kb >> 2)) * 32 + r) * 4 + (kb & 3)] = (uint8_t)(ex + 127);
}

extern "C" int whmr_quantize_mx(const void* src, int kind, void* q, void* s, int R, int K, void* stream) {
    if (!src || !q || !s || R <= 0 || K <= 0 || (K % 128) || kind < 0 || kind > 2) return (int)hipErrorInvalidValue;
    const long total = (long)((R + 31) / 32) * 32 * (K / 32);
    hipLaunchKernelGGL(quantize_mx_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, kind, (uint8_t*)q, (uint8_t*)s, R, K,
                       total);
    WHMR_CHECK_LAUNCH();
    return 0;
}

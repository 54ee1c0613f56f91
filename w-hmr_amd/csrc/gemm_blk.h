// Descriptor of the blocked-layout GEMM (gemm_blk.hip; mirrors `struct whmr_gemm_blk_desc` in include/whmr_hip.h) and what its two kernels
// share: the tile configuration, the counted waits and hidden fragment reads, and the tile / epilogue dispatch of the launchers.  Only
// gemm_blk16_impl.h (bf16, 16x16x32) and gemm_blk_impl.h (split-bf16, 32x32x16) include it.
#pragma once
#include <stdint.h>
#include <type_traits>
#include "common.h"

struct whmr_gemm_blk_desc {
    const void* A;        // bf16 blocked [ceil(M/32)][K/8][32][8]
    const void* W;        // bf16 blocked [N/32][K/8][32][8]      (nn.Linear weight [N, K], re-packed once)
    void* C;              // epi 0/1: bf16 blocked [ceil(M/32)][N/8][32][8];  epi 2/3: fp32 blocked [ceil(M/32)][N/4][32][4]
    const float* bias;    // [N] or null
    const float* res;     // epi 2: fp32 blocked like C (may alias C);  epi 3: row-major [res_rows, N], row = m % res_rows
    int32_t M, N, K;      // N % 256 == 0, K % 32 == 0; buffers hold whole 32-row blocks
    int32_t epi;          // 0: bf16(acc + bias)   1: bf16(gelu(acc + bias))   2 / 3: fp32(acc + bias + res)
    int32_t res_rows;
    int32_t tile;         // 0 = chooser; else (MI0 << 4) | MI1: 0x44 256 rows, 0x55 320, 0x43 224, 0x33 192, 0x32 160, 0x22 128, 0x54 288, 0x21 96
    // ---- LayerNorm folding (vit.py:125,133: the LayerNorm in front of qkv / fc1 never runs as its own pass) ---------------------------
    // producer (epi 2 / 3, xhat != null): besides the fp32 stream C it writes xhat = bf16(C) in the blocked operand layout and, per row and
    //   256-column tile, the partial sums (sum x, sum x^2) of the values it stored: stats_out [rows][N/256][2] fp32 (N <= 1024).
    // consumer (epi 0 / 1, stats_in != null): A = xhat of the raw stream, W = bf16(gamma o W) packed, bias = b + W.beta, colsum[n] = sum_k W'[n,k];
    //   out = rstd[m] * (acc - mean[m] * colsum[n]) + bias[n], mean / rstd of row m from its K/256 partial pairs (fixed summation order).
    void* xhat;
    float* stats_out;
    const float* stats_in;
    const float* colsum;
    float ln_eps;
    // ---- split-bf16 operands ("bf16x3", gemm_blk_x3.hip): x = x_hi + x_lo, three MFMAs per product.  A_lo / W_lo: the lo halves of A / W (same
    // layout); C_lo: lo half of a bf16 result (epi 0 / 1; epi 1 then applies the erf GELU to fp32 accuracy, common.h gelu_as).  All null = plain bf16 operands.
    const void* A_lo;
    const void* W_lo;
    void* C_lo;
    // ---- per-row shift of a folding producer (xhat != null): xhat and stats_out are taken of (C - s_m) with
    //   s_m = (shift ? shift[m] : 0) + (shift_stats ? mean of row m from shift_stats [rows][N/256][2] : 0);   shift_out[m] = s_m when non-null.
    // The consumer formula is unchanged (LayerNorm is shift-invariant); shift_stats must not alias stats_out.
    const float* shift;
    const float* shift_stats;
    float* shift_out;
    void* xhat_lo;        // split-bf16 producer (A_lo set, xhat set): lo half of the centred-row operand pair
};

typedef __attribute__((address_space(3))) void lds_void_t;
typedef const __attribute__((address_space(1))) void gbl_void_t;

template <int N> __device__ __forceinline__ void blk_wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
template <int N> __device__ __forceinline__ void blk_wait_lgkmcnt() { asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory"); }
// fragment read hidden from hipcc's waitcnt bookkeeping (valid after the counted wait + sched_barrier that follows it)
template <int OFF> __device__ __forceinline__ bf16x8_t blk_lds_read128(uint32_t addr) {
    bf16x8_t v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
    return v;
}

// 8 bias floats at addr and the 8 colsum floats 1 KiB behind them, read and waited for in one statement the compiler's waitcnt bookkeeping does not see
// (without a fold the colsum half was never written: the caller discards it)
__device__ __forceinline__ void blk_lds_read_bias(uint32_t addr, float4 (&bq)[2], float4 (&cq)[2]) {
    asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:16\n\tds_read_b128 %2, %4 offset:1024\n\tds_read_b128 %3, %4 offset:1040\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(bq[0]), "=&v"(bq[1]), "=&v"(cq[0]), "=&v"(cq[1]) : "v"(addr) : "memory");
}

// the same value, opaque to the compiler: what is computed from it is computed where it is used, not in front of the loop around it
__device__ __forceinline__ int blk_per_tile(int v) { asm volatile("" : "+v"(v)); return v; }

// A tile is (MI0 + MI1) row blocks x 256 columns on 8 waves: wave row 0 owns MI0 row blocks, wave row 1 owns MI1.
template <int MI0, int MI1>
struct blk_cfg {
    static constexpr int MB = MI0 + MI1;                 // A row blocks (32 rows) per tile
    static constexpr int BM = MB * 32, BN = 256;
    static constexpr int SLOT = (MB + 8) * 2048;         // one half K tile (32 deep) of A and W: 2 KiB per row block
    static constexpr int HU = (MB + 8) * 2;              // 1-KiB DMA units per half tile
    static constexpr int HUPW = (HU + 7) / 8;            // units per wave (waves >= HU % 8 issue one less when HU % 8 != 0)
    static constexpr int BIAS_OFF = 4 * SLOT;            // [256] floats behind the ring, then [256] floats of the LayerNorm-fold column sums
    static constexpr int STAT_OFF = BIAS_OFF + 2048;     // LayerNorm folding: [BM][4][2] floats -- row statistics (consumer) / per-wave-column partial sums (producer)
    static constexpr int LDS = 4 * SLOT + 2048 + BM * 32;
    static constexpr int MIMAX = MI0 > MI1 ? MI0 : MI1;
};

// Launcher dispatch: f(MI0, MI1) of the tile id / f(EPI) of the epilogue, each argument a std::integral_constant.
template <int V> using blk_int = std::integral_constant<int, V>;
template <class F>
static int blk_dispatch_tile(int tile, F&& f) {
    switch (tile) {
        case 0x44: return f(blk_int<4>{}, blk_int<4>{});      // 256 x 256
        case 0x55: return f(blk_int<5>{}, blk_int<5>{});      // 320 x 256
        case 0x43: return f(blk_int<4>{}, blk_int<3>{});      // 224 x 256
        case 0x33: return f(blk_int<3>{}, blk_int<3>{});      // 192 x 256
        case 0x32: return f(blk_int<3>{}, blk_int<2>{});      // 160 x 256
        case 0x22: return f(blk_int<2>{}, blk_int<2>{});      // 128 x 256
        case 0x54: return f(blk_int<5>{}, blk_int<4>{});      // 288 x 256
        case 0x21: return f(blk_int<2>{}, blk_int<1>{});      // 96 x 256: ViT-L at 32 crops (6144 tokens) x N = 1024 is exactly 256 such tiles
    }
    return (int)hipErrorInvalidValue;
}
template <class F>
static int blk_dispatch_epi(int epi, F&& f) {
    switch (epi) {
        case 0: return f(blk_int<0>{});
        case 1: return f(blk_int<1>{});
        case 2: return f(blk_int<2>{});
        case 3: return f(blk_int<3>{});
    }
    return (int)hipErrorInvalidValue;
}

// split-operand launcher (gemm_blk_x3.hip; library-internal), reached through whmr_gemm_blk / whmr_gemm_blk_tile when the descriptor carries lo halves
__attribute__((visibility("hidden"))) int blk_x3_launch_tile(const whmr_gemm_blk_desc* pp, int tile, void* stream);

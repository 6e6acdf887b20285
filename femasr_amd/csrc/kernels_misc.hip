// kernels_misc.hip — the HBM-bound / small kernels of the hot path (everything that is not a
// dense contraction): layout+pad, crop, GroupNorm moments, LayerNorm moments, 8x8 window
// attention, VQ row norms / argmin finalize / gather, weight repack.
// Reduction orders follow DESIGN.md "Arithmetic specification" (== the oracle's), so every
// kernel here is bit-reproducible and bit-identical to the CPU restatement.
#include "common.h"
#include "detmath.h"
#include <stdlib.h>
#include <string.h>
#include <type_traits>

namespace {

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }

// bijective XCD remap (block b runs on XCD b % 8): consecutive logical indices share an XCD
__device__ __forceinline__ int xcd_remap_misc(int bid, int nblk)
{
    const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7, within = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + within;
}

// ------------------------------------------------------------------------------------------
// pad / crop (femasr_arch.py:454-465)
// ------------------------------------------------------------------------------------------
// one thread per output element of NHWC (B,Hp,Wp,C); mirror: padded row H+i <- row H-1-i.
__global__ void pad_nchw_to_nhwc_kernel(const float *__restrict__ in, int B, int C, int H, int W, int Hp, int Wp,
                                        float *__restrict__ out, size_t total)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        size_t r = i / C;
        const int x = (int)(r % Wp);
        r /= Wp;
        const int y = (int)(r % Hp);
        const int n = (int)(r / Hp);
        const int sy = y < H ? y : 2 * H - 1 - y, sx = x < W ? x : 2 * W - 1 - x;
        out[i] = in[(((size_t)n * C + c) * H + sy) * W + sx];
    }
}

// femasr_forward_u8: the image decode arithmetic fused into the pad - uint8 HWC (B,H,W,3) -> (float)u8 / 255.0f (img2tensor + `/255.`,
// img_util.py:9-35, inference_femasr.py:55) mirrored to NHWC (B,Hp,Wp,3); swap_rb = the cv2 BGR order
__global__ void pad_u8hwc_to_nhwc_kernel(const unsigned char *__restrict__ in, int B, int H, int W, int swap_rb, int Hp, int Wp,
                                         float *__restrict__ out, size_t total)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % 3);
        size_t r = i / 3;
        const int x = (int)(r % Wp);
        r /= Wp;
        const int y = (int)(r % Hp);
        const int n = (int)(r / Hp);
        const int sy = y < H ? y : 2 * H - 1 - y, sx = x < W ? x : 2 * W - 1 - x;
        out[i] = (float)in[(((size_t)n * H + sy) * W + sx) * 3 + (swap_rb ? 2 - c : c)] / 255.0f;
    }
}

// ... and tensor2img (img_util.py:38-94) fused into the crop: NHWC (B,Hs,Ws,3) -> clamp [0,1], x255, round half to even -> uint8 HWC (B,Hc,Wc,3)
__global__ void crop_nhwc_to_u8hwc_kernel(const float *__restrict__ in, int B, int Hs, int Ws, int Hc, int Wc, int swap_rb,
                                          unsigned char *__restrict__ out, size_t total)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % 3);
        size_t r = i / 3;
        const int x = (int)(r % Wc);
        r /= Wc;
        const int y = (int)(r % Hc);
        const int n = (int)(r / Hc);
        float v = in[(((size_t)n * Hs + y) * Ws + x) * 3 + (swap_rb ? 2 - c : c)];
        v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
        if (!(v == v)) v = 0.f;
        out[i] = (unsigned char)rintf(v * 255.0f);
    }
}

// one thread per output element of NCHW (B,C,Hc,Wc)
__global__ void crop_nhwc_to_nchw_kernel(const float *__restrict__ in, int B, int Hs, int Ws, int C, int Hc, int Wc,
                                         float *__restrict__ out, size_t total)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % Wc);
        size_t r = i / Wc;
        const int y = (int)(r % Hc);
        r /= Hc;
        const int c = (int)(r % C);
        const int n = (int)(r / C);
        out[i] = in[(((size_t)n * Hs + y) * Ws + x) * C + c];
    }
}

// ------------------------------------------------------------------------------------------
// GroupNorm moments (fema_utils.py:22), two fixed-order fp64 levels
// ------------------------------------------------------------------------------------------
// level 1: thread (n, y, g) sums row y of group g: x ascending, channel-in-group ascending.
template <int CG>
__global__ void gn_rows_kernel(const float *__restrict__ x, int B, int H, int W, int C, int G, double *__restrict__ part)
{
    const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t total = (size_t)B * H * G;
    if (tid >= total) return;
    const int g = (int)(tid % G);
    const size_t ny = tid / G;   // n*H + y
    const float *row = x + ny * (size_t)W * C + g * CG;
    double s = 0.0, ss = 0.0;
    for (int xx = 0; xx < W; ++xx) {
        float v[CG];
        if constexpr (CG == 8) {
            const float4 a = ld4(row + (size_t)xx * C), b = ld4(row + (size_t)xx * C + 4);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
            v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        } else if constexpr (CG == 4) {
            const float4 a = ld4(row + (size_t)xx * C);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        } else {
#pragma unroll
            for (int j = 0; j < CG; ++j) v[j] = row[(size_t)xx * C + j];
        }
#pragma unroll
        for (int j = 0; j < CG; ++j) {
            const double d = (double)v[j];
            s = s + d;
            ss = ss + d * d;
        }
    }
    part[tid * 2] = s;
    part[tid * 2 + 1] = ss;
}

// generic channel-per-group fallback (runtime cg)
__global__ void gn_rows_generic_kernel(const float *__restrict__ x, int B, int H, int W, int C, int G, int cg,
                                       double *__restrict__ part)
{
    const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t total = (size_t)B * H * G;
    if (tid >= total) return;
    const int g = (int)(tid % G);
    const size_t ny = tid / G;
    const float *row = x + ny * (size_t)W * C + g * cg;
    double s = 0.0, ss = 0.0;
    for (int xx = 0; xx < W; ++xx)
        for (int j = 0; j < cg; ++j) {
            const double d = (double)row[(size_t)xx * C + j];
            s = s + d;
            ss = ss + d * d;
        }
    part[tid * 2] = s;
    part[tid * 2 + 1] = ss;
}

// level 2: one block per sample; the (H x G x 2) fp64 row partials are streamed through LDS in coalesced
// 64-row slabs and thread g adds its group's rows in ascending y (the specified order), then folds the moments
// into a[n,c], b[n,c].
constexpr int GN_SLAB = 64;
__global__ __launch_bounds__(256) void gn_finalize_kernel(const double *__restrict__ part, int B, int rows_total, int H, int W, int C, int G,
                                                          const float *__restrict__ gamma, const float *__restrict__ beta,
                                                          float eps, float *__restrict__ a, float *__restrict__ b)
{
    extern __shared__ __attribute__((aligned(16))) double slab[];      // [GN_SLAB][G][2]
    const int n = blockIdx.x, t = threadIdx.x, cg = C / G;
    const double *src = part + (size_t)n * rows_total * G * 2;
    double S = 0.0, SS = 0.0;
    for (int y0 = 0; y0 < rows_total; y0 += GN_SLAB) {
        const int rows = (rows_total - y0) < GN_SLAB ? (rows_total - y0) : GN_SLAB;
        const int cnt = rows * G * 2;
        for (int i = t; i < cnt; i += blockDim.x) slab[i] = src[(size_t)y0 * G * 2 + i];
        __syncthreads();
        if (t < G) {
            for (int y = 0; y < rows; ++y) {
                S = S + slab[(y * G + t) * 2];
                SS = SS + slab[(y * G + t) * 2 + 1];
            }
        }
        __syncthreads();
    }
    if (t < G) {
        const int g = t;
        const double N = (double)H * (double)W * (double)cg;
        const double mean = S / N;
        double var = SS / N - mean * mean;
        if (var < 0.0) var = 0.0;
        const float rstd = 1.0f / sqrtf((float)var + eps);
        const float meanf = (float)mean;
        for (int j = 0; j < cg; ++j) {
            const int c = g * cg + j;
            const float ac = rstd * gamma[c];
            a[n * C + c] = ac;
            b[n * C + c] = __builtin_fmaf(-meanf, ac, beta[c]);
        }
    }
}

// Per-(sample, 8x16 tile, group) partial moments in the order of oracle/femasr_oracle.c orc_gn_coeffs (levels 0-3), for
// tensors that do not come out of a 3x3 halo conv (whose epilogue emits the same partials itself).  One wave per
// (sample, tile, 32-channel slab): lane = (channel c31, half h) exactly like an MFMA accumulator lane.
__global__ __launch_bounds__(64) void gn_tile_partials_kernel(const float *__restrict__ x, int H, int W, int C, int tilesX, int tilesY,
                                                              double *__restrict__ part)
{
    const int lane = threadIdx.x, c31 = lane & 31, h = lane >> 5;
    const int slabs = C >> 5, cg = C >> 5;          // 32 groups: channels per group == number of 32-channel slabs
    int b = blockIdx.x;
    const int slab = b % slabs;
    b /= slabs;
    const int tx = b % tilesX;
    b /= tilesX;
    const int ty = b % tilesY;
    const int n = b / tilesY;
    const float *xn = x + (size_t)n * H * W * C + slab * 32 + c31;
    double S = 0.0, SS = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double s = 0.0, ss = 0.0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = 32 * q + 4 * h + (r & 3) + 8 * (r >> 2);
            const int y = 8 * ty + (m >> 4), xx = 16 * tx + (m & 15);
            if (y < H && xx < W) {
                const double d = (double)xn[((size_t)y * W + xx) * C];
                s = s + d;
                ss = __builtin_fma(d, d, ss);
            }
        }
        s = s + __shfl_xor(s, 32, 64);
        ss = ss + __shfl_xor(ss, 32, 64);
        for (int d = 1; d < cg; d <<= 1) {
            s = s + __shfl_xor(s, d, 64);
            ss = ss + __shfl_xor(ss, d, 64);
        }
        if (q == 0) { S = s; SS = ss; } else { S = S + s; SS = SS + ss; }
    }
    const int ch = slab * 32 + c31;
    if (lane < 32 && (ch & (cg - 1)) == 0) {
        double *dst = part + ((((size_t)n * tilesY + ty) * tilesX + tx) * 32 + ch / cg) * 2;
        dst[0] = S;
        dst[1] = SS;
    }
}

// Finalise from the per-tile partial moments (fp32 halo conv epilogue / gn_tile_partials_kernel: exact fixed order,
// level 4 of orc_gn_coeffs; bf16x3 conv epilogue: tolerance-based path, same finalize) (tolerance-based path: the summation order is
// free but FIXED, so runs are reproducible).  One wave per (image, group): lane l adds tiles l, l+64, ... then an xor
// tree - the sequential version above takes 320 us on the 2592-tile 576^2 layers, this one a few us.
__global__ __launch_bounds__(64) void gn_finalize_partials_kernel(const double *__restrict__ part, int tiles, int H, int W, int C, int G,
                                                                  const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                  float eps, float *__restrict__ a, float *__restrict__ b)
{
    const int n = blockIdx.x / G, g = blockIdx.x % G, lane = threadIdx.x, cg = C / G;
    const double *src = part + ((size_t)n * tiles * G + g) * 2;
    double S = 0.0, SS = 0.0;
    for (int t = lane; t < tiles; t += 64) {
        S += src[(size_t)t * G * 2];
        SS += src[(size_t)t * G * 2 + 1];
    }
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1) {
        S += __shfl_xor(S, sft, 64);
        SS += __shfl_xor(SS, sft, 64);
    }
    const double N = (double)H * (double)W * (double)cg;
    const double mean = S / N;
    double var = SS / N - mean * mean;
    if (var < 0.0) var = 0.0;
    const float rstd = 1.0f / sqrtf((float)var + eps);
    const float meanf = (float)mean;
    if (lane < cg) {
        const int c = g * cg + lane;
        const float ac = rstd * gamma[c];
        a[n * C + c] = ac;
        b[n * C + c] = __builtin_fmaf(-meanf, ac, beta[c]);
    }
}

// y = silu(fmaf(x, a[n][c], b[n][c])): GroupNorm-apply + SiLU (fema_utils.py:22,54-55,73-74,76-77) as a pass of its own - the arithmetic of the
// conv kernels' GN+SiLU prologue (det_silu: the IEEE-exact form), for convs that take their input without a prologue (round 6: the 3x3
// convs in front of the codebook lookup run as the split-bf16 GEMM, kernels_gemm_bf16.hip).  Thread = one float4 of channels.
__global__ void gn_silu_apply_kernel(const float *__restrict__ x, int C, long long hw, const float *__restrict__ a, const float *__restrict__ b,
                                     float *__restrict__ y, size_t total4)
{
    const int c4n = C >> 2;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % c4n);
        const size_t n = (i / c4n) / (size_t)hw;
        const float4 v = ld4(x + 4 * i), ga = ld4(a + n * C + 4 * c4), gb = ld4(b + n * C + 4 * c4);
        float4 o;
        o.x = det_silu(__builtin_fmaf(v.x, ga.x, gb.x));
        o.y = det_silu(__builtin_fmaf(v.y, ga.y, gb.y));
        o.z = det_silu(__builtin_fmaf(v.z, ga.z, gb.z));
        o.w = det_silu(__builtin_fmaf(v.w, ga.w, gb.w));
        *reinterpret_cast<float4 *>(y + 4 * i) = o;
    }
}

// ------------------------------------------------------------------------------------------
// LayerNorm moments (network_swinir.py:199,205): one wave per row of C = 64*PER floats
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_tree_sum(float p)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) p = p + __shfl_xor(p, s, 64);
    return p;
}

__global__ void ln_stats_kernel(const float *__restrict__ x, long long rows, float eps, float *__restrict__ stats)
{
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float4 v = ld4(x + row * 256 + lane * 4);
    float s = v.x;
    s = s + v.y;
    s = s + v.z;
    s = s + v.w;
    const float mean = wave_tree_sum(s) * (1.0f / 256.0f);
    float d = v.x - mean;
    float q = d * d;
    d = v.y - mean;
    q = __builtin_fmaf(d, d, q);
    d = v.z - mean;
    q = __builtin_fmaf(d, d, q);
    d = v.w - mean;
    q = __builtin_fmaf(d, d, q);
    const float var = wave_tree_sum(q) * (1.0f / 256.0f);
    if (lane == 0) {
        stats[2 * row] = mean;
        stats[2 * row + 1] = 1.0f / sqrtf(var + eps);
    }
}

// y = LayerNorm(x): the moments above, then fmaf((x - mean) * rstd, gamma, beta) (network_swinir.py:243,277).  The
// normalised tokens are materialised ONCE so that the qkv / fc1 GEMMs can stream raw operand tiles into LDS by DMA.
__global__ void layernorm_kernel(const float *__restrict__ x, long long rows, const float *__restrict__ gamma,
                                 const float *__restrict__ beta, float eps, float *__restrict__ y)
{
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float4 v = ld4(x + row * 256 + lane * 4);
    float s = v.x;
    s = s + v.y;
    s = s + v.z;
    s = s + v.w;
    const float mean = wave_tree_sum(s) * (1.0f / 256.0f);
    float d = v.x - mean;
    float q = d * d;
    d = v.y - mean;
    q = __builtin_fmaf(d, d, q);
    d = v.z - mean;
    q = __builtin_fmaf(d, d, q);
    d = v.w - mean;
    q = __builtin_fmaf(d, d, q);
    const float var = wave_tree_sum(q) * (1.0f / 256.0f);
    const float rstd = 1.0f / sqrtf(var + eps);
    const float4 g = ld4(gamma + lane * 4), b = ld4(beta + lane * 4);
    float4 o;
    o.x = __builtin_fmaf((v.x - mean) * rstd, g.x, b.x);
    o.y = __builtin_fmaf((v.y - mean) * rstd, g.y, b.y);
    o.z = __builtin_fmaf((v.z - mean) * rstd, g.z, b.z);
    o.w = __builtin_fmaf((v.w - mean) * rstd, g.w, b.w);
    *reinterpret_cast<float4 *>(y + row * 256 + lane * 4) = o;
}

// ------------------------------------------------------------------------------------------
// 8x8 (shifted-)window attention (network_swinir.py:114-145,216-237,249-272)
// ------------------------------------------------------------------------------------------
// Roll / window partition / reverse are index math; the shift mask is the analytic label test (the reference builds a
// (nW,64,64) mask tensor); softmax and both products follow the oracle's fixed orders.
constexpr int ATT_HD = 32, ATT_N = 64;
typedef float att_f32x16 __attribute__((ext_vector_type(16)));

// ------------------------------------------------------------------------------------------
// Window attention, register-resident form (the one the network runs).  One wave per (sample, window, head).
// (One 8-wave block per window - all heads of a token read together - measured SLOWER: 173 vs 129 us per launch at B = 16.)
//   S^T = K (q*scale)^T on v_mfma_f32_32x32x2_f32: tile [32 keys][32 queries], so lane (c = lane&31, half = lane>>5) owns QUERY
//         row i = 32*ti + c and, in its 16 accumulator registers r of key tile tj, the keys  j = (r&3) + 8(r>>2) + 4*half + 32*tj
//         - a softmax row lives in ONE lane pair: max / exp / sum need a single cross-half exchange, no LDS transpose;
//   the probabilities stay in those accumulator registers and ARE the A operand of the P.V MFMA (step (tj, r) multiplies key
//         j(r,tj,0) in k-slot 0 and j(r,tj,1) in k-slot 1), so each o[d] is one fmaf chain over the keys in the order
//         0,4,1,5,2,6,3,7 inside every group of 8 - the order oracle/femasr_oracle.c specifies (ORC_KPERM); the partial
//         sums of the two halves likewise;
//   K / Q rows are read straight from global (one 128-byte row per lane), V as one float per lane and step (128 contiguous
//         bytes per half-wave), issued before the softmax so that its VALU work covers their latency; O leaves as 128-byte
//         row segments.  LDS holds only the 225-entry bias table: no barriers beyond the one after its load.
// ------------------------------------------------------------------------------------------
// UNITS = (window, head) units a wave works through (consecutive unit numbers: the same window, the next head).  With 2 the Q / K rows of the
// second unit are requested as soon as the first unit's S^T MFMAs have consumed their registers - in flight under its softmax and P V -
// and half as many waves are launched.  Every unit is computed by the same instruction sequence either way: bit-identical.  Measured in
// round 4: 2 is 4-5 % SLOWER than 1 - 133 against 127 us at B = 16, 256 registers (profiles/r04_p_attention_units.txt) - so only 1 is
// instantiated.  (The single-trip loops stay: written without them the same kernel compiles to a different instruction order.)
template <int UNITS>
__global__ __launch_bounds__(64, 2) void window_attention_reg_kernel(const float *__restrict__ qkv, int B, int H, int W, int C,
                                                                     int heads, int shift, const float *__restrict__ table,
                                                                     float *__restrict__ out, int total)
{
    __shared__ float Ts[UNITS][232];
    const int lane = threadIdx.x, c = lane & 31, hf = lane >> 5;
    const int nwx = W >> 3, nwy = H >> 3;
    struct Unit { int h, wx, wy, n; };
    auto unit_of = [&](int bid) {
        Unit g;
        g.h = bid % heads;
        bid /= heads;
        g.wx = bid % nwx;
        bid /= nwx;
        g.wy = bid % nwy;
        g.n = bid / nwy;
        return g;
    };
    Unit gs[UNITS];
    bool has[UNITS];
#pragma unroll
    for (int u = 0; u < UNITS; ++u) {
        const int bid = (int)blockIdx.x * UNITS + u;
        has[u] = bid < total;                                     // (uniform)
        gs[u] = unit_of(has[u] ? bid : total - 1);
        for (int i = lane; i < 225; i += 64) Ts[u][i] = table[i * heads + gs[u].h];      // one wave: its own LDS writes are ordered before its reads
    }
    const float scale = 0.17677669529663687f;   // (float)(32 ** -0.5)
    // token offsets of window positions: row part (8 window rows) + column part (8 window columns), roll folded in
    auto rowtok = [&](const Unit &g, int iy) { int y = g.wy * 8 + iy + shift; if (y >= H) y -= H; return y * W; };
    auto coltok = [&](const Unit &g, int ix) { int x = g.wx * 8 + ix + shift; if (x >= W) x -= W; return x; };
    auto qb = [&](const Unit &g) { return qkv + (size_t)g.n * H * W * 3 * C + g.h * ATT_HD; };      // this sample / head: 32-bit element offsets from here on

    // ---- operands of S^T: lane (c, hf) holds row (32*t + c) of K / Q, elements d = 2s + hf
    float ak[2][16], bq[2][16];
    auto load_qk = [&](const Unit &g) {
        const float *qbase = qb(g);
#pragma unroll
        for (int tI = 0; tI < 2; ++tI) {
            const int w = 32 * tI + c;                     // window position 0..63 of this lane's row
            const unsigned tok = (unsigned)(rowtok(g, w >> 3) + coltok(g, w & 7));
            const float *kp = qbase + tok * (unsigned)(3 * C) + C, *qp = qbase + tok * (unsigned)(3 * C);
#pragma unroll
            for (int d4 = 0; d4 < 8; ++d4) {
                const float4 kv = ld4(kp + 4 * d4), qv = ld4(qp + 4 * d4);
                ak[tI][2 * d4] = hf ? kv.y : kv.x;
                ak[tI][2 * d4 + 1] = hf ? kv.w : kv.z;
                bq[tI][2 * d4] = (hf ? qv.y : qv.x) * scale;
                bq[tI][2 * d4 + 1] = (hf ? qv.w : qv.z) * scale;
            }
        }
    };
    load_qk(gs[0]);
#pragma unroll
    for (int u = 0; u < UNITS; ++u) {
        if (!has[u]) break;
        const Unit g = gs[u];
        const float *qbase = qb(g);
        float *obase = out + (size_t)g.n * H * W * C + g.h * ATT_HD;
        // the shift mask is non-zero only in the last window row / column of the shifted frame (network_swinir.py:216-237): everywhere else
        // every key shares its query's region and the reference adds 0.0 - which a wave-uniform test skips (same bits: s + 0.0 == s up to
        // the sign of a zero, which neither the max nor the exponential sees)
        const bool masked = shift > 0 && (g.wy == nwy - 1 || g.wx == nwx - 1);
        att_f32x16 sc[2][2];      // [tj][ti]
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                for (int r = 0; r < 16; ++r) sc[tj][ti][r] = 0.f;
#pragma unroll
        for (int st = 0; st < 16; ++st)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int ti = 0; ti < 2; ++ti) sc[tj][ti] = __builtin_amdgcn_mfma_f32_32x32x2f32(ak[tj][st], bq[ti][st], sc[tj][ti], 0, 0, 0);

        // ---- V operands of O = P V: step (tj, r) needs V[j(r,tj,hf)][d = c]; issued now, consumed after the softmax
        float vf[2][16];
        {
            const float *vb = qbase + 2 * C + c;
            unsigned cto[4];          // per-lane element offset of the 4 window columns this half touches
#pragma unroll
            for (int e = 0; e < 4; ++e) cto[e] = (unsigned)coltok(g, e + 4 * hf) * (unsigned)(3 * C);
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const unsigned ro = (unsigned)__builtin_amdgcn_readfirstlane(rowtok(g, (r >> 2) + 4 * tj)) * (unsigned)(3 * C);   // uniform
                    vf[tj][r] = vb[ro + cto[r & 3]];
                }
        }
        if (u + 1 < UNITS && has[u + 1 < UNITS ? u + 1 : u]) load_qk(gs[u + 1 < UNITS ? u + 1 : u]);      // (the operand registers are free again)
        // ---- softmax per query row (this lane: rows i = 32*ti + c, its half of the keys)
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) {
            const int i = 32 * ti + c, iy = i >> 3, ix = i & 7;
            const int tb = (iy + 7) * 15 + ix + 7 - 4 * hf;          // bias index of key (jy, jx) is tb - 15*jy - (jx - 4*hf)
            unsigned rowdiff = 0, coldiff = 0;                         // bit jy / bit (jx - 4*hf): key in another mask region
            if (masked) {
                const int ysi = g.wy * 8 + iy, xsi = g.wx * 8 + ix;
                const int ryi = ysi < H - 8 ? 0 : (ysi < H - shift ? 1 : 2), rxi = xsi < W - 8 ? 0 : (xsi < W - shift ? 1 : 2);
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int ysj = g.wy * 8 + q, xsj = g.wx * 8 + q;
                    const int ryj = ysj < H - 8 ? 0 : (ysj < H - shift ? 1 : 2), rxj = xsj < W - 8 ? 0 : (xsj < W - shift ? 1 : 2);
                    rowdiff |= (ryj != ryi ? 1u : 0u) << q;
                    coldiff |= (rxj != rxi ? 1u : 0u) << q;
                }
                coldiff >>= 4 * hf;
            }
            float m = -INFINITY;
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int jy = (r >> 2) + 4 * tj, jxl = r & 3;
                    float a1 = sc[tj][ti][r] + Ts[u][tb - 15 * jy - jxl];
                    if (masked) a1 = a1 + ((((rowdiff >> jy) | (coldiff >> jxl)) & 1u) ? -100.0f : 0.0f);
                    sc[tj][ti][r] = a1;
                    m = a1 > m ? a1 : m;
                }
            {
                const float mo = __shfl_xor(m, 32, 64);
                m = mo > m ? mo : m;
            }
            float part = 0.f;
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int r = 0; r < 16; r += 2) {      // the exponential two keys at a time on the packed ALU (bit-identical per element); the sum stays one chain
                    const det_f32x2 e = det_expf2(det_f32x2{sc[tj][ti][r] - m, sc[tj][ti][r + 1] - m});
                    sc[tj][ti][r] = e[0];
                    sc[tj][ti][r + 1] = e[1];
                    part = part + e[0];
                    part = part + e[1];
                }
            const float other = __shfl_xor(part, 32, 64);
            const float rinv = 1.0f / (hf ? other + part : part + other);          // half 0 + half 1; one IEEE division per row
#pragma unroll
            for (int tj = 0; tj < 2; ++tj) sc[tj][ti] = sc[tj][ti] * rinv;          // (vector form: v_pk_mul_f32 on register pairs)
        }

        // ---- O = P V: A = probabilities (accumulator registers of S^T), B = V
        att_f32x16 oc[2];
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int r = 0; r < 16; ++r) oc[ti][r] = 0.f;
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int r = 0; r < 16; ++r)
#pragma unroll
                for (int ti = 0; ti < 2; ++ti) oc[ti] = __builtin_amdgcn_mfma_f32_32x32x2f32(sc[tj][ti][r], vf[tj][r], oc[ti], 0, 0, 0);

        // ---- store: oc[ti][r] = O[i = 32*ti + (r&3) + 8(r>>2) + 4*hf][d = c]
        {
            float *ob = obase + c;
            unsigned cto[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) cto[e] = (unsigned)coltok(g, e + 4 * hf) * (unsigned)C;
#pragma unroll
            for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const unsigned ro = (unsigned)__builtin_amdgcn_readfirstlane(rowtok(g, (r >> 2) + 4 * ti)) * (unsigned)C;
                    ob[ro + cto[r & 3]] = oc[ti][r];
                }
        }
    }
}

// ------------------------------------------------------------------------------------------
// VQ helpers (femasr_arch.py:35-38,63-66,81-82,95,100,102-112)
// ------------------------------------------------------------------------------------------
// |row|^2 as ONE fmaf chain, c ascending; thread per row, float4 loads.
__global__ void row_sqsum_kernel(const float *__restrict__ x, long long rows, int D, float *__restrict__ out)
{
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const float *p = x + r * D;
    float acc = 0.f;
    for (int c = 0; c < D; c += 4) {
        const float4 v = ld4(p + c);
        acc = __builtin_fmaf(v.x, v.x, acc);
        acc = __builtin_fmaf(v.y, v.y, acc);
        acc = __builtin_fmaf(v.z, v.z, acc);
        acc = __builtin_fmaf(v.w, v.w, acc);
    }
    out[r] = acc;
}

// one wave per row: pick the first-min over the n-block partials (ascending block order),
// write idx (int64) and z_q = z + (e[idx] - z).
__global__ void vq_finalize_kernel(const float *__restrict__ z, long long M, int D, const float *__restrict__ cb,
                                   const float *__restrict__ part, int nblk, int n_e, long long *__restrict__ idx,
                                   float *__restrict__ zq)
{
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= M) return;
    const int lane = threadIdx.x & 63;
    const float *pp = part + (size_t)row * nblk * 2;
    float bd = pp[0];
    int bi = __float_as_int(pp[1]);
    for (int b = 1; b < nblk; ++b) {
        const float d = pp[2 * b];
        const int i = __float_as_int(pp[2 * b + 1]);
        if (d < bd || (d == bd && i < bi)) { bd = d; bi = i; }
    }
    bi = bi < 0 ? 0 : (bi >= n_e ? n_e - 1 : bi);     // NaN rows leave the sentinel: never index out of the codebook
    if (lane == 0) idx[row] = (long long)bi;
    const float *e = cb + (size_t)bi * D;
    const float *zr = z + (size_t)row * D;
    float *o = zq + (size_t)row * D;
    for (int c = lane * 4; c < D; c += 256) {
        const float4 zv = ld4(zr + c), ev = ld4(e + c);
        float4 r;
        r.x = zv.x + (ev.x - zv.x);
        r.y = zv.y + (ev.y - zv.y);
        r.z = zv.z + (ev.z - zv.z);
        r.w = zv.w + (ev.w - zv.w);
        *reinterpret_cast<float4 *>(o + c) = r;
    }
}

__global__ void codebook_gather_kernel(const long long *__restrict__ idx, long long M, int D, const float *__restrict__ cb,
                                       int n_e, float *__restrict__ zq)
{
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= M) return;
    const int lane = threadIdx.x & 63;
    long long i = idx[row];
    i = i < 0 ? 0 : (i >= n_e ? n_e - 1 : i);
    for (int c = lane * 4; c < D; c += 256)
        *reinterpret_cast<float4 *>(zq + (size_t)row * D + c) = ld4(cb + (size_t)i * D + c);
}

// OIHW -> the FRAGMENT-MAJOR weight layout the conv kernels read straight into MFMA B operands:
//   out[q][ntile][lane][kk],  q = k/32, kk = (k%32)/2, lane = (k&1)*32 + n%32, ntile = n/32,  zero padded
//   K order:  I % 32 == 0:  k = ((ci/32)*kh*kw + y*kw + x)*32 + ci%32      (channel blocks outermost)
//             otherwise  :  k = (y*kw + x)*I + ci
// thread per OUTPUT element (coalesced stores)
__global__ void repack_oihw_kernel(const float *__restrict__ in, int O, int I, int kh, int kw, float *__restrict__ out,
                                   size_t total)
{
    const bool blocked = (I % 32) == 0;
    const int K = I * kh * kw, NT32 = (O + 31) / 32;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int kk = (int)(i & 15), lane = (int)((i >> 4) & 63);
        const size_t rest = i >> 10;
        const int ntile = (int)(rest % NT32), q = (int)(rest / NT32);
        const int k = q * 32 + kk * 2 + (lane >> 5), o = ntile * 32 + (lane & 31);
        float v = 0.f;
        if (k < K && o < O) {
            int ci, x, y;
            if (blocked) {
                const int cl = k % 32;
                int r = k / 32;
                x = r % kw;
                r /= kw;
                y = r % kh;
                ci = (r / kh) * 32 + cl;
            } else {
                ci = k % I;
                const int r = k / I;
                x = r % kw;
                y = r / kw;
            }
            v = in[(((size_t)o * I + ci) * kh + y) * kw + x];
        }
        out[i] = v;
    }
}

// 3x3 OIHW -> the 4 phase matrices of nearest-x2 + conv (oracle/femasr_oracle.c orc_conv_up2_phases): phase (a, b), slot
// (ty, tx) holds sum over ky in slot ty (ascending) of (sum over kx in slot tx (ascending) of w[o][ci][ky][kx]), slots
// a=0: {0},{1,2}; a=1: {0,1},{2}.  Each matrix in the fragment-major layout of a 2x2 conv (k = (cb*4 + ty*2 + tx)*32 + ci%32).
__global__ void repack_up2_kernel(const float *__restrict__ in, int O, int I, float *__restrict__ out, size_t per_phase)
{
    const int K = I * 4, NT32 = (O + 31) / 32;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < 4 * per_phase; i += (size_t)gridDim.x * blockDim.x) {
        const int ph = (int)(i / per_phase);
        const size_t e = i - (size_t)ph * per_phase;
        const int kk = (int)(e & 15), lane = (int)((e >> 4) & 63);
        const size_t rest = e >> 10;
        const int ntile = (int)(rest % NT32), q = (int)(rest / NT32);
        const int k = q * 32 + kk * 2 + (lane >> 5), o = ntile * 32 + (lane & 31);
        float v = 0.f;
        if (k < K && o < O) {
            const int a = ph >> 1, b = ph & 1;
            const int cl = k % 32, r = k / 32, tap = r & 3, ci = (r >> 2) * 32 + cl;
            const int ty = tap >> 1, tx = tap & 1;
            const int y0 = ty == 0 ? 0 : (a == 0 ? 1 : 2), y1 = ty == 0 ? (a == 0 ? 0 : 1) : 2;
            const int x0 = tx == 0 ? 0 : (b == 0 ? 1 : 2), x1 = tx == 0 ? (b == 0 ? 0 : 1) : 2;
            const float *w = in + ((size_t)o * I + ci) * 9;
            for (int ky = y0; ky <= y1; ++ky) {
                float row = w[ky * 3 + x0];
                for (int kx = x0 + 1; kx <= x1; ++kx) row = row + w[ky * 3 + kx];
                v = ky == y0 ? row : v + row;
            }
        }
        out[i] = v;
    }
}

// compact [k][4] weights of a conv with <= 4 output channels, k in the blocked order above (zero padded to 4 columns)
__global__ void repack_compact_kernel(const float *__restrict__ in, int O, int I, int kh, int kw, float *__restrict__ out, size_t total)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int o = (int)(i & 3), k = (int)(i >> 2);
        const int cl = k % 32;
        int r = k / 32;
        const int x = r % kw;
        r /= kw;
        const int y = r % kh, ci = (r / kh) * 32 + cl;
        out[i] = o < O ? in[(((size_t)o * I + ci) * kh + y) * kw + x] : 0.f;
    }
}

// ------------------------------------------------------------------------------------------
// image pre / post-processing on the GPU (the steps either side of the path)
// ------------------------------------------------------------------------------------------
// img2tensor(...)/255. (basicsr/utils/img_util.py:9-35; inference_femasr.py:55): uint8 HWC (BGR or RGB)
// -> fp32 CHW RGB, value = (float)u8 / 255.0f with an IEEE division.
__global__ void image_u8_to_f32_kernel(const unsigned char *__restrict__ in, int H, int W, int swap_rb,
                                       float *__restrict__ out, size_t total)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % W);
        size_t r = i / W;
        const int y = (int)(r % H);
        const int c = (int)(r / H);
        const int sc = swap_rb ? 2 - c : c;
        out[i] = (float)in[((size_t)y * W + x) * 3 + sc] / 255.0f;
    }
}

// tensor2img (img_util.py:38-94): clamp to [0,1], CHW RGB -> HWC (BGR or RGB), (x*255).round() (half to even) -> uint8
__global__ void image_f32_to_u8_kernel(const float *__restrict__ in, int H, int W, int swap_rb,
                                       unsigned char *__restrict__ out, size_t total)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % 3);
        size_t r = i / 3;
        const int x = (int)(r % W);
        const int y = (int)(r / W);
        const int sc = swap_rb ? 2 - c : c;
        float v = in[((size_t)sc * H + y) * W + x];
        v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);       // NaN -> 1 like neither; NaNs never reach here on finite inputs
        if (!(v == v)) v = 0.f;
        out[i] = (unsigned char)rintf(v * 255.0f);
    }
}

// ------------------------------------------------------------------------------------------
// test_tile (femasr_arch.py:387-447): crops of one shape class -> one batch; upscaled tile bodies -> the canvas
// ------------------------------------------------------------------------------------------
// out[(k*B + b), c, y, x] = in[b, c, yx[2k] + y, yx[2k+1] + x]   (NCHW; the reference's input[:, :, y0p:y1p, x0p:x1p])
__global__ void extract_tiles_kernel(const float *__restrict__ in, int B, int C, int H, int W, const int *__restrict__ yx, int n,
                                     int th, int tw, float *__restrict__ out, size_t total)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % tw);
        size_t r = i / tw;
        const int y = (int)(r % th);
        r /= th;
        const int c = (int)(r % C);
        r /= C;
        const int b = (int)(r % B), k = (int)(r / B);
        out[i] = in[(((size_t)b * C + c) * H + yx[2 * k] + y) * W + yx[2 * k + 1] + x];
    }
}

// canvas[b, c, dy + y, dx + x] = tiles[(k*B + b), c, sy + y, sx + x] for y < h, x < w; rect k = (sy, sx, dy, dx, h, w)
// (`output[:, :, dst] = output_tile[:, :, src]`, femasr_arch.py:443-446).  One block row per (tile, image, channel, row).
__global__ void paste_tiles_kernel(const float *__restrict__ tiles, int B, int C, int th, int tw, const int *__restrict__ rects,
                                   int n, int Ho, int Wo, float *__restrict__ out, int hmax)
{
    size_t r = blockIdx.x;
    const int y = (int)(r % hmax);
    r /= hmax;
    const int c = (int)(r % C);
    r /= C;
    const int b = (int)(r % B), k = (int)(r / B);
    const int *rc = rects + 6 * k;
    if (y >= rc[4]) return;
    const float *src = tiles + ((((size_t)k * B + b) * C + c) * th + rc[0] + y) * tw + rc[1];
    float *dst = out + (((size_t)b * C + c) * Ho + rc[2] + y) * Wo + rc[3];
    for (int x = threadIdx.x; x < rc[5]; x += blockDim.x) dst[x] = src[x];
}

// The same two steps on uint8 HWC images (round 6: the tiled / multi-GPU path moves one byte per value): crops of a (B,H,W,3) image -> (n*B, th, tw, 3);
// tile bodies -> the (B,Ho,Wo,3) canvas.  Thread = one pixel row segment byte; rows are 3 * w contiguous bytes.
__global__ void extract_tiles_u8_kernel(const unsigned char *__restrict__ in, int B, int H, int W, const int *__restrict__ yx, int n,
                                        int th, int tw, unsigned char *__restrict__ out, size_t total)
{
    const int rowb = 3 * tw;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int xb = (int)(i % rowb);
        size_t r = i / rowb;
        const int y = (int)(r % th);
        r /= th;
        const int b = (int)(r % B), k = (int)(r / B);
        out[i] = in[(((size_t)b * H + yx[2 * k] + y) * W + yx[2 * k + 1]) * 3 + xb];
    }
}

__global__ void paste_tiles_u8_kernel(const unsigned char *__restrict__ tiles, int B, int th, int tw, const int *__restrict__ rects,
                                      int n, int Ho, int Wo, unsigned char *__restrict__ out, int hmax)
{
    size_t r = blockIdx.x;
    const int y = (int)(r % hmax);
    r /= hmax;
    const int b = (int)(r % B), k = (int)(r / B);
    const int *rc = rects + 6 * k;
    if (y >= rc[4]) return;
    const unsigned char *src = tiles + ((((size_t)k * B + b) * th + rc[0] + y) * tw + rc[1]) * 3;
    unsigned char *dst = out + (((size_t)b * Ho + rc[2] + y) * Wo + rc[3]) * 3;
    for (int x = threadIdx.x; x < 3 * rc[5]; x += blockDim.x) dst[x] = src[x];
}

// ------------------------------------------------------------------------------------------
// Overlap-blend paste (NOT the reference's arithmetic; opt-in): every canvas pixel is the weighted mean of the
// upscaled WINDOWS (halo included) that contain it, tiles visited in row-major order.  Gather form: one thread per canvas element,
// no atomics, no weight canvas, the canvas is written once and never read.
// geom[8k..] = (window origin y, x on the canvas, th, tw, leading / trailing margin in y, leading / trailing margin in x) in upscaled
// pixels (tiling.blend_table); a margin of 0 is an image border.  ptrs[k] = tile k, image 0; image b follows th*tw*channels later.
// ------------------------------------------------------------------------------------------
// 1-D weight of window coordinate i in [0, len): a linear ramp over the 2*margin wide overlap, centred on the body edge, sampled at
// pixel centres; > 0 everywhere, 1 outside the ramps.  One IEEE divide per side (the integers are exact in fp32: below 2^24).
__device__ __forceinline__ float blend_weight(int i, int len, int lead, int trail)
{
    const float wl = lead == 0 ? 1.0f : fminf(1.0f, (float)(2 * i + 1) / (float)(4 * lead));
    const float wr = trail == 0 ? 1.0f : fminf(1.0f, (float)(2 * (len - 1 - i) + 1) / (float)(4 * trail));
    return fminf(wl, wr);
}

// One block = one canvas row (b, c, Y) inside one body-cell column cx: the candidate tiles - the pixel's own cell and its +-1
// neighbours (2 tile_pad <= tile_size) - depend on the block alone, so the table reads are scalar loads and every tile row is
// read as one contiguous run along x.  The last cell row / column takes what the canvas has beyond it (hand-made tables only).
template <bool U8>
__global__ __launch_bounds__(256) void blend_tiles_kernel(const unsigned long long *__restrict__ ptrs, const int *__restrict__ geom,
                                                         int tiles_y, int tiles_x, int pitch, int C, int Ho, int Wo, void *__restrict__ out_)
{
    using T = typename std::conditional<U8, unsigned char, float>::type;
    // fp32: rows are (b, c, Y), E = 1 element per pixel; uint8 HWC: rows are (b, Y), E = 3 interleaved elements per pixel
    const int E = U8 ? 3 : 1;
    size_t r = blockIdx.x;
    const int Y = (int)(r % Ho);
    r /= Ho;
    const int c = U8 ? 0 : (int)(r % C);
    const size_t b = U8 ? r : r / C;
    const int cx = blockIdx.y, cy = min(Y / pitch, tiles_y - 1);
    const int x0 = cx * pitch, x1 = cx == tiles_x - 1 ? Wo : min(x0 + pitch, Wo);
    T *dst = (T *)out_ + (size_t)blockIdx.x * Wo * E;
    for (int j = x0 * E + threadIdx.x; j < x1 * E; j += blockDim.x) {
        const int X = U8 ? j / 3 : j, ch = U8 ? j - 3 * X : 0;
        float acc = 0.0f, den = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int ty = cy + dy;
            if (ty < 0 || ty >= tiles_y) continue;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int tx = cx + dx;
                if (tx < 0 || tx >= tiles_x) continue;
                const int k = ty * tiles_x + tx;
                const int *g = geom + 8 * k;
                const int ly = Y - g[0], th = g[2], tw = g[3];
                if (ly < 0 || ly >= th) continue;                          // (block-uniform)
                const int lx = X - g[1];
                if (lx < 0 || lx >= tw) continue;                          // every read stays inside the th x tw tile the table names
                const float w = blend_weight(ly, th, g[4], g[5]) * blend_weight(lx, tw, g[6], g[7]);
                const T *t = (const T *)ptrs[k] + b * ((size_t)th * tw * (U8 ? 3 : C));
                const float v = (float)(U8 ? t[((size_t)ly * tw + lx) * 3 + ch] : t[((size_t)c * th + ly) * tw + lx]);
                acc = acc + w * v;
                den = den + w;
            }
        }
        float q = den > 0.0f ? acc / den : 0.0f;                            // (no tile: a hand-made table; 0 like the paste's zero canvas)
        if (U8) {
            q = q < 0.f ? 0.f : (q > 255.f ? 255.f : q);                   // tensor2img's rounding: half to even
            dst[j] = (T)rintf(q);
        } else {
            dst[j] = (T)q;
        }
    }
}

// out[n,y,x,:] = cat(a[n,y,x,:Ca], b[n, y*Hb/H, x*Wb/W, :Cb]); one thread per float4 of the output (Ca, Cb % 4 == 0)
__global__ void concat_resize_kernel(const float *__restrict__ a, int Ca, const float *__restrict__ b, int Hb, int Wb, int Cb,
                                     int H, int W, float *__restrict__ out, size_t total4)
{
    const int C4 = (Ca + Cb) >> 2, Ca4 = Ca >> 2;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4);
        size_t r = i / C4;
        const int x = (int)(r % W);
        r /= W;
        const int y = (int)(r % H);
        const size_t n = r / H;
        float4 v;
        if (c4 < Ca4) {
            v = ld4(a + ((n * H + y) * W + x) * Ca + 4 * c4);
        } else {
            const int sy = (int)(((long long)y * Hb) / H), sx = (int)(((long long)x * Wb) / W);
            v = ld4(b + ((n * Hb + sy) * Wb + sx) * Cb + 4 * (c4 - Ca4));
        }
        *reinterpret_cast<float4 *>(out + i * 4) = v;
    }
}

inline unsigned grid_for(size_t total, int block = 256)
{
    size_t g = (total + block - 1) / block;
    const size_t cap = 256 * 16;
    return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

}  // namespace

// ------------------------------------------------------------------------------------------
// C ABI (include/femasr_hip.h)
// ------------------------------------------------------------------------------------------
// Sustained-clock probe (bench.py): every wave streams back-to-back v_mfma_f32_32x32x2_f32 (64 shader cycles each: the load the
// network's hot kernels put on the chip) and records the s_memtime ticks (= shader cycles) its loop took; ticks / wall time of
// the launch = the clock the chip sustains under that load right now.
typedef float probe_f32x16 __attribute__((ext_vector_type(16)));
__global__ __launch_bounds__(256) void clock_probe_kernel(int groups, float a, float b, unsigned long long *ticks)
{
    probe_f32x16 c0 = {0}, c1 = {0}, c2 = {0}, c3 = {0};
    a += (float)(threadIdx.x & 31) * 0.03125f;        // operands differ from lane to lane (tools/power_probe.py reads the package power under this loop)
    b += (float)((threadIdx.x >> 5) & 1) * 0.25f;
    const unsigned long long t0 = __builtin_readcyclecounter();
    for (int i = 0; i < groups; ++i) {
        c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c1, 0, 0, 0);
        c2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c2, 0, 0, 0);
        c3 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c3, 0, 0, 0);
    }
    float s = 0.f;
    for (int r = 0; r < 16; ++r) s += c0[r] + c1[r] + c2[r] + c3[r];
    const unsigned long long t1 = __builtin_readcyclecounter();
    if ((threadIdx.x & 63) == 0) ticks[blockIdx.x * 4 + (threadIdx.x >> 6)] = (t1 - t0) + (s == 12345.678f ? 1ull : 0ull);
}

extern "C" {

int femasr_pad_nchw_to_nhwc(void *stream, const float *in, int B, int C, int H, int W, int Hp, int Wp, float *out)
{
    FEMASR_REQUIRE(in && out && B > 0 && C > 0 && H > 0 && W > 0, "pad: bad args");
    FEMASR_REQUIRE(Hp >= H && Wp >= W && Hp - H <= H && Wp - W <= W, "pad: mirror pad larger than the image (%d,%d)->(%d,%d)", H, W, Hp, Wp);
    const size_t total = (size_t)B * Hp * Wp * C;
    hipLaunchKernelGGL(pad_nchw_to_nhwc_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, in, B, C, H, W,
                       Hp, Wp, out, total);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

int femasr_pad_u8hwc_to_nhwc(void *stream, const uint8_t *in, int B, int H, int W, int swap_rb, int Hp, int Wp, float *out)
{
    FEMASR_REQUIRE(in && out && B > 0 && H > 0 && W > 0 && Hp >= H && Wp >= W && Hp <= 2 * H && Wp <= 2 * W, "pad_u8: bad args");
    const size_t total = (size_t)B * Hp * Wp * 3;
    hipLaunchKernelGGL(pad_u8hwc_to_nhwc_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, in, B, H, W, swap_rb, Hp, Wp, out, total);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

int femasr_crop_nhwc_to_u8hwc(void *stream, const float *in, int B, int Hs, int Ws, int Hc, int Wc, int swap_rb, uint8_t *out)
{
    FEMASR_REQUIRE(in && out && B > 0 && Hc > 0 && Wc > 0 && Hc <= Hs && Wc <= Ws, "crop_u8: bad args");
    const size_t total = (size_t)B * Hc * Wc * 3;
    hipLaunchKernelGGL(crop_nhwc_to_u8hwc_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, in, B, Hs, Ws, Hc, Wc, swap_rb, out, total);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

int femasr_crop_nhwc_to_nchw(void *stream, const float *in, int B, int Hs, int Ws, int C, int Hc, int Wc, float *out)
{
    FEMASR_REQUIRE(in && out && B > 0 && C > 0 && Hc > 0 && Wc > 0 && Hc <= Hs && Wc <= Ws, "crop: bad args");
    const size_t total = (size_t)B * C * Hc * Wc;
    hipLaunchKernelGGL(crop_nhwc_to_nchw_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, in, B, Hs, Ws,
                       C, Hc, Wc, out, total);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

size_t femasr_gn_scratch_bytes(int B, int H, int W, int C, int G)
{
    if (B <= 0 || H <= 0 || W <= 0 || G <= 0) return 0;
    if (G == 32 && femasr_gn_fusable(C)) return (size_t)B * ((H + 7) / 8) * ((W + 15) / 16) * 32 * 2 * sizeof(double);
    return (size_t)B * H * G * 2 * sizeof(double);
}

int femasr_gn_coeffs(void *stream, const float *x, int B, int H, int W, int C, int G, const float *gamma,
                     const float *beta, float eps, float *a, float *b, void *scratch)
{
    FEMASR_REQUIRE(x && gamma && beta && a && b && scratch, "gn_coeffs: null pointer");
    FEMASR_REQUIRE(B > 0 && H > 0 && W > 0 && G > 0 && C % G == 0, "gn_coeffs: bad shape C=%d G=%d", C, G);
    const int cg = C / G;
    hipStream_t s = (hipStream_t)stream;
    double *part = (double *)scratch;
    if (G == 32 && femasr_gn_fusable(C)) {      // the order the conv epilogues produce (orc_gn_coeffs, tiled branch)
        const int tilesX = (W + 15) / 16, tilesY = (H + 7) / 8;
        hipLaunchKernelGGL(gn_tile_partials_kernel, dim3((unsigned)((size_t)B * tilesY * tilesX * (C / 32))), dim3(64), 0, s, x, H, W, C,
                           tilesX, tilesY, part);
        FEMASR_CHECK_HIP(hipGetLastError());
        return femasr_gn_coeffs_from_partials(stream, part, B, tilesX * tilesY, H, W, C, G, gamma, beta, eps, a, b);
    }
    const size_t total = (size_t)B * H * G;
    const dim3 grid((unsigned)((total + 255) / 256)), blk(256);
    if (cg == 8 && C % 4 == 0)
        hipLaunchKernelGGL(gn_rows_kernel<8>, grid, blk, 0, s, x, B, H, W, C, G, part);
    else if (cg == 4 && C % 4 == 0)
        hipLaunchKernelGGL(gn_rows_kernel<4>, grid, blk, 0, s, x, B, H, W, C, G, part);
    else if (cg == 2)
        hipLaunchKernelGGL(gn_rows_kernel<2>, grid, blk, 0, s, x, B, H, W, C, G, part);
    else
        hipLaunchKernelGGL(gn_rows_generic_kernel, grid, blk, 0, s, x, B, H, W, C, G, cg, part);
    FEMASR_CHECK_HIP(hipGetLastError());
    FEMASR_REQUIRE(G <= 256, "gn_coeffs: at most 256 groups");
    hipLaunchKernelGGL(gn_finalize_kernel, dim3((unsigned)B), dim3(256), (size_t)GN_SLAB * G * 2 * sizeof(double), s, part, B, H, H,
                       W, C, G, gamma, beta, eps, a, b);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

int femasr_gn_coeffs_from_partials(void *stream, const double *part, int B, int tiles, int H, int W, int C, int G,
                                   const float *gamma, const float *beta, float eps, float *a, float *b)
{
    FEMASR_REQUIRE(part && gamma && beta && a && b && B > 0 && tiles > 0 && H > 0 && W > 0, "gn_coeffs_from_partials: bad args");
    FEMASR_REQUIRE(G == 32 && C % G == 0, "gn_coeffs_from_partials: 32 groups");
    FEMASR_REQUIRE(C / G <= 64, "gn_coeffs_from_partials: at most 64 channels per group");
    hipLaunchKernelGGL(gn_finalize_partials_kernel, dim3((unsigned)(B * G)), dim3(64), 0, (hipStream_t)stream, part, tiles, H, W, C,
                       G, gamma, beta, eps, a, b);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

int femasr_gn_silu_apply(void *stream, const float *x, int B, int H, int W, int C, const float *a, const float *b, float *y)
{
    FEMASR_REQUIRE(x && a && b && y && B > 0 && H > 0 && W > 0 && C > 0 && (C % 4) == 0, "gn_silu_apply: bad args (C %% 4 == 0)");
    const size_t total4 = (size_t)B * H * W * (C / 4);
    hipLaunchKernelGGL(gn_silu_apply_kernel, dim3(grid_for(total4)), dim3(256), 0, (hipStream_t)stream, x, C, (long long)H * W, a, b, y, total4);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

int femasr_ln_stats(void *stream, const float *x, int64_t rows, int C, float eps, float *stats)
{
    FEMASR_REQUIRE(x && stats && rows > 0, "ln_stats: bad args");
    FEMASR_REQUIRE(C == 256, "ln_stats: only C == 256 (Swin embed_dim, femasr_arch.py:115) is built, got %d", C);
    hipLaunchKernelGGL(ln_stats_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x,
                       (long long)rows, eps, stats);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

int femasr_layernorm(void *stream, const float *x, int64_t rows, int C, const float *gamma, const float *beta, float eps, float *y)
{
    FEMASR_REQUIRE(x && y && gamma && beta && rows > 0, "layernorm: bad args");
    FEMASR_REQUIRE(C == 256, "layernorm: only C == 256 (Swin embed_dim, femasr_arch.py:115) is built, got %d", C);
    hipLaunchKernelGGL(layernorm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, (long long)rows,
                       gamma, beta, eps, y);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

int femasr_window_attention(void *stream, const float *qkv, int B, int H, int W, int C, int heads, int shift,
                            const float *table, float *out)
{
    FEMASR_REQUIRE(qkv && table && out && B > 0, "window_attention: bad args");
    FEMASR_REQUIRE(H % 8 == 0 && W % 8 == 0 && H >= 8 && W >= 8, "window_attention: H,W must be multiples of 8 (%d,%d)", H, W);
    FEMASR_REQUIRE(heads > 0 && heads <= 8 && C == heads * ATT_HD, "window_attention: head_dim must be 32, at most 8 heads (C=%d heads=%d)", C, heads);
    FEMASR_REQUIRE(shift >= 0 && shift < 8, "window_attention: bad shift %d", shift);
    FEMASR_REQUIRE((size_t)H * W * 3 * C < ((size_t)1 << 30), "window_attention: image too large for 32-bit offsets");
    const size_t total = (size_t)B * (H / 8) * (W / 8) * heads;
    FEMASR_REQUIRE(total < ((size_t)1 << 31), "window_attention: too many (window, head) units");
    hipLaunchKernelGGL(window_attention_reg_kernel<1>, dim3((unsigned)total), dim3(64), 0, (hipStream_t)stream, qkv, B, H, W, C, heads, shift, table,
                       out, (int)total);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

int femasr_row_sqsum(void *stream, const float *x, int64_t rows, int D, float *out)
{
    FEMASR_REQUIRE(x && out && rows > 0 && D > 0 && D % 4 == 0, "row_sqsum: bad args");
    hipLaunchKernelGGL(row_sqsum_kernel, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, (hipStream_t)stream, x,
                       (long long)rows, D, out);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

int femasr_vq(void *stream, const float *z, int64_t M, int D, const float *cb, const float *cbT, const float *ee,
              int n_e, int64_t *idx, float *zq, void *scratch)
{
    FEMASR_REQUIRE(z && cb && cbT && ee && idx && zq && scratch && M > 0, "vq: bad args");
    FEMASR_REQUIRE(D % 32 == 0 && n_e % 128 == 0, "vq: needs e_dim %% 32 == 0 and n_e %% 128 == 0 (D=%d n_e=%d)", D, n_e);
    FEMASR_REQUIRE(M < (1ll << 31) - 256, "vq: too many rows");
    hipStream_t s = (hipStream_t)stream;
    float *zz = (float *)scratch;
    float *part = zz + ((M + 63) / 64) * 64;
    const int nblk = n_e / 128;
    int rc = femasr_row_sqsum(stream, z, M, D, zz);
    if (rc) return rc;
    femasr_conv_args a{};
    a.in = z; a.B = 1; a.H = (int)M; a.W = 1; a.Cin = D; a.w = cbT; a.bias = nullptr; a.Cout = n_e;
    a.ksz = 1; a.stride = 1; a.pad = 0; a.up2 = 0; a.prologue = FEMASR_PRO_NONE; a.act = 0;
    a.Ho = (int)M; a.Wo = 1;
    conv_vq_epilogue ep{zz, ee, part, nblk};
    rc = femasr_conv2d_launch(s, &a, &ep, nullptr, nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL(vq_finalize_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, z, (long long)M, D, cb, part,
                       nblk, n_e, (long long *)idx, zq);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

int femasr_codebook_gather(void *stream, const int64_t *idx, int64_t M, int D, const float *cb, int n_e, float *zq)
{
    FEMASR_REQUIRE(idx && cb && zq && M > 0 && D % 4 == 0 && n_e > 0, "codebook_gather: bad args");
    hipLaunchKernelGGL(codebook_gather_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       (const long long *)idx, (long long)M, D, cb, n_e, zq);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

int femasr_extract_tiles(void *stream, const float *in, int B, int C, int H, int W, const int32_t *yx_dev, int n, int th, int tw, float *out)
{
    FEMASR_REQUIRE(in && yx_dev && out && B > 0 && C > 0 && n > 0 && th > 0 && tw > 0 && th <= H && tw <= W, "extract_tiles: bad args");
    const size_t total = (size_t)n * B * C * th * tw;
    hipLaunchKernelGGL(extract_tiles_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, in, B, C, H, W, yx_dev, n, th, tw, out, total);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

int femasr_paste_tiles(void *stream, const float *tiles, int B, int C, int n, int th, int tw, const int32_t *rects_dev, int hmax,
                       int Ho, int Wo, float *out)
{
    FEMASR_REQUIRE(tiles && rects_dev && out && B > 0 && C > 0 && n > 0 && th > 0 && tw > 0 && hmax > 0 && hmax <= th, "paste_tiles: bad args");
    const size_t rows = (size_t)n * B * C * hmax;
    FEMASR_REQUIRE(rows < ((size_t)1 << 31), "paste_tiles: too many rows");
    hipLaunchKernelGGL(paste_tiles_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, tiles, B, C, th, tw, rects_dev, n, Ho, Wo, out, hmax);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

int femasr_extract_tiles_u8(void *stream, const uint8_t *in, int B, int H, int W, const int32_t *yx_dev, int n, int th, int tw, uint8_t *out)
{
    FEMASR_REQUIRE(in && yx_dev && out && B > 0 && n > 0 && th > 0 && tw > 0 && th <= H && tw <= W, "extract_tiles_u8: bad args");
    const size_t total = (size_t)n * B * th * tw * 3;
    hipLaunchKernelGGL(extract_tiles_u8_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, in, B, H, W, yx_dev, n, th, tw, out, total);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

int femasr_paste_tiles_u8(void *stream, const uint8_t *tiles, int B, int n, int th, int tw, const int32_t *rects_dev, int hmax, int Ho, int Wo, uint8_t *out)
{
    FEMASR_REQUIRE(tiles && rects_dev && out && B > 0 && n > 0 && th > 0 && tw > 0 && hmax > 0 && hmax <= th, "paste_tiles_u8: bad args");
    const size_t rows = (size_t)n * B * hmax;
    FEMASR_REQUIRE(rows < ((size_t)1 << 31), "paste_tiles_u8: too many rows");
    hipLaunchKernelGGL(paste_tiles_u8_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, tiles, B, th, tw, rects_dev, n, Ho, Wo, out, hmax);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

static int blend_launch(bool u8, void *stream, const uint64_t *tile_ptrs_dev, const int32_t *geom_dev, int n, int tiles_y, int tiles_x,
                        int pitch, int B, int C, int Ho, int Wo, void *out)
{
    const char *who = u8 ? "blend_tiles_u8" : "blend_tiles";
    FEMASR_REQUIRE(tile_ptrs_dev && geom_dev && out, "%s: null pointer", who);
    FEMASR_REQUIRE(n > 0 && B > 0 && C > 0 && tiles_y > 0 && tiles_x > 0 && pitch > 0 && Ho > 0 && Wo > 0, "%s: bad sizes", who);
    FEMASR_REQUIRE((long long)tiles_y * tiles_x == n, "%s: %d tiles given for a %d x %d grid", who, n, tiles_y, tiles_x);
    FEMASR_REQUIRE(tiles_x <= 65535, "%s: more than 65535 tile columns", who);
    const size_t rows = (size_t)B * C * Ho;
    FEMASR_REQUIRE(rows < ((size_t)1 << 31), "%s: too many rows", who);
    const dim3 grid((unsigned)rows, (unsigned)tiles_x);
    if (u8)
        hipLaunchKernelGGL(blend_tiles_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned long long *)tile_ptrs_dev,
                           geom_dev, tiles_y, tiles_x, pitch, 1, Ho, Wo, out);
    else
        hipLaunchKernelGGL(blend_tiles_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned long long *)tile_ptrs_dev,
                           geom_dev, tiles_y, tiles_x, pitch, C, Ho, Wo, out);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

int femasr_blend_tiles(void *stream, const uint64_t *tile_ptrs_dev, const int32_t *geom_dev, int n, int tiles_y, int tiles_x, int pitch,
                       int B, int C, int Ho, int Wo, float *out)
{
    return blend_launch(false, stream, tile_ptrs_dev, geom_dev, n, tiles_y, tiles_x, pitch, B, C, Ho, Wo, out);
}

int femasr_blend_tiles_u8(void *stream, const uint64_t *tile_ptrs_dev, const int32_t *geom_dev, int n, int tiles_y, int tiles_x, int pitch,
                          int B, int Ho, int Wo, uint8_t *out)
{
    return blend_launch(true, stream, tile_ptrs_dev, geom_dev, n, tiles_y, tiles_x, pitch, B, 1, Ho, Wo, out);
}

int femasr_concat_resize(void *stream, const float *a, int Ca, const float *b, int Hb, int Wb, int Cb, int B, int H, int W, float *out)
{
    FEMASR_REQUIRE(a && b && out && B > 0 && H > 0 && W > 0 && Hb > 0 && Wb > 0, "concat_resize: bad args");
    FEMASR_REQUIRE(Ca > 0 && Cb > 0 && Ca % 4 == 0 && Cb % 4 == 0, "concat_resize: channel counts must be multiples of 4 (%d, %d)", Ca, Cb);
    const size_t total4 = (size_t)B * H * W * ((Ca + Cb) / 4);
    hipLaunchKernelGGL(concat_resize_kernel, dim3(grid_for(total4)), dim3(256), 0, (hipStream_t)stream, a, Ca, b, Hb, Wb, Cb, H, W, out,
                       total4);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

size_t femasr_packed_weight_floats(int O, int I, int kh, int kw)
{
    if (O <= 0 || I <= 0 || kh <= 0 || kw <= 0) return 0;
    const size_t K = (size_t)I * kh * kw;
    return ((K + 31) / 32) * (size_t)((O + 31) / 32) * 1024 + femasr_compact_weight_floats(O, I, kh, kw);
}

int femasr_repack_oihw(void *stream, const float *in, int O, int I, int kh, int kw, float *out)
{
    FEMASR_REQUIRE(in && out && O > 0 && I > 0 && kh > 0 && kw > 0, "repack: bad args");
    if (kh == 1 && kw == 1 && (I % 32) == 0) return femasr_repack_k1((hipStream_t)stream, in, O, I, out);   // GEMM layout, same size
    const size_t tail = femasr_compact_weight_floats(O, I, kh, kw);
    const size_t total = femasr_packed_weight_floats(O, I, kh, kw) - tail;
    if (tail) {      // <= 4 output channels (out_conv): compact [k][4] copy behind the fragment-major matrix (direct VALU kernel)
        hipLaunchKernelGGL(repack_compact_kernel, dim3(grid_for(tail)), dim3(256), 0, (hipStream_t)stream, in, O, I, kh, kw, out + total, tail);
        FEMASR_CHECK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(repack_oihw_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, in, O, I, kh, kw, out,
                       total);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

size_t femasr_up2_weight_floats(int O, int I)
{
    return (I % 32) == 0 ? 4 * femasr_packed_weight_floats(O, I, 2, 2) : 0;
}

int femasr_repack_oihw_up2(void *stream, const float *in, int O, int I, float *out)
{
    FEMASR_REQUIRE(in && out && O > 0 && I > 0 && (I % 32) == 0, "repack_up2: needs a 3x3 OIHW weight with I %% 32 == 0");
    const size_t per = femasr_packed_weight_floats(O, I, 2, 2);
    hipLaunchKernelGGL(repack_up2_kernel, dim3(grid_for(4 * per)), dim3(256), 0, (hipStream_t)stream, in, O, I, out, per);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

int femasr_image_u8_to_f32(void *stream, const uint8_t *in_hwc, int H, int W, int swap_rb, float *out_chw)
{
    FEMASR_REQUIRE(in_hwc && out_chw && H > 0 && W > 0, "image_u8_to_f32: bad args");
    const size_t total = (size_t)3 * H * W;
    hipLaunchKernelGGL(image_u8_to_f32_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, in_hwc, H, W,
                       swap_rb, out_chw, total);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

int femasr_image_f32_to_u8(void *stream, const float *in_chw, int H, int W, int swap_rb, uint8_t *out_hwc)
{
    FEMASR_REQUIRE(in_chw && out_hwc && H > 0 && W > 0, "image_f32_to_u8: bad args");
    const size_t total = (size_t)3 * H * W;
    hipLaunchKernelGGL(image_f32_to_u8_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, in_chw, H, W,
                       swap_rb, out_hwc, total);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

int femasr_clock_probe_entries(void) { return FEMASR_CLOCK_PROBE_BLOCKS * 4; }      // what femasr_clock_probe writes: one tick count per wave

int femasr_clock_probe(void *stream, int mfmas_per_wave, unsigned long long *ticks)
{
    FEMASR_REQUIRE(ticks && mfmas_per_wave >= 4, "clock_probe: bad args");
    hipLaunchKernelGGL(clock_probe_kernel, dim3(FEMASR_CLOCK_PROBE_BLOCKS), dim3(256), 0, (hipStream_t)stream, mfmas_per_wave / 4, 1.0001f, 0.5f, ticks);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

}  // extern "C"

// ---- the conv forms: one row each, in ConvForm order (profile slots: the variants of the rows in this order)
namespace {

using Args = femasr_conv_args;
int gn_tiles_8x16(const Args *a) { return ((a->Ho + 7) / 8) * ((a->Wo + 15) / 16); }
// fp32 halo kernels: per 8x16 tile; an x2 conv (phase filters) per half-resolution tile and phase
int gn_tiles_direct(const Args *a)
{
    if (!femasr_conv_halo_eligible(a) || !femasr_gn_fusable(a->Cout)) return 0;
    return a->up2 ? 4 * ((a->H + 7) / 8) * ((a->W + 15) / 16) : gn_tiles_8x16(a);
}
int gn_tiles_mfma16(const Args *a) { return femasr_gn_fusable(a->Cout) && a->Cout <= 256 ? gn_tiles_8x16(a) : 0; }      // <= 8 channels per group
int gn_tiles_wino(const Args *a) { return femasr_conv_halo_eligible(a) && femasr_gn_fusable(a->Cout) ? femasr_conv_wino_gn_tiles(a->Ho, a->Wo) : 0; }
bool is_up2(const Args *a) { return a->up2 != 0; }
bool not_up2(const Args *a) { return !a->up2; }
bool is_k1(const Args *a) { return a->ksz == 1; }
bool not_k1(const Args *a) { return a->ksz != 1; }

// adapters to the columns' signatures (plain host functions: a lambda in a constant initialiser would be compiled for the device too)
int direct_launch(hipStream_t s, const Args *a, int *v, double *fl) { return femasr_conv2d_launch(s, a, nullptr, v, fl); }
size_t direct_bytes(int O, int I, int k) { return femasr_packed_weight_floats(O, I, k, k) * sizeof(float); }
int direct_repack(const float *w, int O, int I, int k, void *out) { return femasr_repack_oihw(nullptr, w, O, I, k, k, (float *)out); }
size_t bf16x3_bytes(int O, int I, int k) { return femasr_packed_weight_bf16x3_bytes(O, I, k, k); }
int bf16x3_repack(const float *w, int O, int I, int k, void *out) { return femasr_repack_oihw_bf16x3(nullptr, w, O, I, k, k, out); }
size_t wino_bytes(int O, int I, int) { return femasr_wino_weight_floats(O, I) * sizeof(float); }
int wino_repack(const float *w, int O, int I, int, void *out) { return femasr_repack_oihw_wino(nullptr, w, O, I, (float *)out); }
int wino_up2_count() { return 1; }
const char *wino_up2_name(int) { return femasr_conv_wino_up2_variant_name(); }
int wino_up2_pick(const Args *) { return 0; }
int wino_up2_launch(hipStream_t s, const Args *a, int *, double *fl) { return femasr_conv_wino_up2_launch(s, a, fl); }
size_t wino_up2_bytes(int O, int I, int) { return femasr_wino_up2_weight_floats(O, I) * sizeof(float); }
int wino_up2_repack(const float *w, int O, int I, int, void *out) { return femasr_repack_oihw_wino_up2(nullptr, w, O, I, (float *)out); }
// split form: the three bf16 planes of the (K x Cout) matrix, K = Cin (1x1 / nn.Linear) or 9 Cin (3x3)
int split_launch(hipStream_t s, const Args *a, int *v, double *fl) { return femasr_gemm_bf16s_launch(s, a, a->w_bf16s, v, fl); }
size_t split_bytes(int O, int I, int k) { return k == 1 ? femasr_packed_weight_bf16s_bytes(O, I) : femasr_packed_weight_conv3x3_bf16s_bytes(O, I); }
int split_repack(const float *w, int O, int I, int k, void *out) { return k == 1 ? femasr_repack_k1_bf16s(nullptr, w, O, I, out) : femasr_repack_oihw_bf16s(nullptr, w, O, I, out); }
size_t f16_bytes(int O, int I, int k) { return femasr_packed_weight_f16_bytes(O, I, k, k); }
int f16_repack(const float *w, int O, int I, int k, void *out) { return femasr_repack_oihw_f16(nullptr, w, O, I, k, k, out); }
size_t gemm_f16_bytes(int O, int I, int) { return femasr_packed_weight_k1_f16_bytes(O, I); }
int gemm_f16_repack(const float *w, int O, int I, int, void *out) { return femasr_repack_k1_f16(nullptr, w, O, I, out); }

}  // namespace

#define FORM_KERNELS(prefix) femasr_##prefix##_variant_count, femasr_##prefix##_variant_name, femasr_##prefix##_pick_variant
// (file-local: a constant with external linkage would be emitted for the device as well, host function pointers and all)
static const ConvFormDesc kConvForms[CONV_FORM_COUNT] = {
    {CONV_DIRECT, femasr_conv_variant_count, femasr_conv_variant_name, femasr_conv2d_pick_variant, direct_launch,
     offsetof(Args, w), direct_bytes, direct_repack, nullptr, 5, nullptr, nullptr, nullptr, gn_tiles_direct},
    {CONV_BF16X3, FORM_KERNELS(conv_bf16x3), femasr_conv_bf16x3_launch,
     offsetof(Args, w_bf16x3), bf16x3_bytes, bf16x3_repack, nullptr, 2, nullptr, femasr_conv_bf16x3_shape_ok,
     "conv2d: w_bf16x3 given but the layer is not eligible for the bf16x3 path", gn_tiles_mfma16},
    {CONV_WINO, FORM_KERNELS(conv_wino), femasr_conv_wino_launch,
     offsetof(Args, w_wino), wino_bytes, wino_repack, nullptr, 4, not_up2, femasr_conv_wino_shape_ok,
     "conv2d: w_wino given but the layer is not a 3x3 stride-1 pad-1 conv with Cin % 32 == 0, Cout % 64 == 0", gn_tiles_wino},
    {CONV_WINO_UP2, wino_up2_count, wino_up2_name, wino_up2_pick, wino_up2_launch,
     offsetof(Args, w_wino), wino_up2_bytes, wino_up2_repack, nullptr, 4, is_up2, femasr_conv_wino_up2_shape_ok,
     "conv2d: w_wino given with up2 but the layer is not a 3x3 stride-1 pad-1 conv with Cin % 32 == 0, Cout % 64 == 0, no prologue", gn_tiles_wino},
    {CONV_SPLIT, FORM_KERNELS(gemm_bf16s), split_launch,
     offsetof(Args, w_bf16s), split_bytes, split_repack, nullptr, 1, nullptr, femasr_gemm_bf16s_shape_ok,
     "conv2d: w_bf16s given but the layer is neither a 1x1 stride-1 layer nor a 3x3 pad-1 conv of stride 1 or 2, with Cin % 64 == 0 and no prologue", nullptr},
    {CONV_F16, FORM_KERNELS(conv_f16), femasr_conv_f16_launch,
     offsetof(Args, w_f16), f16_bytes, f16_repack, femasr_repack_packed_f16, 3, not_k1, femasr_conv_f16_shape_ok,
     "conv2d: w_f16 given but the layer is not eligible for the fp16 path (the bf16x3 shape rule)", gn_tiles_mfma16},
    {CONV_GEMM_F16, FORM_KERNELS(gemm_f16), femasr_gemm_f16_launch,
     offsetof(Args, w_f16), gemm_f16_bytes, gemm_f16_repack, femasr_repack_packed_k1_f16, 3, is_k1, femasr_gemm_f16_shape_ok,
     "conv2d: w_f16 given with ksz = 1 but the layer is not a 1x1 stride-1 layer with Cin % 64 == 0 and no prologue", nullptr},
};
#undef FORM_KERNELS
const ConvFormDesc &femasr_conv_form_desc(int f) { return kConvForms[f]; }

int femasr_conv_form_launch(hipStream_t s, ConvForm f, const femasr_conv_args *a, int *slot_out, double *flops_out)
{
    int v = 0;
    const int r = kConvForms[f].launch(s, a, &v, flops_out);
    for (int g = 0; g < f; ++g) v += kConvForms[g].variant_count();
    if (slot_out) *slot_out = v;
    return r;
}

// femasr_conv2d: the form whose weights are given (several: w_bf16s, then w_bf16x3, then w_f16, then w_wino - the rows' rank)
static ConvForm conv2d_form(const femasr_conv_args *a)
{
    ConvForm best = CONV_DIRECT;
    for (int f = 0; a && f < CONV_FORM_COUNT; ++f) {
        const ConvFormDesc &d = kConvForms[f];
        if (d.rank < kConvForms[best].rank && femasr_conv_form_image(f, a) && (!d.chosen || d.chosen(a))) best = (ConvForm)f;
    }
    return best;
}

extern "C" int femasr_debug_conv_variant_name(const femasr_conv_args *a, char *name, int cap)
{
    FEMASR_REQUIRE(a && name && cap > 0, "debug_conv_variant_name: bad args");
    // the shape checks of femasr_conv2d_launch that the variant rules divide by
    FEMASR_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0 && a->Cin > 0 && a->Cout > 0 && a->ksz >= 1 && a->ksz <= 11 &&
                   (a->stride == 1 || a->stride == 2 || a->stride == 4) && a->pad >= 0,
                   "debug_conv_variant_name: empty shape or unsupported ksz=%d stride=%d pad=%d", a->ksz, a->stride, a->pad);
    const ConvFormDesc &d = kConvForms[conv2d_form(a)];
    const char *s = d.variant_name(d.pick_variant(a));
    const size_t n = strlen(s);
    FEMASR_REQUIRE(n < (size_t)cap, "debug_conv_variant_name: the name needs %zu bytes, the buffer holds %d", n + 1, cap);
    memcpy(name, s, n + 1);
    return FEMASR_OK;
}

extern "C" int femasr_conv2d(void *stream, const femasr_conv_args *a)
{
    FEMASR_REQUIRE(!a || !a->in_add || (a->w_wino && a->up2 && !a->w_bf16x3 && !a->w_bf16s && !a->w_f16),
                   "conv2d: in_add is only taken by the x2 Winograd-type form (up2 = 1 with w_wino, no w_bf16x3 / w_bf16s / w_f16)");
    const ConvForm f = conv2d_form(a);
    FEMASR_REQUIRE(!kConvForms[f].shape_ok || kConvForms[f].shape_ok(a), "%s", kConvForms[f].refusal);
    return femasr_conv_form_launch((hipStream_t)stream, f, a, nullptr, nullptr);
}

// kernels_norm.hip — the normalisations: GroupNorm moments (row / tile partials, two finalizers), the stand-alone GN+SiLU apply, and
// LayerNorm (moments alone, or applied).  Reduction orders follow DESIGN.md "Arithmetic specification" (== the oracle's), so every
// kernel here is bit-reproducible and bit-identical to the CPU restatement.
#include "common.h"
#include "detmath.h"

namespace {

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

// (mean, biased variance) of a 256-float row from the lane's float4 of it: both kernels below, one operation order
__device__ __forceinline__ float2 ln_moments(const float4 &v)
{
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
    return float2{mean, wave_tree_sum(q) * (1.0f / 256.0f)};
}

__global__ void ln_stats_kernel(const float *__restrict__ x, long long rows, float eps, float *__restrict__ stats)
{
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float2 m = ln_moments(ld4(x + row * 256 + lane * 4));
    if (lane == 0) {
        stats[2 * row] = m.x;
        stats[2 * row + 1] = 1.0f / sqrtf(m.y + eps);
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
    const float2 m = ln_moments(v);
    const float mean = m.x, rstd = 1.0f / sqrtf(m.y + eps);
    const float4 g = ld4(gamma + lane * 4), b = ld4(beta + lane * 4);
    float4 o;
    o.x = __builtin_fmaf((v.x - mean) * rstd, g.x, b.x);
    o.y = __builtin_fmaf((v.y - mean) * rstd, g.y, b.y);
    o.z = __builtin_fmaf((v.z - mean) * rstd, g.z, b.z);
    o.w = __builtin_fmaf((v.w - mean) * rstd, g.w, b.w);
    *reinterpret_cast<float4 *>(y + row * 256 + lane * 4) = o;
}

}  // namespace

extern "C" {

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

}  // extern "C"

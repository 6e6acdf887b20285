// wino_common.h - what the two Winograd-form conv kernels share: kernels_wino.hip (F(4x4,3x3): 6 components per dimension, 36 products
// per 4x4 outputs) and kernels_wino_up2.hip (Upsample(x2) + conv: 5 per dimension, 25 products).  Both: block = 8 waves, two 16x16-pixel
// OUTPUT sub-blocks (consecutive in (n, y, x) order; 2 x 16 Winograd tiles = ONE 32-row MFMA tile) x 64 output channels, K in steps of
// 8 input channels, one barrier per step.  Here: the launch parameters, the LDS geometry, the 1-D transforms, the weight repack, the
// host helpers and WinoFrame - the block decode, the output descriptors, the accumulator-tile store and the GroupNorm reduction.  Per
// kernel: patch staging, the input transform, the M-phase pair ownership with its U-fragment ring, the prologue order, the step body
// and the loop that writes the accumulators out.  The U-fragment load and the epilogue's border masks, `fetch` and `round` are the
// same text in both kernels (6 / 5 components, H, W / Ho, Wo): as shared functions they cost SGPR spills and VGPRs, or changed an
// MFMA-loop sequence (profiles/wino_frame_isa_diff.txt).
//
// The epilogue, one 32-column tile (round) at a time: accumulators ->
// Mx[component][tile pair][channel][2] (overlays the main-loop buffers; rows e, e + 1 of an accumulator tile are two horizontally
// adjacent Winograd tiles and sit in an aligned register pair: one ds_write_b64, store_acc_tile).  A thread = (tile pair pi =
// (sub-block, tile row, left / right half), channel c31) handles BOTH tiles at once: one ds_read_b64 per component, and every operation
// of the output transform (at6 / at5, applied twice), the bias / residual adds and the moment sums is a packed fp32 instruction over the
// pair (component-wise IEEE: the same values as two scalar sequences).  Outputs and residuals go through buffer instructions:
// descriptors in SGPRs (base = the image of sub-block 0), ONE 32-bit byte offset per lane, a uniform offset per pixel and tile of the
// pair; in a block whose 32 tiles lie wholly inside the image (FULL, the common case) nothing is masked; otherwise a pixel outside gets
// an offset beyond num_records (stores dropped, loads return 0).
// GroupNorm partial moments of what was stored (orc_gn_wino_partial; orc_gn_coeffs mode 2): per (tile, channel) an fp32 sum and an fp32
// fma chain of squares over the 16 pixels (row-major, a pixel outside adds +0), then fp64: the two tiles of the pair, the channels of
// the group (xor butterfly), the two pairs of the tile row, then the four tile rows (= waves) of the sub-block in order.
//
// Round 4's second block shape (16x16 pixels x 128 channels, kernels_wino_c128.hip: 7 % fewer cycles, 3 % more time at the 1400 W
// package limit) was removed in round 6; git history and profiles/r04_j_* have it.
// The including file defines FEMASR_WTT_BUF (the name of its cycle-stamp buffer) first.
#pragma once
#include "conv_common.h"
#include "detmath.h"
#include <stdlib.h>
#include <type_traits>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
typedef float tf2 __attribute__((ext_vector_type(2)));

#ifdef FEMASR_WINO_TT      // tools/build_debug.sh tt: cycle stamps (s_memtime) of waves 0 and 7 of every block, written straight to a global
// buffer [block][wave 0 | 7][128] - no accumulators in registers, one scalar read + one 8-byte store per stamp.  Slots: 63 block start,
// 0 prologue done, 16 + s main-loop step s done (s < 40), 1 main loop done, per epilogue round r: 2 + 4r accumulators in LDS,
// 3 + 4r residuals requested + barrier passed, 4 + 4r round computed / stored, 5 + 4r second barrier; 10 end; F(4x4) only, inside step
// s < 24: 64 + 2s M phase issued (+ hoisted transform reads), 65 + 2s T phase done (before the barrier).
__device__ unsigned long long *FEMASR_WTT_BUF;
#define WTT(slot) { if (lane == 0 && (wave == 0 || wave == 7)) FEMASR_WTT_BUF[((size_t)blockIdx.x * 2 + (wave == 7 ? 1 : 0)) * 128 + (slot)] = __builtin_readcyclecounter(); }
#define WTTR(slot) { if (lane == 0 && (wave == 0 || wave == 7)) FEMASR_WTT_BUF[((size_t)blockIdx.x * 2 + (wave == 7 ? 1 : 0)) * 128 + (slot)] = wall_clock64(); }
#define WTT_INIT { WTTR(62) WTT(63) }
#define WTT_END { WTT(10) WTTR(11) }
#else
#define WTT(slot) {}
#define WTT_INIT
#define WTT_END {}
#endif

namespace {

struct WinoParams {
    const float *in, *u, *bias, *res1, *res2;
    float *out;
    double *gn_part;
    int B, H, W, Cin, Cout;             // H, W: input
    int sbX, sbY, nsb;                  // 16x16-pixel output sub-blocks per row / per column / in the batch
    int MB, NB, nsteps, NT32;
    int Ho, Wo;                         // output: H, W (F(4x4) form) or 2H, 2W (x2 form)
    const float *in2;                   // x2 form: optional second input, added to `in` while staging (femasr_conv_args.in_add)
    const float *pro_a, *pro_b;         // F(4x4) form: GroupNorm coefficients of the prologue
};

constexpr int WINO_NT = 512;
constexpr int WINO_RED = 8 * 2 * 16 * 2 * 2;                      // floats: [8 waves][2 sub-blocks][<= 16 groups][2] doubles
constexpr int WINO_MAX_CIN = 1024;                                // femasr_conv_wino*_shape_ok
constexpr int wino_vsz(int nv) { return nv * 32 * 8; }            // floats per V buffer of nv transformed values: [nv][32 tiles][8 channels]
constexpr int wino_mx(int n) { return n * n * 32 * 32; }          // epilogue: one 32-column tile of all n x n components

// patch geometry of the F(4x4,3x3) form: 18x18 pixels per sub-block
constexpr int W4_PS = 10;                         // floats per patch pixel: 8 channels + 2 (tiles 4 pixels apart land 8 banks apart)
constexpr int W4_PW = 18;
constexpr int W4_PPIX = W4_PW * W4_PW;            // 324
constexpr int W4_PSZ = 2 * W4_PPIX * W4_PS;       // floats per patch buffer (two sub-blocks)
constexpr int W4_VSZ = wino_vsz(36);
constexpr int W4_MAIN = 2 * W4_PSZ + 2 * W4_VSZ;  // main-loop floats ahead of the GN coefficient table
constexpr int W4_UNITS_SB = W4_PPIX * 2;          // float4 staging units per sub-block and step (648)
// ... and of the x2 form: the 10x10 low-resolution patch of a sub-block (8x8 + halo)
constexpr int WU_PS = 12;                         // floats per patch pixel: 8 channels + 4
constexpr int WU_PW = 10;
constexpr int WU_PPIX = WU_PW * WU_PW;            // 100
constexpr int WU_PSZ = 2 * WU_PPIX * WU_PS;       // floats per patch buffer (two sub-blocks): 2400
constexpr int WU_VSZ = wino_vsz(16);              // the 16 DISTINCT transformed values (components P and Q share v3)
constexpr int WU_MAIN = 2 * WU_PSZ + 2 * WU_VSZ;
constexpr int WU_UNITS = 2 * WU_PPIX * 2;         // float4 staging units per step: 400

// n: components per dimension; main_f: main-loop floats of the form; gn_cin: channels of the GN coefficient table behind them (or 0)
constexpr size_t wino_lds_bytes(int n, int main_f, int gn_cin)
{
    const size_t m = (size_t)main_f + 4 * (size_t)gn_cin, epi_f = (size_t)wino_mx(n) + WINO_RED;
    return (m > epi_f ? m : epi_f) * sizeof(float);
}
static_assert(wino_lds_bytes(6, W4_MAIN, WINO_MAX_CIN) <= 160 * 1024 && wino_lds_bytes(5, WU_MAIN, 0) <= 160 * 1024,
              "the largest request of either form (F(4x4): GN table of WINO_MAX_CIN channels) must fit the CU's 160 KiB of LDS");

// 6-point transforms of F(4x4,3x3).  Input rows of B^T (Lavin & Gray), written so that each value is one fixed sequence of
// IEEE operations (the oracle restates them literally):
//   r0 = 4 d0 - 5 d2 + d4          r1 = (d4 - 4 d2) + (d3 - 4 d1)      r2 = (d4 - 4 d2) - (d3 - 4 d1)
//   r3 = (d4 - d2) + 2 (d3 - d1)   r4 = (d4 - d2) - 2 (d3 - d1)        r5 = 4 d1 - 5 d3 + d5
__device__ __forceinline__ void bt_lo(float d0, float d1, float d2, float d3, float d4, float &r0, float &r1, float &r2)
{
    r0 = __builtin_fmaf(4.0f, d0, __builtin_fmaf(-5.0f, d2, d4));
    const float a = __builtin_fmaf(-4.0f, d2, d4), b = __builtin_fmaf(-4.0f, d1, d3);
    r1 = a + b;
    r2 = a - b;
}
__device__ __forceinline__ void bt_hi(float d1, float d2, float d3, float d4, float d5, float &r3, float &r4, float &r5)
{
    const float c = d4 - d2, e = d3 - d1;
    r3 = __builtin_fmaf(2.0f, e, c);
    r4 = __builtin_fmaf(-2.0f, e, c);
    r5 = __builtin_fmaf(4.0f, d1, __builtin_fmaf(-5.0f, d3, d5));
}
// output rows of A^T:  y0 = (m0 + (m1 + m2)) + (m3 + m4),  y1 = (m1 - m2) + 2 (m3 - m4),  y2 = (m1 + m2) + 4 (m3 + m4),
//                      y3 = ((m1 - m2) + 8 (m3 - m4)) + m5
// (on PAIRS: v_pk_add_f32 / v_pk_fma_f32 are IEEE per component)
__device__ __forceinline__ void at6(tf2 m0, tf2 m1, tf2 m2, tf2 m3, tf2 m4, tf2 m5, tf2 &y0, tf2 &y1, tf2 &y2, tf2 &y3)
{
    const tf2 pp = m1 + m2, qq = m1 - m2, rr = m3 + m4, ss = m3 - m4;
    y0 = (m0 + pp) + rr;
    y1 = __builtin_elementwise_fma(tf2{2.0f, 2.0f}, ss, qq);
    y2 = __builtin_elementwise_fma(tf2{4.0f, 4.0f}, rr, pp);
    y3 = __builtin_elementwise_fma(tf2{8.0f, 8.0f}, ss, qq) + m5;
}
// output rows of the x2 form's 5 -> 4 transform (kernels_wino_up2.hip, header), on pairs like at6
__device__ __forceinline__ void at5(tf2 m0, tf2 m1, tf2 mP, tf2 mQ, tf2 m5, tf2 &y0, tf2 &y1, tf2 &y2, tf2 &y3)
{
    y0 = (m0 + m1) + mP;
    y1 = __builtin_elementwise_fma(tf2{2.0f, 2.0f}, mQ, m1);
    y2 = __builtin_elementwise_fma(tf2{4.0f, 4.0f}, mP, m1);
    y3 = __builtin_elementwise_fma(tf2{8.0f, 8.0f}, mQ, m1) + m5;
}

// 1-D filter transforms, rows (over ky) then columns (over kx), each one fixed sequence of IEEE operations.  F(4x4,3x3), G g G^T:
//   u0 = g0 * 0.25     u1 = ((g0 + g1) + g2) * (-1/6)     u2 = ((g0 - g1) + g2) * (-1/6)
//   u3 = fma(4, g2, fma(2, g1, g0)) * (1/24)     u4 = fma(4, g2, fma(-2, g1, g0)) * (1/24)     u5 = g2
__device__ __forceinline__ float wino_g6(int r, float g0, float g1, float g2)
{
    const float c6 = -1.0f / 6.0f, c24 = 1.0f / 24.0f;
    switch (r) {
    case 0: return g0 * 0.25f;
    case 1: return ((g0 + g1) + g2) * c6;
    case 2: return ((g0 - g1) + g2) * c6;
    case 3: return __builtin_fmaf(4.0f, g2, __builtin_fmaf(2.0f, g1, g0)) * c24;
    case 4: return __builtin_fmaf(4.0f, g2, __builtin_fmaf(-2.0f, g1, g0)) * c24;
    default: return g2;
    }
}
// the five filters e0, e1, eP, eQ, e5 of the x2 form (kernels_wino_up2.hip, header)
__device__ __forceinline__ float e5(int r, float g0, float g1, float g2)
{
    const float c3 = -1.0f / 3.0f, c12 = 1.0f / 12.0f, c6 = 1.0f / 6.0f;
    switch (r) {
    case 0: return g0 * 0.25f;
    case 1: return ((g0 + g1) + g2) * c3;
    case 2: return __builtin_fmaf(4.0f, g2, __builtin_fmaf(4.0f, g1, g0)) * c12;
    case 3: return __builtin_fmaf(4.0f, g2, g0 + g1) * c6;
    default: return g2;
    }
}

// The part of a block both kernels share (header): block decode, output descriptors, accumulator-tile store, GroupNorm reduction.
// The members are plain values the kernels copy into locals.
struct WinoFrame {
    int t, lane, wave, c31, hh, nb, mb, n0;
    int sn[2], sy0[2], sx0[2], sbi[2];       // the two sub-blocks (uniform): image, origin in the output, index inside the image
    bool sval[2];
    __amdgpu_buffer_rsrc_t rs_out, rs_r1, rs_r2;

    __device__ __forceinline__ explicit WinoFrame(const WinoParams &p)
    {
        t = threadIdx.x, lane = t & 63;
        wave = __builtin_amdgcn_readfirstlane(t >> 6);
        WTT_INIT
        c31 = lane & 31, hh = lane >> 5;
        const int L = xcd_remap(blockIdx.x, p.MB * p.NB);
        nb = L % p.NB, mb = L / p.NB;
        n0 = nb * 64;
#pragma unroll
        for (int z = 0; z < 2; ++z) {
            const int sb = 2 * mb + z, per = p.sbY * p.sbX;
            sval[z] = sb < p.nsb;
            const int sbc = sval[z] ? sb : 0;
            sn[z] = sbc / per;
            sbi[z] = sbc - sn[z] * per;
            const int by = sbi[z] / p.sbX, bx = sbi[z] - by * p.sbX;
            sy0[z] = 16 * by;
            sx0[z] = 16 * bx;
        }
    }

    // descriptors of the output and the residual operands: base = the image of sub-block 0 (an absent operand aliases the output)
    template <int NRES>
    __device__ __forceinline__ void out_descriptors(const WinoParams &p)
    {
        const size_t img0 = (size_t)sn[0] * p.Ho * p.Wo * p.Cout;
        rs_out = __builtin_amdgcn_make_buffer_rsrc((void *)(p.out + img0), 0, 0x7fffffff, 0x00020000);
        rs_r1 = __builtin_amdgcn_make_buffer_rsrc((void *)((NRES >= 1 ? p.res1 : p.out) + img0), 0, 0x7fffffff, 0x00020000);
        rs_r2 = __builtin_amdgcn_make_buffer_rsrc((void *)((NRES >= 2 ? p.res2 : p.out) + img0), 0, 0x7fffffff, 0x00020000);
    }

    // one accumulator tile -> Mx: pair row ((e & 3) + 8 (e >> 2) + 4 hh) / 2, 256 bytes each
    static __device__ __forceinline__ void store_acc_tile(char *dst, const f32x16 &a)
    {
#pragma unroll
        for (int e = 0; e < 16; e += 2) *reinterpret_cast<tf2 *>(dst + (((e & 3) >> 1) + 4 * (e >> 2)) * 256) = tf2{a[e], a[e + 1]};
    }

    // behind the barrier that follows round r: the four tile rows (= waves) of each sub-block in order -> gn_part
    // (cg: channels per GroupNorm group, gpt: groups per 32-channel tile)
    __device__ __forceinline__ void gn_reduce(const WinoParams &p, const double *red, int cg, int gpt, int r) const
    {
        if (p.gn_part != nullptr && t < 2 * gpt) {
            const int z = t / gpt, gl = t - z * gpt;
            if (z ? sval[1] : sval[0]) {
                double S = red[((size_t)(4 * z) * 16 + gl) * 2], SS = red[((size_t)(4 * z) * 16 + gl) * 2 + 1];
#pragma unroll
                for (int w = 1; w < 4; ++w) {
                    S = S + red[((size_t)(4 * z + w) * 16 + gl) * 2];
                    SS = SS + red[((size_t)(4 * z + w) * 16 + gl) * 2 + 1];
                }
                const int g = (n0 + 32 * r) / cg + gl;
                double *dst = p.gn_part + (((size_t)(z ? sn[1] : sn[0]) * p.sbY * p.sbX + (z ? sbi[1] : sbi[0])) * 32 + g) * 2;
                dst[0] = S;
                dst[1] = SS;
            }
        }
    }
};

// 3x3 OIHW -> out[step = ci/8][component N i + j][32-column tile][lane][e]: column o = 32 tile + lane%32,
// ci = 8 step + 2 e + lane/32 (the B fragments of the four k-pairs of a step: one 16-byte load per lane, 1 KiB per wave)
typedef float (*wino_filter_t)(int, float, float, float);
template <int N, wino_filter_t G>
__global__ void repack_wino_kernel(const float *__restrict__ in, int O, int I, float *__restrict__ out, size_t total)
{
    const int NT32 = (O + 31) / 32;
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int e = (int)(idx & 3), lane = (int)((idx >> 2) & 63);
        size_t rest = idx >> 8;
        const int ntile = (int)(rest % NT32);
        rest /= NT32;
        const int comp = (int)(rest % (N * N)), step = (int)(rest / (N * N));
        const int ci = 8 * step + 2 * e + (lane >> 5), o = ntile * 32 + (lane & 31);
        float v = 0.f;
        if (ci < I && o < O) {
            const int i = comp / N, j = comp - N * i;
            const float *gw = in + ((size_t)o * I + ci) * 9;
            float ur[3];
#pragma unroll
            for (int x = 0; x < 3; ++x) ur[x] = G(i, gw[x], gw[3 + x], gw[6 + x]);
            v = G(j, ur[0], ur[1], ur[2]);
        }
        out[idx] = v;
    }
}

inline size_t wino_weight_floats(int n, int O, int I) { return (I % 32) == 0 ? (size_t)(I / 8) * n * n * ((O + 31) / 32) * 256 : 0; }

template <int N, wino_filter_t G>
inline int wino_repack(void *stream, const float *in, int O, int I, float *out, const char *who)
{
    FEMASR_REQUIRE(in && out && O > 0 && I > 0 && (I % 32) == 0, "%s: needs a 3x3 OIHW weight with I %% 32 == 0", who);
    const size_t total = wino_weight_floats(N, O, I);
    size_t blocks = (total + 255) / 256;
    if (blocks > 65535) blocks = 65535;
    hipLaunchKernelGGL((repack_wino_kernel<N, G>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, in, O, I, out, total);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

// The shape test both forms share.  n: components per dimension; os: output-size factor per dimension (1, or 2 for the x2 form).
// Element limits (32-bit byte offsets): 2^31 elements per tensor, 2^27 per image by default.  A handle may LOWER them for its planner
// (femasr_debug_set_wino_limits, include/femasr_hip_debug.h: tests of both sides of the limit at sizes they can allocate).
inline bool wino_shape_ok(const femasr_conv_args *a, int n, int os, int log2_total, int log2_image)
{
    const size_t tot = (size_t)1 << log2_total, img = (size_t)1 << log2_image, opix = (size_t)os * os * a->H * a->W;
    return a->ksz == 3 && a->stride == 1 && a->pad == 1 && a->act == FEMASR_ACT_NONE && (a->Cin % BK) == 0 && a->Cin <= WINO_MAX_CIN &&
           (a->Cout % 64) == 0 && (size_t)a->B * a->H * a->W * a->Cin < tot && (size_t)a->B * opix * a->Cout < tot &&
           (size_t)a->H * a->W * a->Cin < img &&          // two images within the 2 GiB range of the input descriptor
           opix * a->Cout < img &&                        // ... and of the output / residual descriptors
           (size_t)n * n * a->Cin * a->Cout < ((size_t)1 << 29);
}

// The launch checks and parameter fields both forms share (who: the form's name in error messages); Ho, Wo are the caller's
inline int wino_params(const femasr_conv_args *a, const char *who, WinoParams &p)
{
    FEMASR_REQUIRE(!a->gn_part || femasr_gn_fusable(a->Cout), "%s: gn_part needs 32 | Cout and Cout/32 a power of two <= 32", who);
    FEMASR_REQUIRE(a->res1 || !a->res2, "%s: res2 without res1", who);
    p.in = a->in; p.in2 = a->in_add; p.u = (const float *)a->w_wino; p.bias = a->bias; p.pro_a = a->pro_a; p.pro_b = a->pro_b;
    p.res1 = a->res1; p.res2 = a->res2; p.out = a->out; p.gn_part = a->gn_part;
    p.B = a->B; p.H = a->H; p.W = a->W; p.Cin = a->Cin; p.Cout = a->Cout; p.Ho = a->Ho; p.Wo = a->Wo;
    p.sbX = (a->Wo + 15) / 16;
    p.sbY = (a->Ho + 15) / 16;
    p.nsb = a->B * p.sbX * p.sbY;
    p.MB = (p.nsb + 1) / 2;
    p.NB = a->Cout / 64;
    p.nsteps = a->Cin / 8;
    p.NT32 = a->Cout / 32;
    return FEMASR_OK;
}

}  // namespace

// Schedule variants built and A/B-measured in round 4 (all bit-identical; profiles/r04_wino_variants.txt), removed again except the two
// marked kept.  F(4x4) kernel unless the x2 kernel is named; what was measured on both is listed once:
//   * the patch of step s+2 requested at the start of the M phase instead of at pair 5: 4 % SLOWER - loads return in order, the slow HBM
//     request ahead of the L2-resident U fragments delays them;
//   * staging ahead of the transform arithmetic (its LDS reads in flight meanwhile): 0 .. +1 %;
//   * the transform's patch reads at the start of the M phase, or the whole transform inside the M phase: +-1 % (both kernels);
//   * the input transform on (tile, channel PAIR) items - both passes packed, 72 instead of 2 x 57 instructions per SIMD and step, but
//     only on waves 0-3: 2 - 9 % SLOWER: one wave's VALU stream alone does not reach the issue rate two interleaved waves do;
//   * prologue: every global request first, the patches of steps 0 and 1 requested together (second register set): 1 % faster - kept;
//   * the second register set also used in the main loop - kept (both kernels), see the main loop;
//   * the nt cache-policy bit on the streaming accesses: 5 - 18 % SLOWER on the input patches, +-2 % on the residual loads / output
//     stores (both kernels; profiles/r04_i_wino_nt.txt);
//   * ablation builds (no patch loads, no U loads, no transform, no MFMAs, no output items, no activation, no staging stores; timings
//     only, results garbage) gave the per-phase costs quoted in the kernels' comments.

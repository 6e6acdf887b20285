// gemm_common.h - what the three row GEMMs share:   out[M][N] = epi( A[M][K] . W[K][N] )
//   kernels_gemm.hip       gemm_dma_kernel     fp32 chain on the fp32 MFMA, both operands by LDS-DMA (and the VQ first-min epilogue)
//   kernels_gemm_bf16.hip  gemm_bf16s_kernel   exact three-term bf16 split, six products, two accumulators; also the 3x3 conv form
//   kernels_gemm_f16.hip   gemm_f16_kernel     one fp16 pass
// All three: block = 256 threads = 4 waves in 2 x 2, each wave WT x WT accumulator tiles of 32 x 32 (block tile 64 WT x 64 WT), weights
// packed per 32-column tile.  Here: the launch parameters, GemmFrame (the block decode), the store epilogue, the decode of the
// fragment-major weight images, and the host side (variant row, argument checks, launch).  Per kernel: the main loop - operand staging,
// waits, MFMA order -, the packed weight layout, the VQ epilogue of gemm_dma_kernel and the split form's copy of the store epilogue.
//
// THE STORE EPILOGUE, the one description of what a GEMM layer stores:
//     out[row][col] = act(x + bias[col]) + res1[row][col] + res2[row][col]        fp32, in exactly this order (bit-exact contract)
//   * x is the tile element the kernel's functor yields: acc (fp32, fp16 forms) or hi + lo (split form), added to the bias afterwards;
//   * act = exact-erf GELU or nothing: det_gelu2 (two values per packed instruction) on the vector path, det_gelu on the scalar path -
//     the same value per element;
//   * NRES operands are added: ra = the first non-null of (res1, res2), then rb = res2 when both are set;
//   * a null bias (NULL_BIAS forms only: fp16) still ADDS +0.0f, so that -0.0 + 0.0 stays +0.0 as in the oracle;
//   * vector path (N % 4 == 0): each 32 x 32 accumulator tile is transposed through the wave's own LDS scratch (TSCRATCH floats at
//     lds + wave * TSCRATCH, overlaying the dead main-loop buffers) so that lane l owns columns 4 (l & 7) .. + 3 of tile rows
//     (l >> 3) + 8 k: float4 bias / residual loads and float4 stores.  A lane whose column or row lies outside stores nothing and reads
//     bias column 0 / residual element 0 instead of its own address: no access leaves the operands;
//   * scalar path (N % 4 != 0): every lane stores its own accumulator elements, guarded by row < M and col < N, loads inside the guard.
// Two copies of it exist.  gemm_store_epilogue (below; fp32 and fp16 forms) requests the bias and the residual rows of a tile when the tile
// is processed; the caller has passed the barrier behind which the main-loop LDS buffers are dead.  gemm_bf16s_kernel keeps its own text,
// the same arithmetic in another FETCH ORDER: the bias of both column tiles and the residual rows of tile 0 are requested before the
// block's last barrier, the residual rows of tile t + 1 before tile t is processed (one exposed round trip per block instead of one per
// tile).  As a policy of this function that order compiled to other VGPR counts (+14 in three instantiations) and another MFMA-loop
// schedule in three to six of the nine split kernels - the loop's scheduling follows the register pressure of the whole kernel -, in
// every way of passing the state that was tried (profiles/gemm_frame_isa_diff.txt).  A change to one copy is a change to both.
#pragma once
#include "conv_common.h"
#include "detmath.h"
#include <stdlib.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

// The fields every form reads; the fp32 and split forms extend them (GemmDmaParams, GemmSParams)
struct GemmParams {
    const float *A;
    const void *W;               // the form's packed image (femasr_repack_k1, femasr_repack_k1_bf16s / _oihw_bf16s, femasr_repack_k1_f16)
    const float *bias, *res1, *res2;
    float *out;
    int M, N, K, MB, NB, NT32;
};

// The block decode.  bt: the block tile (rows = columns).  The members are plain values the kernels copy into locals.
struct GemmFrame {
    int t, lane, wave, wm, wn;          // wave: uniform; (wm, wn): its place in the 2 x 2 wave grid
    int nb, mb, m0, n0;                 // block column / row (XCD-remapped), first row / column
    int h, c31;                         // lane >> 5, lane & 31: the MFMA fragment coordinates

    __device__ __forceinline__ GemmFrame(int MB, int NB, int bt)
    {
        t = threadIdx.x, lane = t & 63;
        wave = __builtin_amdgcn_readfirstlane(t >> 6);
        wm = wave >> 1, wn = wave & 1;
        const int L = xcd_remap(blockIdx.x, MB * NB);
        nb = L % NB, mb = L / NB;
        m0 = mb * bt, n0 = nb * bt;
        h = lane >> 5, c31 = lane & 31;
    }
};

// elem(i, j, r): element r of the wave's accumulator tile (i, j); lds: the block's LDS base (see the header for everything else)
template <int WT, int ACT, int NRES, bool NULL_BIAS, class Elem>
__device__ __forceinline__ void gemm_store_epilogue(const GemmParams &p, const GemmFrame &f, float *lds, Elem elem)
{
    const int m0 = f.m0, n0 = f.n0, wm = f.wm, wn = f.wn, h = f.h, c31 = f.c31;
    float *T = lds + f.wave * TSCRATCH;
    const int trow = f.lane >> 3, tq = f.lane & 7;
    const float *ra = p.res1 ? p.res1 : p.res2, *rb = (p.res1 && p.res2) ? p.res2 : nullptr;
    const bool vec = (p.N & 3) == 0;
    f32x4_t r1[4] = {}, r2[4] = {};
    auto fetch_bias = [&](int j) {
        const int col = n0 + (wn * WT + j) * 32 + 4 * tq;
        f32x4_t b4 = {0.f, 0.f, 0.f, 0.f};
        if (!NULL_BIAS || p.bias) b4 = *reinterpret_cast<const f32x4_t *>(p.bias + (col < p.N ? col : 0));
        return b4;
    };
    auto fetch_res = [&](int tl) {
        if (NRES == 0 || !vec) return;
        const int rbase = m0 + (wm * WT + tl / WT) * 32, col = n0 + (wn * WT + tl % WT) * 32 + 4 * tq;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int row = rbase + trow + 8 * k;
            const size_t o = (col < p.N && row < p.M) ? (size_t)row * p.N + col : 0;
            r1[k] = *reinterpret_cast<const f32x4_t *>(ra + o);
            if (NRES >= 2) r2[k] = *reinterpret_cast<const f32x4_t *>(rb + o);
        }
    };
#pragma unroll
    for (int tl = 0; tl < WT * WT; ++tl) {
        const int i = tl / WT, j = tl % WT;
        const int rbase = m0 + (wm * WT + i) * 32, cbase = n0 + (wn * WT + j) * 32;
        if (vec) {
            const int col = cbase + 4 * tq;
            const bool cok = col < p.N;
            fetch_res(tl);
#pragma unroll
            for (int r = 0; r < 16; ++r) T[((r & 3) + 8 * (r >> 2) + 4 * h) * TPITCH + c31] = elem(i, j, r);
            const f32x4_t b4 = fetch_bias(j);
            // (same wave wrote and reads the scratch: LDS ops of one wave complete in order)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const f32x4_t a4 = *reinterpret_cast<const f32x4_t *>(T + (trow + 8 * k) * TPITCH + 4 * tq);
                float v[4] = {a4[0] + b4[0], a4[1] + b4[1], a4[2] + b4[2], a4[3] + b4[3]};
                if (ACT == FEMASR_ACT_GELU) {         // two at a time on the packed fp32 ALU (bit-identical per element)
                    const det_f32x2 g0 = det_gelu2(det_f32x2{v[0], v[1]}), g1 = det_gelu2(det_f32x2{v[2], v[3]});
                    v[0] = g0[0]; v[1] = g0[1]; v[2] = g1[0]; v[3] = g1[1];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (NRES >= 1) v[e] = v[e] + r1[k][e];
                    if (NRES >= 2) v[e] = v[e] + r2[k][e];
                }
                const int row = rbase + trow + 8 * k;
                if (cok && row < p.M) *reinterpret_cast<f32x4_t *>(p.out + (size_t)row * p.N + col) = f32x4_t{v[0], v[1], v[2], v[3]};
            }
        } else {
            const int col = cbase + c31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rbase + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (row < p.M && col < p.N) {
                    const size_t o = (size_t)row * p.N + col;
                    float v = elem(i, j, r) + ((!NULL_BIAS || p.bias) ? p.bias[col] : 0.f);
                    if (ACT == FEMASR_ACT_GELU) v = det_gelu(v);
                    if (NRES >= 1) v = v + ra[o];
                    if (NRES >= 2) v = v + rb[o];
                    p.out[o] = v;
                }
            }
        }
    }
}

// Fragment-major weight images of the bf16 / fp16 MFMAs, [k step][n / 32][lane] x 8 values (split form: x 3 planes): item -> its place.
// lane (j = lane & 31, h = lane >> 5) holds k = k0 .. k0 + 7, k0 = 16 step + 8 h, of column n = 32 (n / 32) + j.
struct FragItem {
    int lane, n, k0;
    size_t tile;        // step * NT32 + n / 32
};
__device__ __forceinline__ FragItem frag_item(size_t item, int NT32)
{
    const int lane = (int)(item & 63);
    const size_t tile = item >> 6;
    const int nt = (int)(tile % NT32), st = (int)(tile / NT32);
    return {lane, 32 * nt + (lane & 31), 16 * st + 8 * (lane >> 5), tile};
}

// Host side.  A row of a form's variant table ...
template <class Params>
struct GemmVariant {
    const char *name;
    void (*kern)(const Params);
    int lds;                            // dynamic LDS bytes
    unsigned long long attr_devs;       // bit d: MaxDynamicSharedMemorySize set on device d
};

// ... the argument checks and parameter fields the forms share (who: the form's name in error messages; Ho, Wo, K: what the form
// computes from *a) ...
inline int gemm_params(const femasr_conv_args *a, const char *who, int Ho, int Wo, int K, GemmParams &p)
{
    FEMASR_REQUIRE(a->act == FEMASR_ACT_NONE || a->act == FEMASR_ACT_GELU, "%s: bad activation %d", who, a->act);
    const long long M = (long long)a->B * Ho * Wo;
    FEMASR_REQUIRE(a->Ho == Ho && a->Wo == Wo, "%s: Ho/Wo mismatch", who);
    FEMASR_REQUIRE(M > 0 && M < (1ll << 31) - 256, "%s: bad row count", who);
    p.A = a->in; p.bias = a->bias; p.res1 = a->res1; p.res2 = a->res2; p.out = a->out;
    p.M = (int)M; p.N = a->Cout; p.K = K;
    p.NT32 = (p.N + 31) / 32;
    return FEMASR_OK;
}

// ... and the launch of row vi with block tile bt
template <class Params, int N>
int gemm_variant_launch(hipStream_t s, GemmVariant<Params> (&table)[N], int vi, int bt, Params &p, int *variant_out, double *flops_out)
{
    GemmVariant<Params> &v = table[vi];
    p.MB = (p.M + bt - 1) / bt; p.NB = (p.N + bt - 1) / bt;
    FEMASR_CHECK(femasr_allow_dynamic_lds((const void *)v.kern, &v.attr_devs, (size_t)v.lds));
    hipLaunchKernelGGL(v.kern, dim3((unsigned)(p.MB * p.NB)), dim3(256), (size_t)v.lds, s, p);
    FEMASR_CHECK_HIP(hipGetLastError());
    if (variant_out) *variant_out = vi;
    if (flops_out) *flops_out = 2.0 * (double)p.M * (double)p.N * (double)p.K;
    return FEMASR_OK;
}

}  // namespace

// kernels_conv_f16.hip — 3x3 halo convolution on the fp16 matrix cores, ONE pass (decoder_math 'fp16', C ABI mode 4).
//
// Where it is used: the same layers as the bf16x3 path (kernels_conv_bf16.hip) - the convs BEHIND every codebook lookup with
// Cout > 4, under the same shape rule - and only when the caller opts in (femasr_set_decoder_math(4)).  They cannot move a VQ
// index, so the indices stay identical to every other mode; the IMAGE is half-precision grade (NOT within the 1e-3 bound of
// the fp32-grade modes; DESIGN.md "decoder_math='fp16'").
//
// Arithmetic (include/femasr_hip.h, femasr_conv_args.w_f16):
//   t   = activated input in fp32 (GroupNorm apply + hardware-unit SiLU as in the bf16x3 prologue, nearest-x2 folded into the
//         patch indexing, zero outside the image)
//   t16 = fp16_rne(clamp(t, +-65504))            (a finite input never becomes Inf)
//   w16 = fp16_rne(w), packed once by femasr_repack_oihw_f16
//   products t16 * w16 are exact in fp32 (11 + 11 significand bits), accumulated in fp32 by v_mfma_f32_32x32x16_f16;
//   bias and residuals are added in fp32 (the accumulators start from them); activations stay fp32 in memory.
//
// Structure = the bf16x3 kernel's, on the frame both share (halo_mma.h): 8x16 output pixels x BN channels per block, one halo patch
// per 32-channel block staged once and swept by nine taps, fragment-major weights ([q][ntile][k-step][lane] x 8 halves: every
// wave-level load is one contiguous KiB), branch-free main loop, residual-initialised accumulators, LDS-transposed dwordx4 stores,
// fused GroupNorm partials.  What differs:
//   * ONE fp16 image per patch buffer (no lo plane): 14.1 KiB per buffer, so EVERY tiling double-buffers its patch - two buffers
//     (28.3 KiB) are about the epilogue's transpose scratch (26 KiB), which every block needs anyway; the single-buffered
//     narrow tilings of the bf16x3 kernel have no reason to exist here.
//   * ONE MFMA per (k-step, accumulator tile).  A 32x32x16 MFMA occupies the SIMD for 32 cycles and two ds_read_b128 per MFMA
//     gap are nearly free, so the wave tiles are chosen with >= 2 MFMAs per A-fragment read wherever Cout allows: 128 px x 64 ch
//     (Cout > 128), 64 x 64 (65..128), 32 x 64 (33..64); only Cout <= 32 is left with 32 x 32.
//   * the A fragments of all tilings are fetched one k-step ahead into a second register set (the 128 x 64 tile has room for it
//     now: 128 accumulator + 32 fragment + 16 weight registers), so there is one main loop, not two.
#include "halo_mma.h"
#include <stdlib.h>

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

namespace {

__device__ __forceinline__ f16x8 as_f16x8(const uint4 &v) { return __builtin_bit_cast(f16x8, v); }

template <int BN, int WM, int WN, int PRO, bool UP2>
__global__ __launch_bounds__(WM * WN * 64, BN <= 64 ? 4 : 2) void conv3x3_halo_f16_kernel(const ConvParams p, const uint4 *__restrict__ wf16,
                                                                                         double *__restrict__ stats_part)
{
    using Frame = HaloFrame<BN, WM, WN, UP2>;
    constexpr int TW = Frame::TW, NT = Frame::NT, PW = Frame::PW, PP = Frame::PP, PUNITS = Frame::PUNITS, PROWS = Frame::PROWS;
    constexpr int TM = Frame::TM, TN = Frame::TN;
    static_assert(WM * WN == 4, "tile config");
    static_assert(PRO != FEMASR_PRO_LN, "no LayerNorm prologue on 3x3 convs");
    static_assert(PUNITS <= 8, "patch slices are stored over the last PUNITS taps, after the loads of tap 0");

    extern __shared__ __attribute__((aligned(16))) unsigned short smem_u16[];
    constexpr int IMG = (PP + 1) * PPITCH;       // halves per buffer; pixel PP is a write-only dummy slot
    unsigned short *Ps = smem_u16;               // [2][PP + 1][PPITCH]

    Frame f(p);        // block decode and patch unit addressing
    const int t = f.t, lane = f.lane, wave = f.wave, wm = f.wm, wn = f.wn, n = f.n, oy0 = f.oy0, ox0 = f.ox0, n0 = f.n0, kq = f.kq;
    float *gco = reinterpret_cast<float *>(smem_u16 + 2 * IMG);      // [2][Cin] floats behind the patch buffers
    if (PRO == FEMASR_PRO_GN_SILU) f.stage_gn(p, gco);
    float4 rp[PUNITS];
    auto load_patch = [&](int cc) {
#pragma unroll
        for (int i = 0; i < PUNITS; ++i) rp[i] = ld4(p.in + (size_t)f.poff[i] + (size_t)cc * BK);
    };
    auto store_patch_unit = [&](int buf, int i, int cc) {
        int pix = (t >> 3) + PROWS * i;
        if (PP % PROWS != 0 && i == PUNITS - 1) pix = pix < PP ? pix : PP;     // no branch: keeps the wait counters exact
        float4 v = rp[i];
        if (PRO == FEMASR_PRO_GN_SILU) {
            const float4 ga = *reinterpret_cast<const float4 *>(gco + cc * BK + 4 * kq);
            const float4 gb = *reinterpret_cast<const float4 *>(gco + p.Cin + cc * BK + 4 * kq);
            v.x = fast_silu(__builtin_fmaf(v.x, ga.x, gb.x));
            v.y = fast_silu(__builtin_fmaf(v.y, ga.y, gb.y));
            v.z = fast_silu(__builtin_fmaf(v.z, ga.z, gb.z));
            v.w = fast_silu(__builtin_fmaf(v.w, ga.w, gb.w));
        }
        if (!(f.pmask & (1u << i))) v = make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<uint2 *>(Ps + buf * IMG + pix * PPITCH + 4 * kq) = make_uint2(pack_f16(v.x, v.y), pack_f16(v.z, v.w));
    };

    // Output addressing = uniform part (SGPRs) + one per-lane offset: element r of row tile i sits at pixel row
    // 2*(wm*TM+i) + (r>>3), pixel column (r&3) + 8*((r>>2)&1) + 4*(lane>>5) of the 8x16 tile (the C/D layout of the 32x32 MFMA).
    const size_t obase = (((size_t)n * p.Ho + oy0) * p.Wo + ox0) * p.Cout + n0;             // uniform
    const unsigned loff4 = 4u * ((unsigned)(4 * (lane >> 5)) * (unsigned)p.Cout + (unsigned)(lane & 31));      // bytes
    auto uoff = [&](int i, int j, int r) -> size_t {            // uniform
        return obase + (size_t)((2 * (wm * TM + i) + (r >> 3)) * p.Wo + (r & 3) + 8 * ((r >> 2) & 1)) * p.Cout + (wn * TN + j) * 32;
    };
    auto ok_u = [&](int i, int j, int r) -> bool {
        return (oy0 + 2 * (wm * TM + i) + (r >> 3)) < p.Ho && (ox0 + (r & 3) + 8 * ((r >> 2) & 1)) < p.Wo && (n0 + (wn * TN + j) * 32) < p.Cout;
    };
    auto ok_l = [&](int i, int j, int r) -> bool {
        return (oy0 + 2 * (wm * TM + i) + (r >> 3)) < p.Ho && (ox0 + (r & 3) + 8 * ((r >> 2) & 1) + 4 * (lane >> 5)) < p.Wo &&
               (n0 + (wn * TN + j) * 32 + (lane & 31)) < p.Cout;
    };
    auto ld_res = [&](const float *res, int i, int j, int r) -> float {     // clamped: out-of-range elements read the tile origin
        return ldg_u32(res + (ok_u(i, j, r) ? uoff(i, j, r) : obase), ok_l(i, j, r) ? loff4 : 0u);
    };
    // accumulators start from the first residual, loaded as ONE branch-free batch (out-of-range elements read the tile origin and
    // are never stored); the second residual and the bias are added right before the main loop
    f32x16 acc[TM][TN];
    const float *ra = p.res1 ? p.res1 : p.res2, *rb = (p.res1 && p.res2) ? p.res2 : nullptr;
    if (ra) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = ld_res(ra, i, j, r);
    } else {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    }

    // fp16 weights, fragment-major: [q][ntile][k-step(2)][lane] x 8 halves = 128 uint4 per (q, ntile)
    const uint4 *wl[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) wl[j] = wf16 + ((size_t)wtile(n0, wn * TN + j, p.NT32) * 128 + lane);
    const size_t wstride = (size_t)p.NT32 << 7;     // uint4 per K chunk

    const int ncc = p.Cin / BK;
    load_patch(0);
    uint4 bc[TN][2];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int s = 0; s < 2; ++s) bc[j][s] = wl[j][s * 64];
    if (PRO == FEMASR_PRO_GN_SILU) __syncthreads();     // gco visible
#pragma unroll
    for (int i = 0; i < PUNITS; ++i) store_patch_unit(0, i, 0);
    __syncthreads();

    int py[TM], px;
    {
        const int m = wm * TM * 32 + (lane & 31);
        px = m & 15;
#pragma unroll
        for (int i = 0; i < TM; ++i) py[i] = (m >> 4) + 2 * i;
    }
    const int koff = 8 * (lane >> 5);                // this lane's k sub-block inside a 16-deep k-step

    const int abase = (py[0] * PW + px) * PPITCH;      // LDS index of the fragment pixel of row tile 0 (Frame::patch_idx)

    const int nq = ncc * 9;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int col = n0 + (wn * TN + j) * 32 + (lane & 31);
            const float bv = col < p.Cout ? p.bias[col] : 0.f;
            if (rb) {           // second residual (rare: last ResBlock of an up block): one batch per 32x32 tile
                float tmp[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) tmp[r] = ld_res(rb, i, j, r);
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] += tmp[r];
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] += bv;
        }

    // Main loop.  Everything inside is UNCONDITIONAL straight-line code (9 taps unrolled; the last channel block re-stages
    // itself into the idle LDS buffer and re-reads the last weight chunk) so that the compiler knows exactly how many loads are
    // in flight and emits exact s_waitcnt values.
    for (int cc = 0; cc < ncc; ++cc) {
        const unsigned short *Pb = Ps + (cc & 1) * IMG + koff;
        const int ccn = cc + 1 < ncc ? cc + 1 : cc;
        const int nbuf = (cc + 1) & 1;
        uint4 af[2][TM];
        int aidx[TM];
        Frame::patch_idx(0, py, px, abase, aidx);
#pragma unroll
        for (int i = 0; i < TM; ++i) af[0][i] = *reinterpret_cast<const uint4 *>(Pb + aidx[i]);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int q1 = cc * 9 + tap + 1;
            const size_t qn = (size_t)(q1 < nq ? q1 : nq - 1);
            if (tap == 0) load_patch(ccn);
            int nidx[TM];
            Frame::patch_idx(tap < 8 ? tap + 1 : 8, py, px, abase, nidx);
            // A fragments are fetched one k-step ahead (s=1 while s=0 multiplies, the next tap's s=0 while s=1 multiplies),
            // pinned with sched_barrier so the LDS latency hides behind MFMAs: TM ds_read_b128 per TM*TN MFMAs
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (s == 0) {
#pragma unroll
                    for (int i = 0; i < TM; ++i) af[1][i] = *reinterpret_cast<const uint4 *>(Pb + aidx[i] + 16);
                } else if (tap < 8) {
#pragma unroll
                    for (int i = 0; i < TM; ++i) af[0][i] = *reinterpret_cast<const uint4 *>(Pb + nidx[i]);
                }
                __builtin_amdgcn_sched_barrier(0);
                // consecutive MFMAs hit DIFFERENT accumulator tiles wherever the wave tile has more than one
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(as_f16x8(af[s][i]), as_f16x8(bc[j][s]), acc[i][j], 0, 0, 0);
                // this k-step's weight registers are free now: refill them with the NEXT tap's fragments (one tap of MFMAs ahead
                // of their use), no register copies
#pragma unroll
                for (int j = 0; j < TN; ++j) bc[j][s] = (wl[j] + qn * wstride)[s * 64];
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i) aidx[i] = nidx[i];
            // next channel block's patch: loaded at tap 0, one unit normalised / rounded / stored per tap over the LAST PUNITS taps
            if (tap >= 9 - PUNITS) store_patch_unit(nbuf, tap - (9 - PUNITS), ccn);
        }
        __syncthreads();
    }

    // ---- epilogue (the bf16x3 kernel's).  Each 32x32 tile is transposed through a per-wave LDS scratch (pitch TPITCH floats) and
    // written with dwordx4 stores: lane l holds channels 4(l&7)..+3 of pixel rows (l>>3) + 8k, k = 0..3.  Needs Cout % 4 == 0;
    // anything else keeps the scalar stores.
    float colsum[TM][TN], colsq[TM][TN];
    const bool full = (oy0 + 8 <= p.Ho) && (ox0 + TW <= p.Wo) && (n0 + BN <= p.Cout);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            float ps = 0.f, pss = 0.f;      // this lane's share of the GroupNorm moments of the OUTPUT (its column)
            if (full) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    ps += acc[i][j][r];
                    pss = __builtin_fmaf(acc[i][j][r], acc[i][j][r], pss);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (ok_l(i, j, r)) {
                        ps += acc[i][j][r];
                        pss = __builtin_fmaf(acc[i][j][r], acc[i][j][r], pss);
                    }
            }
            colsum[i][j] = ps;
            colsq[i][j] = pss;
        }
    if ((p.Cout & 3) == 0) {
        float *T = reinterpret_cast<float *>(smem_u16) + HALO_EPI_OFF + wave * TSCRATCH;      // clear of the GN `red` area
        const int trow = lane >> 3, tq = lane & 7;
        const unsigned lvec4 = 4u * ((unsigned)trow * (unsigned)p.Cout + 4u * (unsigned)tq);      // bytes
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
#pragma unroll
                for (int r = 0; r < 16; ++r) T[((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * TPITCH + (lane & 31)] = acc[i][j][r];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float4 v = *reinterpret_cast<const float4 *>(T + (trow + 8 * k) * TPITCH + 4 * tq);
                    const int prow = 2 * (wm * TM + i) + (k >> 1), pcol0 = 8 * (k & 1);               // uniform
                    const bool okv = full || ((oy0 + prow) < p.Ho && (ox0 + pcol0 + trow) < p.Wo && (n0 + (wn * TN + j) * 32 + 4 * tq) < p.Cout);
                    if (okv) {
                        float *ub = p.out + obase + (size_t)(prow * p.Wo + pcol0) * p.Cout + (wn * TN + j) * 32;
                        const unsigned long long a = uniform_u64(reinterpret_cast<unsigned long long>(ub));
                        *reinterpret_cast<__attribute__((address_space(1))) f32x4_t *>(a + lvec4) = f32x4_t{v.x, v.y, v.z, v.w};
                    }
                }
            }
    } else {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (ok_l(i, j, r)) stg_u32(p.out + uoff(i, j, r), loff4, acc[i][j][r]);
    }

    f.gn_partials(p, colsum, colsq, stats_part, smem_u16);
}

// fp32 -> fp16 (RNE) fragment-major: out half index = ((((q*NT32 + ntile)*2 + s)*64 + lane)*8 + e)
//   k = q*32 + 16 s + 8 (lane>>5) + e  in the blocked K order (k = ((ci/32)*kh*kw + y*kw + x)*32 + ci%32), n = ntile*32 + (lane&31)
// PACKED = false: `in` is the OIHW tensor; true: `in` is the fragment-major fp32 image of femasr_repack_oihw (the same values in
// the same K order), which is how a handle builds its fp16 images when the mode is first selected, long after the OIHW tensors are gone.
template <bool PACKED>
__global__ void repack_f16_kernel(const float *__restrict__ in, int O, int I, int kh, int kw, _Float16 *__restrict__ out, size_t total)
{
    const int K = I * kh * kw, NT32 = (O + 31) / 32;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int e = (int)(i & 7), lane = (int)((i >> 3) & 63), s = (int)((i >> 9) & 1);
        const size_t rest = i >> 10;
        const int ntile = (int)(rest % NT32), q = (int)(rest / NT32);
        const int k = q * 32 + 16 * s + 8 * (lane >> 5) + e, o = ntile * 32 + (lane & 31);
        float v = 0.f;
        if (k < K && o < O) {
            if (PACKED) {
                v = in[((((size_t)q * NT32 + ntile) * 64 + (k & 1) * 32 + (o & 31)) << 4) + ((k & 31) >> 1)];
            } else {
                const int cl = k % 32;
                int r = k / 32;
                const int x = r % kw;
                r /= kw;
                const int y = r % kh;
                const int ci = (r / kh) * 32 + cl;
                v = in[(((size_t)o * I + ci) * kh + y) * kw + x];
            }
        }
        out[i] = (_Float16)v;       // round to nearest even; |w| > 65504 would become Inf (no trained conv weight is near it)
    }
}

template <bool UP2>
constexpr size_t f16_lds_bytes() { return (size_t)2 * ((UP2 ? 60 : 180) + 1) * PPITCH * sizeof(unsigned short); }   // + 2*Cin floats (GN)

#define FEMASR_HF16(BN, WM, WN, PRO, UP2)                                                        \
    { "conv3x3_halo_f16<8x16x" #BN "," #PRO ",up2=" #UP2 ",waves=" #WM "x" #WN ">", BN, WM * WN * 64,   \
      conv3x3_halo_f16_kernel<BN, WM, WN, PRO, UP2>, f16_lds_bytes<UP2>(), 0ull }

HaloVariant g_vf16[] = {
    FEMASR_HF16(128, 2, 2, FEMASR_PRO_NONE, false),     // 0   Cout 65..128: 64 px x 64 ch per wave
    FEMASR_HF16(128, 2, 2, FEMASR_PRO_GN_SILU, false),  // 1
    FEMASR_HF16(128, 2, 2, FEMASR_PRO_NONE, true),      // 2
    FEMASR_HF16(64, 4, 1, FEMASR_PRO_NONE, false),      // 3   Cout 33..64: 32 px x 64 ch per wave
    FEMASR_HF16(64, 4, 1, FEMASR_PRO_GN_SILU, false),   // 4
    FEMASR_HF16(64, 4, 1, FEMASR_PRO_NONE, true),       // 5
    FEMASR_HF16(32, 4, 1, FEMASR_PRO_NONE, false),      // 6   Cout <= 32: 32 px x 32 ch per wave
    FEMASR_HF16(32, 4, 1, FEMASR_PRO_GN_SILU, false),   // 7
    FEMASR_HF16(32, 4, 1, FEMASR_PRO_NONE, true),       // 8
    FEMASR_HF16(256, 1, 4, FEMASR_PRO_NONE, false),     // 9   Cout > 128: 128 px x 64 ch per wave, one column block for Cout = 256
    FEMASR_HF16(256, 1, 4, FEMASR_PRO_GN_SILU, false),  // 10
    FEMASR_HF16(256, 1, 4, FEMASR_PRO_NONE, true),      // 11
};
constexpr int kNumF16 = sizeof(g_vf16) / sizeof(g_vf16[0]);

}  // namespace

int femasr_conv_f16_variant_count() { return kNumF16; }
const char *femasr_conv_f16_variant_name(int v) { return (v >= 0 && v < kNumF16) ? g_vf16[v].name : "?"; }

// the shape and size rule of the bf16x3 form: the two forms take the same layers
bool femasr_conv_f16_shape_ok(const femasr_conv_args *a) { return femasr_conv_bf16x3_shape_ok(a); }

int femasr_conv_f16_pick_variant(const femasr_conv_args *a)
{
    const int cls = a->Cout > 128 ? 3 : (a->Cout > 64 ? 0 : (a->Cout > 32 ? 1 : 2));
    return cls * 3 + (a->up2 ? 2 : a->prologue);
}

int femasr_conv_f16_launch(hipStream_t s, const femasr_conv_args *a, int *variant_out, double *flops_out)
{
    return halo_variant_launch(s, a, "conv f16", g_vf16, a ? a->w_f16 : nullptr, femasr_conv_f16_shape_ok, femasr_conv_f16_pick_variant, variant_out, flops_out);
}

// the fp16 image of a layer from its fragment-major fp32 image (femasr_repack_oihw; 3x3, I % 32 == 0): model.hip, first selection of mode 4
int femasr_repack_packed_f16(hipStream_t stream, const float *packed, int O, int I, void *out)
{
    FEMASR_REQUIRE(packed && out && O > 0 && I > 0 && (I % 32) == 0, "repack f16: needs I %% 32 == 0");
    const size_t total = femasr_packed_weight_f16_bytes(O, I, 3, 3) / sizeof(unsigned short);
    hipLaunchKernelGGL(repack_f16_kernel<true>, dim3(grid_for(total)), dim3(256), 0, stream, packed, O, I, 3, 3, (_Float16 *)out, total);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

extern "C" {

size_t femasr_packed_weight_f16_bytes(int O, int I, int kh, int kw)
{
    if (O <= 0 || I <= 0 || kh <= 0 || kw <= 0 || (I % 32) != 0) return 0;
    const size_t K = (size_t)I * kh * kw;
    return (K / 32) * (size_t)((O + 31) / 32) * 1024 * sizeof(unsigned short);
}

int femasr_repack_oihw_f16(void *stream, const float *in, int O, int I, int kh, int kw, void *out)
{
    FEMASR_REQUIRE(in && out && O > 0 && I > 0 && kh > 0 && kw > 0 && (I % 32) == 0, "repack f16: needs I %% 32 == 0");
    const size_t total = femasr_packed_weight_f16_bytes(O, I, kh, kw) / sizeof(unsigned short);
    hipLaunchKernelGGL(repack_f16_kernel<false>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, in, O, I, kh, kw,
                       (_Float16 *)out, total);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

}  // extern "C"

// halo_mma.h — the kernel frame of the two matrix-core 3x3 halo forms (kernels_conv_bf16.hip: bf16x3, kernels_conv_f16.hip: fp16).
//
// Both kernels compute 8x16 output pixels x BN channels per block with v_mfma_f32_32x32x16_*: one halo patch per 32-channel block is
// staged in LDS (GroupNorm-apply + SiLU in fp32, nearest-x2 folded into the patch indexing, zero outside the image) and swept by nine
// taps, and the block can emit GroupNorm partial moments of its output.  HaloFrame holds what does not depend on the operand format
// and moves without changing the kernels' registers or main-loop schedules: the tile constants, the block decode, the patch unit
// addressing, the GroupNorm coefficient staging, the A-fragment index and the GroupNorm partials.  The output addressing, the
// accumulator initialisation and the store epilogue stay written out in both kernels: as members they compiled to other register
// counts (profiles/halo_frame_isa_diff.txt).
#pragma once
#include "conv_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int PPITCH = 40;     // 16-bit elements per patch pixel (32 channels + 8 pad): 80-byte pitch, conflict-free ds_read_b128 per 16 lanes

// SiLU with the hardware exp2 / rcp approximations (1 ulp each): these forms are tolerance-based, so the 28-instruction
// bit-reproducible det_silu of the fp32 kernels is not needed here.
__device__ __forceinline__ float fast_silu(float t)
{
    return t * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(t * -1.44269504088896341f));
}

template <int BN, int WM, int WN, bool UP2>
struct HaloFrame {
    static constexpr int BM = 128, TW = 16, NT = WM * WN * 64;
    static constexpr int PH = UP2 ? 6 : 10, PW = UP2 ? 10 : 18, PP = PH * PW;       // patch; pixel PP of an LDS image is a write-only dummy slot
    static constexpr int PUNITS = (PP * 8 + NT - 1) / NT, PROWS = NT / 8;
    static constexpr int TM = BM / (WM * 32), TN = BN / (WN * 32);
    static_assert(TM >= 1 && TN >= 1, "tile config");
    // the GroupNorm `red` area ([WM][BN][2] doubles at the LDS base) ends below the transpose scratch
    static_assert(WM * BN * 2 * sizeof(double) <= HALO_EPI_OFF * sizeof(float), "red area overlaps the epilogue scratch");

    int t, lane, wave, wm, wn, tx, ty, n, oy0, ox0, n0, sy0, sx0;
    int kq;                         // patch unit i of this thread: pixel (t >> 3) + PROWS * i, channels 4 * kq .. + 3 of the channel block
    unsigned poff[PUNITS], pmask;   // its element offset in p.in (channel block 0) and whether it lies inside the image

    // block decode; patch units: pixels outside the image (and the units past the patch) read element 0 and are zeroed before the store
    __device__ __forceinline__ explicit HaloFrame(const ConvParams &p)
    {
        t = threadIdx.x, lane = t & 63;
        wave = __builtin_amdgcn_readfirstlane(t >> 6);
        wm = wave / WN, wn = wave % WN;
        const int L = xcd_remap(blockIdx.x, p.MB * p.NB);
        const int nb = L % p.NB;
        int tile = L / p.NB;
        tx = tile % p.tilesX;
        tile /= p.tilesX;
        ty = tile % p.tilesY;
        n = tile / p.tilesY;
        oy0 = ty * 8, ox0 = tx * TW, n0 = nb * BN;
        sy0 = UP2 ? (oy0 >> 1) - 1 : oy0 - 1, sx0 = UP2 ? (ox0 >> 1) - 1 : ox0 - 1;

        kq = t & 7;
        pmask = 0;
#pragma unroll
        for (int i = 0; i < PUNITS; ++i) {
            const int pix = (t >> 3) + PROWS * i;
            const int ppy = pix / PW, ppx = pix - ppy * PW;
            const int sy = sy0 + ppy, sx = sx0 + ppx;
            const bool ok = (pix < PP) & (sy >= 0) & (sy < p.H) & (sx >= 0) & (sx < p.W);
            poff[i] = ok ? (unsigned)((((size_t)n * p.H + sy) * p.W + sx) * p.Cin + 4 * kq) : 0u;
            pmask |= (ok ? 1u : 0u) << i;
        }
    }

    // GroupNorm coefficients of this sample: staged once in LDS behind the patch buffers ([2][Cin] floats), read back per unit at store
    // time (no per-channel-block global loads in the main loop, no registers held across taps).  Visible after the next barrier.
    __device__ __forceinline__ void stage_gn(const ConvParams &p, float *dst) const
    {
        for (int c = t; c < p.Cin; c += NT) {
            dst[c] = p.pro_a[(size_t)n * p.Cin + c];
            dst[p.Cin + c] = p.pro_b[(size_t)n * p.Cin + c];
        }
    }

    // LDS index of this lane's A-fragment pixel (px, py[i]) for (tap, row tile i).  Without the fused x2 upsample it is ONE per-lane
    // base (abase, the pixel of row tile 0) plus a compile-time constant (folded into the ds_read offset field); with it the halving
    // depends on the lane.
    static __device__ __forceinline__ void patch_idx(int tap, const int (&py)[TM], int px, int abase, int (&idx)[TM])
    {
        const int ky = tap / 3, kx = tap - ky * 3;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            if (UP2) {
                const int prow = ((py[i] + ky - 1) >> 1) + 1, pcol = ((px + kx - 1) >> 1) + 1;
                idx[i] = (prow * PW + pcol) * PPITCH;
            } else {
                idx[i] = abase + ((2 * i + ky) * PW + kx) * PPITCH;
            }
        }
    }

    // Optional fused GroupNorm moments of the output (consumed by the NEXT conv's GN prologue): per (tile, group) partial sums,
    // reduced lane -> group (xor shuffles over the cg lanes of a group, then the two row halves) -> waves (LDS) and written as
    // doubles to stats_part[((n*tiles + tile)*32 + g)*2]; a fixed order, so runs are reproducible.
    // lds: the block's LDS base (the patch buffers are dead after the main loop's last barrier).
    __device__ __forceinline__ void gn_partials(const ConvParams &p, const float (&colsum)[TM][TN], const float (&colsq)[TM][TN], double *stats_part, void *lds) const
    {
        if (!stats_part) return;
        const int cg = p.Cout >> 5;                       // channels per group (32 groups): 8 / 4 / 2 / 1 (halo_variant_launch)
        double *red = reinterpret_cast<double *>(lds);    // [WM][BN][2]
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            double s_ = 0.0, q_ = 0.0;      // fp64 from here on: across row tiles, lanes and waves (a per-lane partial is 16 fp32 terms)
#pragma unroll
            for (int i = 0; i < TM; ++i) { s_ += (double)colsum[i][j]; q_ += (double)colsq[i][j]; }
            for (int sft = 1; sft < cg; sft <<= 1) {
                s_ += __shfl_xor(s_, sft, 64);
                q_ += __shfl_xor(q_, sft, 64);
            }
            s_ += __shfl_xor(s_, 32, 64);
            q_ += __shfl_xor(q_, 32, 64);
            if (lane < 32 && (lane % cg) == 0) {
                const int gl = ((wn * TN + j) * 32 + lane) / cg;        // group index inside this block's BN columns
                red[(wm * BN + gl) * 2] = s_;
                red[(wm * BN + gl) * 2 + 1] = q_;
            }
        }
        __syncthreads();
        const int ngl = BN / cg;                                         // groups covered by this block
        if (t < ngl && n0 + t * cg < p.Cout) {
            double S = 0.0, Q = 0.0;
#pragma unroll
            for (int w2 = 0; w2 < WM; ++w2) {
                S += red[(w2 * BN + t) * 2];
                Q += red[(w2 * BN + t) * 2 + 1];
            }
            const int g = n0 / cg + t;
            const size_t tile_id = (size_t)n * p.tilesX * p.tilesY + (size_t)ty * p.tilesX + tx;
            stats_part[(tile_id * 32 + g) * 2] = S;
            stats_part[(tile_id * 32 + g) * 2 + 1] = Q;
        }
    }
};

}  // namespace

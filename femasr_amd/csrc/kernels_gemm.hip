// kernels_gemm.hip — fp32 GEMM for every 1x1 conv / nn.Linear of the hot path and for the VQ distance matrix:
//     out[M][N] = epi( A[M][K] . W[K][N] ),   A = NHWC activations / tokens (row-major), W = packed weights
// (network_swinir.py:19-21,105-112 qkv / proj / fc1 / fc2;  femasr_arch.py:298 before_quant;  femasr_arch.py:35-38 z.e^T)
//
// MI355X design (this replaces the K1 variants of conv_igemm_kernel, which staged A through registers):
//   * BOTH operands reach LDS by LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave-instruction): no staging VGPRs, no
//     ds_write, no VALU in the main loop at all — fp32 MFMA shares its lanes with the VALU (SQ_VALU_MFMA_COEXEC = 0),
//     so every VALU instruction removed from the loop is matrix time won back.
//   * A tile [128 rows][32 k] per K chunk, one 128-byte line per row, XOR-swizzled by the SOURCE address (the DMA
//     destination is lane-linear): 16-byte granule g of row r sits at  r*8 + (g ^ ((r>>1)&7))  -> the MFMA A fragment
//     A[i = lane&31][k-granule 2j + (lane>>5)] is ONE conflict-free ds_read_b128 per lane and row tile.
//   * W is stored in the order the B fragments are consumed,  [chunk][n/32][j][lane][t]  with
//     k = 32*chunk + 8j + 4*(lane>>5) + t,  n = 32*(n/32) + (lane&31):  the DMA copy is linear and the fragment read is
//     one conflict-free ds_read_b128 per lane and column tile.
//   * One 16-byte fragment feeds 4 MFMA steps: step t multiplies k = 8j + t (lanes 0-31) and k = 8j + 4 + t (lanes 32-63),
//     i.e. each output is ONE fp32 fmaf chain in the order 0,4,1,5,2,6,3,7 inside every group of 8 channels — the order
//     oracle/femasr_oracle.c (ORC_KPERM) specifies for these layers, so results stay bit-identical to the CPU oracle.
//   * 256 threads = 4 waves of 64 x 64 outputs (2 x 2 accumulator tiles of v_mfma_f32_32x32x2_f32).  Two pipeline
//     configurations, chosen per launch by which wastes less of its last round of (equal-cost) tiles:
//       <KB=4, ST=2>  32-deep chunks, two 32 KB stages, 2 blocks per CU, two barriers per chunk (landed / free again);
//       <KB=2, ST=3>  16-deep chunks, three 16 KB stages, 3 blocks per CU, one barrier per chunk.
//     Waits are counted (vmcnt(8) / vmcnt(4): the next chunk's pieces stay in flight across the barrier); fragment
//     double buffering is pinned with sched_barrier.
//   * Measured (B = 16, M = 82944): all pipeline shapes tried - these two, 4 blocks per CU, and a persistent block with
//     cross-tile prefetch - land within 2 % of each other (MFMA busy 0.66-0.74 in the network at 2.4 GHz); ablations
//     price the epilogue stores at ~10 %, the A and W DMA at 5-8 % each, the barriers at 0.
//   * Epilogue: bias, exact-erf GELU, up to two residuals (order fixed by the bit-exact contract), each 32 x 32 tile
//     transposed through a per-wave LDS scratch and stored as float4 rows (gemm_store_epilogue, gemm_common.h, which also holds the
//     block decode and the host side the three row GEMMs share); or the VQ first-min epilogue.
#include "gemm_common.h"
#include <type_traits>
#include <atomic>

namespace {

struct GemmDmaParams : GemmParams {
    const float *vq_zz, *vq_ee;  // the VQ epilogue
    float *vq_part;
    int vq_nblk;
};

// Configuration <WT, KB, ST>: WT = accumulator tiles (32 x 32) per wave and dimension - the block (4 waves, 2 x 2) computes
//   64 WT x 64 WT outputs (WT = 2: 128 x 128, WT = 1: 64 x 64 for launches that would not fill the chip otherwise);
//   KB = 8-channel groups per K chunk (4: 32-deep chunks, 2: 16-deep), ST = LDS stages.
//   ST = 2: two barriers per chunk (data landed / stage free again);  ST = 3: one barrier per chunk.
template <int WT, int KB, int ST>
struct GCfg {
    static constexpr int kBM = 64 * WT;                     // block tile (rows = columns)
    static constexpr int kTile = 512 * KB * WT;             // floats of one operand tile per stage (64 WT rows x 8 KB floats)
    static constexpr int kStage = 2 * kTile;                // A tile + W tile
    static constexpr int kLdsBytes = (ST * kStage * 4) > (4 * TSCRATCH * 4) ? (ST * kStage * 4) : (4 * TSCRATCH * 4);
    static constexpr int kBlocksPerCU = (160 * 1024) / kLdsBytes > 4 ? 4 : (160 * 1024) / kLdsBytes;
};

typedef __attribute__((address_space(3))) void *lds_vptr;
typedef __attribute__((address_space(1))) const void *glb_cvptr;

__device__ __forceinline__ void dma16(const float *gsrc, float *lds_dst_uniform)
{
    // 64 lanes x 16 bytes -> 1 KiB at lds_dst_uniform (wave-uniform) + lane*16
    __builtin_amdgcn_global_load_lds((glb_cvptr)gsrc, (lds_vptr)lds_dst_uniform, 16, 0, 0);
}

template <int WT, int KB, int ST, int ACT, int NRES, bool VQ>
__global__ __launch_bounds__(256, (GCfg<WT, KB, ST>::kBlocksPerCU)) void gemm_dma_kernel(const GemmDmaParams p)
{
    using C = GCfg<WT, KB, ST>;
    constexpr int G_BM = C::kBM, G_BN = C::kBM;
    constexpr int GR = 2 * KB;                 // 16-byte granules per A row and chunk
    constexpr int RPP = 64 / GR;               // rows per 1 KiB DMA piece
    constexpr int SW = GR == 8 ? 1 : 2;        // swizzle: granule g of row r sits at r*GR + (g ^ ((r >> SW) & (GR-1)))
    constexpr int PP = WT * KB / 2;            // DMA pieces per wave, stage and operand (the tile has 2 WT KB pieces of 1 KiB)
    constexpr int PW = 2 * PP;                 // DMA pieces per wave and stage
    static_assert(KB == 2 || KB == 4, "chunk depth");
    static_assert(ST >= 2 && ST <= 4, "stages");
    static_assert(WT == 2 || (WT == 1 && KB == 4), "block tile");
    static_assert(!VQ || WT == 2, "the VQ epilogue reduces over 128-column blocks");
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const GemmFrame f(p.MB, p.NB, G_BM);
    const int t = f.t, lane = f.lane, wave = f.wave, wm = f.wm, wn = f.wn, nb = f.nb, m0 = f.m0, n0 = f.n0, h = f.h, c31 = f.c31;

    // ---- DMA sources.  A piece i of this wave = rows RPP*(PP*wave+i) .. of the tile: lane -> (row, granule).
    const float *srcA[PP];
#pragma unroll
    for (int i = 0; i < PP; ++i) {
        const int row = RPP * (PP * wave + i) + lane / GR;
        const int g = (lane & (GR - 1)) ^ ((row >> SW) & (GR - 1));
        int grow = m0 + row;
        grow = grow < p.M ? grow : p.M - 1;                 // tail rows: clamp (computed, never stored)
        srcA[i] = p.A + (size_t)grow * p.K + 4 * g;
    }
    // W pieces: the packed matrix is [chunk32][ntile][j = 0..3][lane][t] (a KB = 2 chunk takes j = 2*(c&1) + {0,1}); the stage
    // holds [column tile of the block][j < KB] pieces; this wave copies pieces PP*wave .. PP*wave + PP-1 of them, which lie in
    // ONE column tile (WT = 2: tile `wave`, all its j; WT = 1: tile wave/2, j = 2*(wave&1) + {0,1}).
    int ntile = (n0 >> 5) + (PP * wave) / KB;
    ntile = ntile < p.NT32 ? ntile : p.NT32 - 1;            // tiles past the packed matrix: clamp (never stored)
    const float *srcW = static_cast<const float *>(p.W) + ((size_t)ntile * 256 + lane) * 4 + ((PP * wave) % KB) * 256;
    const size_t wchunk = (size_t)p.NT32 * 1024;            // floats per 32-deep K chunk of the packed matrix

    auto issue = [&](int sb, int c) {
        float *dA = smem + sb * C::kStage + wave * (256 * PP);          // this wave's PP A pieces
        float *dW = smem + sb * C::kStage + C::kTile + wave * (256 * PP);
#pragma unroll
        for (int i = 0; i < PP; ++i) dma16(srcA[i] + c * (8 * KB), dA + i * 256);
        const float *w = KB == 4 ? srcW + (size_t)c * wchunk : srcW + (size_t)(c >> 1) * wchunk + (c & 1) * 512;
#pragma unroll
        for (int j = 0; j < PP; ++j) dma16(w + j * 256, dW + j * 256);
    };

    // ---- fragment addresses (floats inside a stage)
    const int xq = h ^ ((c31 >> SW) & (GR - 1));
    int aoff[KB];
#pragma unroll
    for (int j = 0; j < KB; ++j) aoff[j] = ((wm * 32 * WT + c31) * GR + ((2 * j) ^ xq)) * 4;
    const int boff = C::kTile + (wn * WT * KB) * 256 + lane * 4;
    constexpr int AROW32 = 32 * GR * 4;        // floats between the two row tiles of a wave

    f32x16 acc[WT][WT];
#pragma unroll
    for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int j = 0; j < WT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nch = p.K / (8 * KB);
#pragma unroll
    for (int i = 0; i < (ST == 2 ? 2 : ST - 1); ++i) issue(i, i < nch ? i : nch - 1);

    // Fragment double buffering is PINNED with sched_barrier(0): left alone, the scheduler funnels both fragment sets through
    // one register set (load -> wait -> 16 MFMAs -> load -> wait ...), exposing an LDS round trip per 8-channel group.
    auto compute = [&](const float *S) {
        f32x4_t af[2][WT], bf[2][WT];
#pragma unroll
        for (int i = 0; i < WT; ++i) af[0][i] = *reinterpret_cast<const f32x4_t *>(S + aoff[0] + i * AROW32);
#pragma unroll
        for (int j = 0; j < WT; ++j) bf[0][j] = *reinterpret_cast<const f32x4_t *>(S + boff + j * (256 * KB));
#pragma unroll
        for (int g = 0; g < KB; ++g) {
            const int cur = g & 1, nxt = cur ^ 1;
            if (g + 1 < KB) {
#pragma unroll
                for (int i = 0; i < WT; ++i) af[nxt][i] = *reinterpret_cast<const f32x4_t *>(S + aoff[g + 1 < KB ? g + 1 : 0] + i * AROW32);
#pragma unroll
                for (int j = 0; j < WT; ++j) bf[nxt][j] = *reinterpret_cast<const f32x4_t *>(S + boff + j * (256 * KB) + (g + 1) * 256);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < WT; ++i)
#pragma unroll
                    for (int j = 0; j < WT; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur][i][e], bf[cur][j][e], acc[i][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    if constexpr (ST == 2) {
        for (int c = 0; c < nch; ++c) {
            if constexpr (PW == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            __builtin_amdgcn_s_barrier();                         // this wave's pieces of chunk c have landed ... and every other wave's
            asm volatile("" ::: "memory");
            compute(smem + (c & 1) * C::kStage);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // this wave's fragment reads of stage c&1 have RETURNED ...
            __builtin_amdgcn_s_barrier();                         // ... and every other wave's: the stage may be overwritten
            asm volatile("" ::: "memory");
            const int cn = c + 2 < nch ? c + 2 : nch - 1;         // unconditional (keeps the vmcnt count constant); the
            issue(c & 1, cn);                                     // surplus copies at the end land in a dead stage
        }
    } else {
        // ST >= 3: chunk c + ST-1 is issued at the START of chunk c (into the stage chunk c-1 just left): ST-2 chunks stay in
        // flight under the MFMAs of chunk c, one barrier per chunk
        int sc = 0, sn = ST - 1;                                  // stage of chunk c / of chunk c + ST-1
        for (int c = 0; c < nch; ++c) {
            asm volatile("s_waitcnt vmcnt(%0)" :: "n"((ST - 2) * PW) : "memory");
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // (the previous chunk's fragment reads have returned)
            __builtin_amdgcn_s_barrier();                         // chunk c landed everywhere; stage of chunk c-1 is free everywhere
            asm volatile("" ::: "memory");
            const int cn = c + ST - 1 < nch ? c + ST - 1 : nch - 1;
            issue(sn, cn);
            compute(smem + sc * C::kStage);
            sc = sc == ST - 1 ? 0 : sc + 1;
            sn = sn == ST - 1 ? 0 : sn + 1;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // no DMA may still be writing LDS when the epilogue re-uses it
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");

    if constexpr (!VQ) {
        gemm_store_epilogue<WT, ACT, NRES, false>(p, f, smem, [&](int i, int j, int r) { return acc[i][j][r]; });
    } else if constexpr (WT == 2) {
        // d = (|z|^2 + |e|^2) - 2 z.e ; first-min over this block's 128 columns, per row (femasr_arch.py:35-38,63-66).
        float *red = smem;   // [2 (wn)][128 rows][2]  (2 KB)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rowl = (wm * 2 + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                const int row = m0 + rowl;
                const float zz = row < p.M ? p.vq_zz[row] : 0.f;
                float bd = INFINITY;
                int bi = 0x7fffffff;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int col = n0 + (wn * 2 + j) * 32 + c31;
                    if (col < p.N) {
                        const float d = (zz + p.vq_ee[col]) - 2.0f * acc[i][j][r];
                        if (d < bd || (d == bd && col < bi)) { bd = d; bi = col; }
                    }
                }
#pragma unroll
                for (int s = 16; s >= 1; s >>= 1) {
                    const float od = __shfl_xor(bd, s, 64);
                    const int oi = __shfl_xor(bi, s, 64);
                    if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
                }
                if (c31 == 0) {
                    red[(wn * G_BM + rowl) * 2] = bd;
                    red[(wn * G_BM + rowl) * 2 + 1] = __int_as_float(bi);
                }
            }
        __syncthreads();
        if (t < G_BM && m0 + t < p.M) {
            float bd = red[t * 2];
            int bi = __float_as_int(red[t * 2 + 1]);
            const float od = red[(G_BM + t) * 2];
            const int oi = __float_as_int(red[(G_BM + t) * 2 + 1]);
            if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
            float *dst = p.vq_part + ((size_t)(m0 + t) * p.vq_nblk + nb) * 2;
            dst[0] = bd;
            dst[1] = __int_as_float(bi);
        }
    }
}

#define G_VARIANT(WT, KB, ST, ACT, NRES, VQ) { "gemm_dma<tile=64*" #WT ",k=8*" #KB ",stages=" #ST ",act=" #ACT ",nres=" #NRES ",vq=" #VQ ">", \
                                                gemm_dma_kernel<WT, KB, ST, ACT, NRES, VQ>, GCfg<WT, KB, ST>::kLdsBytes, 0ull }
#define G_CFG(WT, KB, ST, VQ) G_VARIANT(WT, KB, ST, 0, 0, false), G_VARIANT(WT, KB, ST, 0, 1, false), G_VARIANT(WT, KB, ST, 0, 2, false), \
                              G_VARIANT(WT, KB, ST, 1, 0, false), G_VARIANT(WT, KB, ST, 1, 1, false), G_VARIANT(WT, KB, ST, 1, 2, false), \
                              G_VARIANT(WT, KB, ST, 0, 0, VQ)
// (the 64 x 64 configuration has no VQ form: slot unused.  Measured and dropped again: 64 x 64 with 3 / 4 stages and 128 x 128 with
// four 16-deep stages - G_CFG(1, 4, 3) / (1, 4, 4) / (2, 2, 4) - are within +-3 % of these at every batch size: prefetch depth is
// not what bounds the kernel)
GemmVariant<GemmDmaParams> g_gv[] = { G_CFG(2, 4, 2, true), G_CFG(2, 2, 3, true), G_CFG(1, 4, 2, false) };
constexpr int kPerCfg = 7;
constexpr int kTileOf[] = { 128, 128, 64 };
constexpr int kNumG = sizeof(g_gv) / sizeof(g_gv[0]);
std::atomic<int> g_cfg{-1};          // negative: automatic, 0 / 1 / 2: forced (femasr_gemm_force_config; test hook, process-global)

// [chunk][n/32][j][lane][t] <- W[n][k]  (torch (out,in) / OIHW with 1x1 taps), zero padded in n
__global__ void repack_k1_kernel(const float *__restrict__ in, int O, int I, float *__restrict__ out, size_t total)
{
    const int NT32 = (O + 31) / 32;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int tt = (int)(i & 3), lane = (int)((i >> 2) & 63), j = (int)((i >> 8) & 3);
        const size_t rest = i >> 10;
        const int ntile = (int)(rest % NT32), c = (int)(rest / NT32);
        const int k = 32 * c + 8 * j + 4 * (lane >> 5) + tt, n = 32 * ntile + (lane & 31);
        out[i] = n < O ? in[(size_t)n * I + k] : 0.f;
    }
}

}  // namespace

bool femasr_gemm_eligible(const femasr_conv_args *a)
{
    return a->ksz == 1 && a->stride == 1 && a->pad == 0 && !a->up2 && (a->Cin % 32) == 0 && a->prologue == FEMASR_PRO_NONE;
}

int femasr_gemm_variant_count() { return kNumG; }

extern "C" int femasr_gemm_force_config(int cfg)
{
    return g_cfg.exchange((cfg >= 0 && cfg < kNumG / kPerCfg) ? cfg : -1);
}
const char *femasr_gemm_variant_name(int v) { return (v >= 0 && v < kNumG) ? g_gv[v].name : "?"; }

int femasr_repack_k1(hipStream_t s, const float *in, int O, int I, float *out)
{
    FEMASR_REQUIRE(in && out && O > 0 && I > 0 && (I % 32) == 0, "repack_k1: bad args");
    const size_t total = (size_t)I * ((O + 31) / 32) * 32;
    hipLaunchKernelGGL(repack_k1_kernel, dim3(grid_for(total)), dim3(256), 0, s, in, O, I, out, total);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

// the variant a launch runs: epilogue (VQ argmin / activation + residual operands) and block configuration
int femasr_gemm_pick_variant(const femasr_conv_args *a, bool vq)
{
    const long long M = (long long)a->B * a->H * a->W;
    const int mb128 = (int)((M + 127) / 128), nb128 = (a->Cout + 127) / 128;
    int vi;
    if (vq) {
        vi = 6;
    } else {
        const int nres = (a->res1 ? 1 : 0) + (a->res2 ? 1 : 0);
        vi = (a->act == FEMASR_ACT_GELU ? 3 : 0) + nres;
    }
    // Configuration by tile count.  All tiles of a launch cost the same, so it takes ceil(tiles / resident slots) rounds:
    //   * fewer than kSmallTiles 128 x 128 tiles (small batches: B = 1 has 82 of them for proj / fc2 on 256 CUs,
    //     each a serial chain of K/2 MFMAs per wave): 64 x 64 tiles - 4x the blocks, a quarter of the chain each;
    //   * (measured and dropped: 64 x 64 tiles also where 128 x 128 tiles leave > 10 % of their last round empty - proj / fc2 at B = 16 win
    //     stand-alone, the step gets 0.4 ms SLOWER, 79.65 vs 79.27: the second sub-batch stream already fills those tails)
    //   * otherwise <4,2> (32-deep chunks, 2 blocks per CU) unless the 3-blocks-per-CU configuration <2,3> wastes less of its
    //     last round.
    int cfg = g_cfg.load();
    if (cfg < 0 || (vq && kTileOf[cfg] != 128)) {
        const double tiles = (double)mb128 * nb128;
        auto eff = [&](double slots) { const double r = tiles / slots; return r / (double)(long long)(r + 0.999999); };
        constexpr double kSmallTiles = 700.0;
        const double e2 = eff(512.0), e3 = eff(768.0);
        cfg = (!vq && tiles < kSmallTiles) ? 2 : (e3 > e2 + 0.02 ? 1 : 0);
    }
    return vi + cfg * kPerCfg;
}

int femasr_gemm_launch(hipStream_t s, const femasr_conv_args *a, const conv_vq_epilogue *vq, int *variant_out, double *flops_out)
{
    FEMASR_REQUIRE(a && a->in && a->w && femasr_gemm_eligible(a), "gemm: layer is not a 1x1 / linear layer with Cin %% 32 == 0");
    FEMASR_REQUIRE(vq || (a->bias && a->out), "gemm: bias/out must be set");
    GemmDmaParams p{};
    FEMASR_CHECK(gemm_params(a, "gemm", a->H, a->W, a->Cin, p));
    p.W = a->w;
    if (vq) {
        FEMASR_REQUIRE(vq->zz && vq->ee && vq->part && vq->nblk == (p.N + 127) / 128 && (a->Cout % 32) == 0, "vq epilogue: bad args");
        p.vq_zz = vq->zz; p.vq_ee = vq->ee; p.vq_part = vq->part; p.vq_nblk = vq->nblk;
    }
    const int vi = femasr_gemm_pick_variant(a, vq != nullptr);
    return gemm_variant_launch(s, g_gv, vi, kTileOf[vi / kPerCfg], p, variant_out, flops_out);
}

// kernels_gemm_f16.hip — the 1x1 stride-1 layers (Swin qkv / proj / fc1 / fc2, before_quant) on the fp16 matrix cores, ONE pass
// (linear_math 'fp16', C ABI mode 2):   out[M][N] = epi( A[M][K] . W[K][N] )
//
// Where it is used: the 1x1 layers the split GEMM (kernels_gemm_bf16.hip) takes, under its k1 shape rule, and only when the caller opts
// in (femasr_set_linear_math(2)).  These layers sit in FRONT of the codebook lookup: the mode may move a VQ index.
//
// Arithmetic (include/femasr_hip.h, femasr_conv_args.w_f16 with ksz = 1):
//   a16 = fp16_rne(clamp(a, +-65504))   the fp32 input row, converted while the A tile is staged (not the truncating pack conversion)
//   w16 = fp16_rne(w)                   packed once by femasr_repack_k1_f16; fp16 subnormals take part with their value
//   out = epi(bias + sum_k a16_k w16_k) products exact in fp32 (11 + 11 significand bits), accumulated in fp32 by
//                                       v_mfma_f32_32x32x16_f16, k ascending; bias in fp32; GELU by det_gelu2 - the device function of
//                                       every GEMM epilogue (gemm_common.h) -; one residual added in fp32; stored as fp32.
//
// The kernel is memory-side at the network's shapes (M = 82 944 rows, K and N in 256..1024: 8 MFMAs per wave against 16 KiB of fp32
// rows per 64-deep chunk), so it is built for bytes in flight, not for MFMA scheduling: no inline asm, no counted waits.
// Block = 256 threads = 4 waves of 64 x 64 outputs (2 x 2 tiles of 32 x 32), 128 x 128 block tile.  Per 64-deep K chunk:
//   * A: every thread loads eight float4 (rows (t >> 4) + 16 i, channels 4 (t & 15) .. + 3: 16 lanes cover 256 contiguous bytes of a
//     row) one chunk ahead, clamps, rounds and stores them as 8-byte LDS writes into the idle half of a double buffer
//     ([128 rows][72 halves]: the 144-byte pitch keeps the 16-lane ds_read_b128 groups conflict-free); one barrier per chunk;
//   * W: fp16 fragments, fragment-major ([k step][n / 32][lane] x 8 halves: every wave-level load is one contiguous KiB), read from
//     global / L2 straight into registers two k steps ahead - the whole matrix is at most 512 KiB and stays in L2.
// 36 KiB of LDS; the epilogue (gemm_store_epilogue of gemm_common.h: per-wave LDS transpose, float4 loads / stores) overlays the A buffers.
#include "gemm_common.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

namespace {

constexpr int GH_CK = 64;                             // K chunk
constexpr int GH_PITCH = 72;                          // halves per staged row (64 + 8 pad)
constexpr int GH_BUF = 128 * GH_PITCH;                // halves per buffer
constexpr int GH_LDS_BYTES = 2 * GH_BUF * 2;          // 36 864
static_assert(4 * TSCRATCH * 4 <= GH_LDS_BYTES, "epilogue scratch overlays the main-loop buffers");

template <int ACT, int NRES>
// (130 VGPRs: three blocks per CU; a bound of four waves per SIMD spills 7 - 9 dwords to scratch, which the build gate refuses)
__global__ __launch_bounds__(256, 2) void gemm_f16_kernel(const GemmParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    unsigned short *As = reinterpret_cast<unsigned short *>(smem_raw);      // [2][128][GH_PITCH]

    const GemmFrame f(p.MB, p.NB, 128);
    const int t = f.t, lane = f.lane, wm = f.wm, wn = f.wn, m0 = f.m0, n0 = f.n0, h = f.h, c31 = f.c31;
    const int nch = p.K / GH_CK, nsteps = p.K >> 4;

    // ---- A staging: rows (t >> 4) + 16 i, channels 4 (t & 15) .. + 3 of the chunk; tail rows are clamped (computed, never stored)
    const int kq = t & 15, sr0 = t >> 4;
    const float *srcA[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int grow = m0 + sr0 + 16 * i;
        grow = grow < p.M ? grow : p.M - 1;
        srcA[i] = p.A + (size_t)grow * p.K + 4 * kq;
    }
    float4 rp[8];
    auto load_A = [&](int c) {
#pragma unroll
        for (int i = 0; i < 8; ++i) rp[i] = ld4(srcA[i] + (size_t)c * GH_CK);
    };
    auto store_A = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            *reinterpret_cast<uint2 *>(As + buf * GH_BUF + (sr0 + 16 * i) * GH_PITCH + 4 * kq) =
                make_uint2(pack_f16(rp[i].x, rp[i].y), pack_f16(rp[i].z, rp[i].w));
    };

    // ---- W fragments of this wave's two column tiles: [k step][n / 32][lane]; tiles past the packed matrix are clamped (never stored)
    const uint4 *wl[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) wl[ct] = static_cast<const uint4 *>(p.W) + ((size_t)wtile(n0, wn * 2 + ct, p.NT32) * 64 + lane);
    const size_t wstep = (size_t)p.NT32 * 64;          // uint4 per k step

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    load_A(0);
    uint4 bc[2][2];                                     // [column tile][k step parity]
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int s = 0; s < 2; ++s) bc[ct][s] = wl[ct][(size_t)s * wstep];      // (K >= 64: steps 0 and 1 exist)
    store_A(0);
    __syncthreads();

    // this lane's A fragment of row tile rt at k step s of a chunk: As[row][16 s + 8 h .. + 7]
    int aoff[2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) aoff[rt] = (wm * 64 + rt * 32 + c31) * GH_PITCH + 8 * h;

    for (int cc = 0; cc < nch; ++cc) {
        const unsigned short *Ab = As + (cc & 1) * GH_BUF;
        load_A(cc + 1 < nch ? cc + 1 : cc);             // the last chunk re-stages itself into the idle buffer: no branch in the loop
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            uint4 af[2];
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) af[rt] = *reinterpret_cast<const uint4 *>(Ab + aoff[rt] + 16 * s);
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
                    acc[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, af[rt]), __builtin_bit_cast(f16x8, bc[ct][s & 1]),
                                                                         acc[rt][ct], 0, 0, 0);
            // this step's weight registers are free: refill them with the fragments of two steps on (clamped at the end of K)
            const int sn = cc * 4 + s + 2;
            const size_t so = (size_t)(sn < nsteps ? sn : nsteps - 1) * wstep;
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) bc[ct][s & 1] = wl[ct][so];
        }
        store_A((cc + 1) & 1);                          // (every wave left that buffer before the barrier that ended chunk cc - 1)
        __syncthreads();
    }

    // ---- epilogue (gemm_common.h); a null bias adds +0.  (The last barrier of the loop has passed: the A buffers are dead.)
    gemm_store_epilogue<2, ACT, NRES, true>(p, f, reinterpret_cast<float *>(smem_raw), [&](int i, int j, int r) { return acc[i][j][r]; });
}

// [k step][n / 32][lane] x 8 halves  <-  W[n][k] (torch (out, in)), zero padded in n, round to nearest even;
// lane (j = lane & 31, h = lane >> 5) holds k = 16 step + 8 h + 0..7 of column n = 32 (n / 32) + j.
// PACKED = true: `in` is the GEMM-layout fp32 image of femasr_repack_oihw (kh = kw = 1; the same values), which is how a handle builds
// its fp16 images when the mode is first selected, after the (out, in) tensors are gone.
template <bool PACKED>
__global__ void repack_k1_f16_kernel(const float *__restrict__ in, int O, int I, _Float16 *__restrict__ out, size_t total)
{
    const int NT32 = (O + 31) / 32;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const FragItem it = frag_item(i >> 3, NT32);      // (gemm_common.h)
        const int n = it.n, nt = n >> 5, k = it.k0 + (int)(i & 7);
        float v = 0.f;
        if (n < O) {
            if (PACKED)      // out[q][ntile][j][lane][t] = W[32 ntile + lane % 32][32 q + 8 j + 4 (lane / 32) + t]  (kernels_gemm.hip)
                v = in[(((((size_t)(k >> 5) * NT32 + nt) * 4 + ((k & 31) >> 3)) * 64 + ((k & 7) >> 2) * 32 + (n & 31)) << 2) + (k & 3)];
            else
                v = in[(size_t)n * I + k];
        }
        out[i] = (_Float16)v;       // round to nearest even; |w| > 65504 would become Inf (no trained weight is near it)
    }
}

#define GH_VARIANT(ACT, NRES) { "gemm_f16<act=" #ACT ",nres=" #NRES ">", gemm_f16_kernel<ACT, NRES>, GH_LDS_BYTES, 0ull }
GemmVariant<GemmParams> g_ghv[] = { GH_VARIANT(0, 0), GH_VARIANT(1, 0), GH_VARIANT(0, 1) };      // what the network uses: qkv / before_quant, fc1, proj / fc2
constexpr int kNumGH = sizeof(g_ghv) / sizeof(g_ghv[0]);

template <bool PACKED>
int repack_k1_f16(hipStream_t s, const float *in, int O, int I, void *out)
{
    FEMASR_REQUIRE(in && out && O > 0 && I > 0 && (I % 64) == 0, "repack_k1_f16: needs a (out, in) weight with in %% 64 == 0");
    const size_t total = femasr_packed_weight_k1_f16_bytes(O, I) / sizeof(unsigned short);
    hipLaunchKernelGGL(repack_k1_f16_kernel<PACKED>, dim3(grid_for(total)), dim3(256), 0, s, in, O, I, (_Float16 *)out, total);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

}  // namespace

// the k1 shape rule of the split GEMM: the two forms take the same 1x1 layers
bool femasr_gemm_f16_shape_ok(const femasr_conv_args *a) { return a->ksz == 1 && femasr_gemm_bf16s_shape_ok(a); }
int femasr_gemm_f16_variant_count() { return kNumGH; }
const char *femasr_gemm_f16_variant_name(int v) { return (v >= 0 && v < kNumGH) ? g_ghv[v].name : "?"; }

// plain, GELU, one residual
int femasr_gemm_f16_pick_variant(const femasr_conv_args *a) { return a->act == FEMASR_ACT_GELU ? 1 : ((a->res1 || a->res2) ? 2 : 0); }

int femasr_gemm_f16_launch(hipStream_t s, const femasr_conv_args *a, int *variant_out, double *flops_out)
{
    FEMASR_REQUIRE(a && a->in && a->w_f16 && femasr_gemm_f16_shape_ok(a), "gemm_f16: not a 1x1 stride-1 layer with Cin %% 64 == 0 and no prologue");
    FEMASR_REQUIRE(a->out, "gemm_f16: out must be set");
    const int nres = (a->res1 ? 1 : 0) + (a->res2 ? 1 : 0);
    FEMASR_REQUIRE(nres <= 1 && !(nres && a->act == FEMASR_ACT_GELU),
                   "gemm_f16: the kernel has three epilogues - plain, GELU, one residual -, not act %d with %d residual operands", a->act, nres);
    GemmParams p{};
    FEMASR_CHECK(gemm_params(a, "gemm_f16", a->H, a->W, a->Cin, p));
    p.W = a->w_f16;
    return gemm_variant_launch(s, g_ghv, femasr_gemm_f16_pick_variant(a), 128, p, variant_out, flops_out);
}

// the fp16 image of a 1x1 layer from its GEMM-layout fp32 image (femasr_repack_oihw, kh = kw = 1): model.hip, first selection of linear_math 2
int femasr_repack_packed_k1_f16(hipStream_t stream, const float *packed, int O, int I, void *out) { return repack_k1_f16<true>(stream, packed, O, I, out); }

extern "C" {

size_t femasr_packed_weight_k1_f16_bytes(int O, int I)
{
    if (O <= 0 || I <= 0 || (I % 64) != 0) return 0;
    return (size_t)(I / 16) * ((O + 31) / 32) * 64 * sizeof(uint4);
}

int femasr_repack_k1_f16(void *stream, const float *w_oi, int O, int I, void *out) { return repack_k1_f16<false>((hipStream_t)stream, w_oi, O, I, out); }

}  // extern "C"

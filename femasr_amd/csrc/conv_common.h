// conv_common.h — definitions shared by the conv and GEMM kernel translation units: the launch parameters, uniform-base global
// loads / stores, the epilogue transpose scratch, and the host launcher of the two matrix-core halo forms (device frame: halo_mma.h)
#pragma once
#include "common.h"

namespace {

struct ConvParams {
    const float *in, *w, *bias, *pro_a, *pro_b, *pro_c, *res1, *res2;
    const float *w_wino;  // Winograd-domain weights (femasr_repack_oihw_wino), kernels_wino.hip only
    const float *w_up2;   // 4 phase matrices of a nearest-x2 3x3 conv (femasr_repack_oihw_up2), halo kernels only
    float *out;
    const float *vq_zz, *vq_ee;
    float *vq_part;
    int vq_nblk;
    double *gn_part;      // fused GroupNorm partial moments of the OUTPUT, [B][tiles][32][2] (halo kernels) or null
    int B, H, W, Cin, Cout, ksz, stride, pad, up2, act, Ho, Wo;
    int M, K, nchunks, taps, MB, NB, NT32;
    int tilesX, tilesY;
    int kperm;            // conv_igemm: weights are in the GEMM layout of the 1x1 layers (k order 0,4,1,5,.. inside groups of 8)
};

constexpr int BK = 32;
constexpr int ALD = BK + 1;

// Uniform base (SGPR pair) + 32-bit unsigned per-lane BYTE offset: the global_load/store "saddr + voffset" form.  The
// readfirstlane on both halves pins the (truly uniform) pointer into SGPRs and stops LLVM re-associating
// (base + lane offset) + uniform offset into per-element 64-bit VALU adds (which then stay live across batched loads).
typedef __attribute__((address_space(1))) const float *gcptr_f32;
typedef __attribute__((address_space(1))) float *gptr_f32;

__device__ __forceinline__ unsigned long long uniform_u64(unsigned long long a)
{
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ float ldg_u32(const float *ubase, unsigned byteoff)
{
    const unsigned long long a = uniform_u64(reinterpret_cast<unsigned long long>(ubase));
    return *reinterpret_cast<gcptr_f32>(a + byteoff);
}
__device__ __forceinline__ void stg_u32(float *ubase, unsigned byteoff, float v)
{
    const unsigned long long a = uniform_u64(reinterpret_cast<unsigned long long>(ubase));
    *reinterpret_cast<gptr_f32>(a + byteoff) = v;
}

typedef float f32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4_t ldg4_u32(const float *ubase, unsigned byteoff)
{
    const unsigned long long a = uniform_u64(reinterpret_cast<unsigned long long>(ubase));
    return *reinterpret_cast<__attribute__((address_space(1))) const f32x4_t *>(a + byteoff);
}
__device__ __forceinline__ void stg4_u32(float *ubase, unsigned byteoff, f32x4_t v)
{
    const unsigned long long a = uniform_u64(reinterpret_cast<unsigned long long>(ubase));
    *reinterpret_cast<__attribute__((address_space(1))) f32x4_t *>(a + byteoff) = v;
}
constexpr int TPITCH = 36;                   // epilogue transpose scratch: 32 rows x 36 floats per wave (16-byte rows)
constexpr int TSCRATCH = 32 * TPITCH;        // floats per wave
// matrix-core halo forms (halo_mma.h): the scratch starts 8 KiB past the LDS base, behind the GroupNorm `red` area of the fused partials
// ([WM][BN][2] doubles, 4 KiB in the widest tilings; HaloFrame asserts it)
constexpr int HALO_EPI_OFF = 2048;           // floats

// two fp32 -> one dword of two fp16, round to nearest even, clamped to the largest finite half first (a finite input never becomes Inf)
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pack_f16(float x0, float x1)
{
    x0 = __builtin_fminf(__builtin_fmaxf(x0, -65504.f), 65504.f);
    x1 = __builtin_fminf(__builtin_fmaxf(x1, -65504.f), 65504.f);
    const f16x2 h = {(_Float16)x0, (_Float16)x1};
    return __builtin_bit_cast(unsigned, h);
}

__device__ __forceinline__ float f4get(const float4 &v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w)); }

// 32-column weight tile a wave reads for its accumulator tile t: tiles past the packed matrix (Cout not a multiple of the
// block width) are clamped to the last real tile - their products land in columns >= Cout, which are never stored - so
// the fragment loads never leave the packed buffer.
__device__ __forceinline__ int wtile(int n0, int t, int nt32)
{
    const int idx = (n0 >> 5) + t;
    return idx < nt32 ? idx : nt32 - 1;
}

__device__ __forceinline__ int xcd_remap(int bid, int nblk)
{
    const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7, within = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + within;
}

// Host side of the two matrix-core halo forms (kernels_conv_bf16.hip, kernels_conv_f16.hip): a row of a form's variant table and the
// launch of the row `pick` names.  who: the first word of the messages; image: the form's weight fragments (the field of *a, or null).
struct HaloVariant {
    const char *name;
    int bn, threads;
    void (*kern)(const ConvParams, const uint4 *, double *);
    size_t lds;
    unsigned long long attr_devs;       // bit d: MaxDynamicSharedMemorySize set on device d (the attribute is per device)
};

template <int N>
int halo_variant_launch(hipStream_t s, const femasr_conv_args *a, const char *who, HaloVariant (&table)[N], const void *image,
                        bool (*shape_ok)(const femasr_conv_args *), int (*pick)(const femasr_conv_args *), int *variant_out, double *flops_out)
{
    FEMASR_REQUIRE(a && a->in && a->bias && a->out && image && shape_ok(a), "%s: not eligible", who);
    const int Hv = a->up2 ? 2 * a->H : a->H, Wv = a->up2 ? 2 * a->W : a->W;
    FEMASR_REQUIRE(Hv == a->Ho && Wv == a->Wo, "%s: Ho/Wo mismatch", who);
    if (a->prologue == FEMASR_PRO_GN_SILU) FEMASR_REQUIRE(a->pro_a && a->pro_b, "%s: GN prologue needs a,b", who);
    ConvParams p{};
    p.in = a->in; p.bias = a->bias; p.pro_a = a->pro_a; p.pro_b = a->pro_b; p.res1 = a->res1; p.res2 = a->res2; p.out = a->out;
    p.B = a->B; p.H = a->H; p.W = a->W; p.Cin = a->Cin; p.Cout = a->Cout; p.ksz = 3; p.stride = 1; p.pad = 1; p.up2 = a->up2;
    p.Ho = Hv; p.Wo = Wv; p.NT32 = (a->Cout + 31) / 32;
    const int vi = pick(a);
    HaloVariant &v = table[vi];
    p.tilesX = (p.Wo + 15) / 16;
    p.tilesY = (p.Ho + 7) / 8;
    p.MB = a->B * p.tilesX * p.tilesY;
    p.NB = (a->Cout + v.bn - 1) / v.bn;
    FEMASR_CHECK(femasr_allow_dynamic_lds((const void *)v.kern, &v.attr_devs, v.lds + 40 * 1024));
    size_t lds = v.lds + (a->prologue == FEMASR_PRO_GN_SILU ? (size_t)2 * a->Cin * sizeof(float) : 0);
    const size_t epi = (HALO_EPI_OFF + (size_t)(v.threads / 64) * TSCRATCH) * sizeof(float);       // epilogue transpose scratch
    if (lds < epi) lds = epi;
    FEMASR_REQUIRE(!a->gn_part || (a->Cout % 32 == 0 && (a->Cout / 32) <= 8 && ((a->Cout / 32) & (a->Cout / 32 - 1)) == 0),
                   "%s: fused GN moments need Cout = 32 * {1, 2, 4, 8} (32 groups, power-of-two channels per group)", who);
    hipLaunchKernelGGL(v.kern, dim3((unsigned)(p.MB * p.NB)), dim3((unsigned)v.threads), lds, s, p, (const uint4 *)image, (double *)a->gn_part);
    FEMASR_CHECK_HIP(hipGetLastError());
    if (variant_out) *variant_out = vi;
    if (flops_out) *flops_out = 2.0 * (double)a->B * p.Ho * p.Wo * (double)a->Cout * 9.0 * a->Cin;
    return FEMASR_OK;
}

}  // namespace

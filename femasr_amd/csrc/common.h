// common.h — internal declarations shared by the .hip translation units of libfemasr_hip.so
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/femasr_hip_debug.h"      // (includes femasr_hip.h)

// thread-local error message plumbing (model.hip)
int femasr_set_error(int code, const char *fmt, ...);
#define FEMASR_CHECK_HIP(expr)                                                            \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess)                                                             \
            return femasr_set_error(FEMASR_ERR_HIP, "%s failed: %s (%s:%d)", #expr,       \
                                    hipGetErrorString(_e), __FILE__, __LINE__);           \
    } while (0)
#define FEMASR_REQUIRE(cond, ...)                                                         \
    do {                                                                                  \
        if (!(cond)) return femasr_set_error(FEMASR_ERR_INVALID, __VA_ARGS__);            \
    } while (0)

// A launch with more than 64 KiB of dynamic LDS needs the kernel's MaxDynamicSharedMemorySize raised first.  The attribute is per device:
// *devs holds one bit per device on which `kern` already has it (one mask per kernel, zero-initialised).  Idempotent: a race between
// threads only repeats the call.
inline int femasr_allow_dynamic_lds(const void *kern, unsigned long long *devs, size_t bytes)
{
    int dev = 0;
    FEMASR_CHECK_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64 || !((__atomic_load_n(devs, __ATOMIC_ACQUIRE) >> dev) & 1ull)) {
        FEMASR_CHECK_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        if (dev >= 0 && dev < 64) __atomic_fetch_or(devs, 1ull << dev, __ATOMIC_RELEASE);
    }
    return FEMASR_OK;
}
#define FEMASR_CHECK(expr) do { const int _rc = (expr); if (_rc != FEMASR_OK) return _rc; } while (0)

// blocks of 256 threads for a grid-stride kernel over `total` items (relayouts, tile copies, weight repacks): at most 4096, at least one
inline unsigned grid_for(size_t total)
{
    const size_t g = (total + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

// device helpers that more than one translation unit uses
namespace {
__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
}  // namespace

// conv launcher with the VQ-argmin epilogue option (kernels_conv.hip)
//   vq_part != nullptr : instead of storing the tile, each block writes, per row, the
//   first-min (distance, column) over its BN columns of d = (vq_zz[row] + vq_ee[col]) - 2*acc
//   to vq_part[(row*vq_nblk + nblock)*2 + {0,1}] (column stored as a float-bit-cast int).
struct conv_vq_epilogue {
    const float *zz;
    const float *ee;
    float *part;
    int nblk;
};
int femasr_conv2d_launch(hipStream_t s, const femasr_conv_args *a, const conv_vq_epilogue *vq,
                         int *variant_out, double *flops_out);
int femasr_conv2d_pick_variant(const femasr_conv_args *a);      // the variant femasr_conv2d_launch runs (no VQ epilogue); shape-only
int femasr_conv_variant_count();
const char *femasr_conv_variant_name(int v);
bool femasr_conv_halo_eligible(const femasr_conv_args *a);      // 3x3 s1 p1, Cin % 32 == 0: the halo kernels
// fused GroupNorm(32) partial moments in a halo conv's epilogue: channels per group a power of two <= 32
inline bool femasr_gn_fusable(int cout) { const int cg = cout / 32; return cout % 32 == 0 && cg >= 1 && cg <= 32 && (cg & (cg - 1)) == 0; }

// convs with <= 4 output channels and a 3x3 stride-1 halo shape (out_conv) keep a compact [k][4] weight copy behind the
// fragment-major matrix for the direct VALU kernel (an MFMA tile would compute 32 columns for 3)
inline size_t femasr_compact_weight_floats(int O, int I, int kh, int kw)
{
    return (O <= 4 && kh == 3 && kw == 3 && (I % 32) == 0) ? (size_t)I * 9 * 4 : 0;
}

// 1x1 convs / nn.Linear / VQ distance matrix on the LDS-DMA GEMM (kernels_gemm.hip)
bool femasr_gemm_eligible(const femasr_conv_args *a);
int femasr_gemm_launch(hipStream_t s, const femasr_conv_args *a, const conv_vq_epilogue *vq, int *variant_out, double *flops_out);
int femasr_gemm_variant_count();
int femasr_gemm_pick_variant(const femasr_conv_args *a, bool vq);
const char *femasr_gemm_variant_name(int v);
int femasr_repack_k1(hipStream_t s, const float *in, int O, int I, float *out);

// What the translation unit of a conv form defines under its prefix besides the launch: the pointer-free shape rule, the variant table
// (names in profile-slot order) and the variant a call runs (shape-only)
#define FEMASR_FORM_DECLS(prefix)                                          \
    bool femasr_##prefix##_shape_ok(const femasr_conv_args *a);            \
    int femasr_##prefix##_variant_count();                                 \
    const char *femasr_##prefix##_variant_name(int v);                     \
    int femasr_##prefix##_pick_variant(const femasr_conv_args *a)

// 1x1 convs / nn.Linear as an fp32-grade product on the bf16 matrix pipe (kernels_gemm_bf16.hip); shape_ok: a 1x1 layer or the 3x3 form
FEMASR_FORM_DECLS(gemm_bf16s);
bool femasr_conv3x3_bf16s_shape_ok(const femasr_conv_args *a);      // the 3x3 pad-1 form (K = 9 Cin, stride 1 or 2) of the same kernel
int femasr_gemm_bf16s_launch(hipStream_t s, const femasr_conv_args *a, const void *w_bf16s, int *variant_out, double *flops_out);

// Winograd F(4x4,3x3) 3x3 convs (kernels_wino.hip)
constexpr int FEMASR_WINO_LOG2_TOTAL = 31, FEMASR_WINO_LOG2_IMAGE = 27;      // element limits of the Winograd-form kernels (32-bit byte offsets)
FEMASR_FORM_DECLS(conv_wino);
int femasr_conv_wino_launch(hipStream_t s, const femasr_conv_args *a, int *variant_out, double *flops_out);
bool femasr_conv_wino_shape_ok_lim(const femasr_conv_args *a, int log2_total, int log2_image);      // a handle's planner may lower the limits (femasr_debug_set_wino_limits)
int femasr_conv_wino_gn_tiles(int H, int W);      // fused GroupNorm partials of a Winograd conv: one per 16x16-pixel sub-block
// nn.Upsample(x2) + 3x3 conv in the 25-product Winograd-type form (kernels_wino_up2.hip), one variant; GroupNorm partials per 16x16 OUTPUT sub-block
bool femasr_conv_wino_up2_shape_ok(const femasr_conv_args *a);
bool femasr_conv_wino_up2_shape_ok_lim(const femasr_conv_args *a, int log2_total, int log2_image);
int femasr_conv_wino_up2_launch(hipStream_t s, const femasr_conv_args *a, double *flops_out);
const char *femasr_conv_wino_up2_variant_name();

// bf16x3 3x3 halo convs (kernels_conv_bf16.hip)
FEMASR_FORM_DECLS(conv_bf16x3);
int femasr_conv_bf16x3_launch(hipStream_t s, const femasr_conv_args *a, int *variant_out, double *flops_out);
// one-pass fp16 3x3 halo convs (kernels_conv_f16.hip): the bf16x3 form's layers and shape rule, FEMASR_DECODER_MATH_FP16
FEMASR_FORM_DECLS(conv_f16);
int femasr_conv_f16_launch(hipStream_t s, const femasr_conv_args *a, int *variant_out, double *flops_out);
// the fp16 image built from the layer's fragment-major fp32 image (femasr_repack_oihw of a 3x3 conv with I % 32 == 0) instead of the OIHW tensor
int femasr_repack_packed_f16(hipStream_t stream, const float *packed, int O, int I, void *out);

// one-pass fp16 GEMM of the 1x1 layers (kernels_gemm_f16.hip): the split GEMM's k1 layers and shape rule, FEMASR_LINEAR_MATH_FP16
FEMASR_FORM_DECLS(gemm_f16);
int femasr_gemm_f16_launch(hipStream_t s, const femasr_conv_args *a, int *variant_out, double *flops_out);
// the fp16 image built from the layer's GEMM-layout fp32 image (femasr_repack_oihw with kh = kw = 1) instead of the (out, in) tensor
int femasr_repack_packed_k1_f16(hipStream_t stream, const float *packed, int O, int I, void *out);

// The forms a conv runs in, in profile-slot order (femasr_create lays the slots out from this list)
enum ConvForm {
    CONV_DIRECT,      // fp32 halo / implicit-GEMM kernels, the VALU out_conv kernel (kernels_conv.hip, kernels_gemm.hip)
    CONV_BF16X3,      // bf16x3 halo kernels (w_bf16x3)
    CONV_WINO,        // Winograd F(4x4,3x3) (w_wino)
    CONV_WINO_UP2,    // the 25-product form of nearest-x2 + 3x3 conv (w_wino with up2)
    CONV_SPLIT,       // split-bf16 GEMM: 1x1 / linear layer, or 3x3 conv over K = 9 Cin (w_bf16s)
    CONV_F16,         // one-pass fp16 halo kernels (w_f16 with ksz = 3)
    CONV_GEMM_F16,    // one-pass fp16 GEMM of a 1x1 layer (w_f16 with ksz = 1); new forms go last, so the slots of the others keep their numbers
    CONV_FORM_COUNT
};

// Everything the library knows about a form, one row each in kConvForms (conv_forms.hip): a new form is an enum value, a row, its kernel
// file and its place in conv_form()'s precedence (model.hip).
struct ConvFormDesc {
    ConvForm form;      // the row's own index (femasr_create asserts it)
    // the kernels: variants in profile-slot order, the variant a call runs (shape-only), the launch
    int (*variant_count)();
    const char *(*variant_name)(int v);
    int (*pick_variant)(const femasr_conv_args *a);
    int (*launch)(hipStream_t s, const femasr_conv_args *a, int *variant_out, double *flops_out);
    // the weight image: the femasr_conv_args field that carries it (offsetof), its size and its repack from the torch-layout tensor
    // (OIHW with ksz x ksz taps, (out, in) with ksz = 1); from_packed, where the form has one, builds it from the layer's CONV_DIRECT image
    size_t field;
    size_t (*image_bytes)(int O, int I, int ksz);
    int (*repack)(const float *w, int O, int I, int ksz, void *out);
    int (*from_packed)(hipStream_t s, const float *packed, int O, int I, void *out);
    // femasr_conv2d runs the form of lowest `rank` whose image is given and whose `chosen` (null = always) holds, and refuses with
    // `refusal` unless the pointer-free shape rule (null = the launch checks) accepts the call
    int rank;
    bool (*chosen)(const femasr_conv_args *a);
    bool (*shape_ok)(const femasr_conv_args *a);
    const char *refusal;
    // fused GroupNorm partial moments a conv of this form writes when its output feeds a GroupNorm: tiles per sample (null = none: the
    // GroupNorm then runs the stand-alone moments kernel, which gives the same coefficients bit for bit)
    int (*gn_tiles)(const femasr_conv_args *a);
};
const ConvFormDesc &femasr_conv_form_desc(int f);      // row f of kConvForms, f a ConvForm
inline const void *femasr_conv_form_image(int f, const femasr_conv_args *a)
{
    const void *p;
    __builtin_memcpy(&p, (const char *)a + femasr_conv_form_desc(f).field, sizeof p);
    return p;
}
inline void femasr_conv_form_set_image(int f, femasr_conv_args *a, const void *image) { __builtin_memcpy((char *)a + femasr_conv_form_desc(f).field, &image, sizeof image); }
// Launches the conv in form f (the form's weight image in its femasr_conv_args field).  *slot_out: the launch's profile slot counted
// from the first conv slot (variants of the forms before f, then the variant that ran).
int femasr_conv_form_launch(hipStream_t s, ConvForm f, const femasr_conv_args *a, int *slot_out, double *flops_out);

// conv_forms.hip — host code only: kConvForms, the table with one row per conv form (variants, launch, weight image, femasr_conv2d's
// precedence and refusals, fused GroupNorm partials), and what reads it: femasr_conv_form_desc / _launch and femasr_conv2d.
#include "common.h"
#include <string.h>

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

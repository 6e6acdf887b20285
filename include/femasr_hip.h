/*
 * femasr_hip.h — flat C ABI of libfemasr_hip.so (MI355X / gfx950 HIP kernels for the
 * FeMaSR SR-inference hot path).
 *
 * The reference is pure PyTorch: it has NO native boundary for this path
 * (SURVEY 2.2).  Each entry point therefore cites the reference *Python* interface
 * whose arithmetic it replaces; `INTEGRATION.md` shows the ctypes binding a
 * reference maintainer would add (it is the binding femasr_amd/_lib.py uses).
 *
 * Conventions
 *   - plain pointers + sizes only; every tensor pointer is a DEVICE pointer owned by the
 *     caller (e.g. torch allocations, `.data_ptr()`); the library never frees or keeps
 *     them past the call, except weights, which `femasr_set_weight` COPIES (repacked)
 *     into allocations the handle owns and frees in `femasr_destroy`.
 *   - `stream` is a hipStream_t passed as void* (0 = default stream); all work is
 *     enqueued on it, no hidden synchronisation (except set_weight/finalize, which sync).
 *   - activations inside the library are NHWC fp32 ("tokens (B,HW,C)" == NHWC);
 *     NCHW only at femasr_forward / femasr_decode_indices / pad / crop edges.
 *   - every function returns 0 on success or a negative femasr_status; the message is
 *     available from femasr_last_error() (thread-local).  No C++ exception crosses the ABI.
 *   - a handle is bound to one device and is not thread-safe; one handle per rank.
 */
#ifndef FEMASR_HIP_H
#define FEMASR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    FEMASR_OK = 0,
    FEMASR_ERR_INVALID = -1,   /* bad argument / unsupported configuration */
    FEMASR_ERR_HIP = -2,       /* a HIP runtime call failed                */
    FEMASR_ERR_WEIGHT = -3,    /* unknown key, wrong shape, or missing weight at finalize */
    FEMASR_ERR_WORKSPACE = -4  /* workspace too small                      */
} femasr_status;

typedef struct femasr_handle femasr_handle;

/* Mirrors FeMaSRNet.__init__ keyword arguments (basicsr/archs/femasr_arch.py:216-228).  codebook_params rows
 * [scale, n_e, e_dim] in ascending scale order (femasr_arch.py:231-235); rows after the first are the multi-scale
 * quantisers of femasr_arch.py:277-300 (before_quant on cat(enc_feat, dec_feat), CombineQuantBlock fema_utils.py:87-99). */
#define FEMASR_MAX_CODEBOOKS 3
typedef struct {
    int32_t in_channel;      /* 3 */
    int32_t gt_resolution;   /* 256 */
    int32_t lq_stage;        /* LQ_stage */
    int32_t scale_factor;    /* 4 / 2 (ignored -> 1 when !lq_stage, femasr_arch.py:241) */
    int32_t use_quantize;
    int32_t use_residual;
    int32_t n_codebooks;     /* 1..FEMASR_MAX_CODEBOOKS */
    int32_t codebook_scale[FEMASR_MAX_CODEBOOKS];  /* e.g. {32} */
    int32_t n_e[FEMASR_MAX_CODEBOOKS];             /* e.g. {1024} */
    int32_t e_dim[FEMASR_MAX_CODEBOOKS];           /* e.g. {512} */
    int32_t device;          /* HIP device ordinal the handle is bound to */
} femasr_config;

const char *femasr_last_error(void);
/* 100 * major + minor.  107 (additive since: femasr_repack_k1_f16 / femasr_packed_weight_k1_f16_bytes, the ksz = 1 meaning of w_f16 and
 * femasr_set_linear_math mode 2; the struct layout and every earlier entry point are unchanged, so the number stays): femasr_conv_args ends with w_f16; femasr_repack_oihw_f16 / femasr_packed_weight_f16_bytes; femasr_set_decoder_math takes 4 ('fp16').  106: femasr_blend_tiles / femasr_blend_tiles_u8 (the opt-in overlap-blend paste).  105: the femasr_niqe_* and femasr_imresize* entry points.  104: the femasr_psnr_ssim* entry points and femasr_ssim_window.  103: FEMASR_ACT_RELU and the femasr_lpips_* entry points (femasr_conv_args is unchanged).  102: the debug hooks moved to femasr_hip_debug.h; femasr_mlp_fused and the process-global femasr_debug_wino_* switches are gone;
 * femasr_extract_tiles_u8 / femasr_paste_tiles_u8 are new (femasr_conv_args is unchanged since 101). */
int femasr_version(void);

/* ---- model handle ------------------------------------------------------------------ */
int femasr_create(const femasr_config *cfg, femasr_handle **out);
void femasr_destroy(femasr_handle *h);

/* Number of weight tensors the configuration expects, and the i-th key / shape
 * (state-dict names and torch layouts of the reference, SURVEY 8b "Weights"). */
int femasr_num_weights(const femasr_handle *h);
int femasr_weight_info(const femasr_handle *h, int i, const char **key, int64_t shape[4], int *ndim);

/* Copy one fp32 tensor (device pointer, torch layout: conv OIHW, linear (out,in), vectors)
 * into the handle, repacking conv/linear weights to the K-major layout of femasr_conv_args.w.
 * Replaces nn.Module.load_state_dict for the path (inference_femasr.py:40). */
int femasr_set_weight(femasr_handle *h, const char *key, const float *dev_ptr,
                      const int64_t *shape, int ndim);
/* Verify every expected weight was set; build derived tensors (codebook^T, |e|^2). */
int femasr_finalize_weights(femasr_handle *h);

/* Number of internal streams the batch is split over (default 1).  Samples are independent (every op is
 * per-sample), so sub-batches run concurrently on separate streams, forked from / joined to the caller's
 * stream by events only; results are bit-identical for any n.  Call before femasr_workspace_bytes. */
int femasr_set_streams(femasr_handle *h, int n);

/* pad_mode 1 = FeMaSRNet.test geometry (mirror-pad to (h/wsz+1)*wsz, crop to h*s; femasr_arch.py:449-468)
 * pad_mode 0 = FeMaSRNet.forward (no pad, output (H*s_out) as produced; femasr_arch.py:470-479)          */
int femasr_workspace_bytes(const femasr_handle *h, int B, int H, int W, int pad_mode, size_t *bytes);

/* Shapes of one call: the output image (out_h, out_w), and per codebook the index map (idx_h[q], idx_w[q]) (arrays of
 * FEMASR_MAX_CODEBOOKS ints).  Follows the reference geometry exactly, including test()'s truncated mirror pad of images
 * smaller than the pad when there is no Swin stage (femasr_arch.py:454-465). */
int femasr_forward_shapes(const femasr_handle *h, int H, int W, int pad_mode, int *out_h, int *out_w, int *n_index_maps,
                          int *idx_h, int *idx_w);

/* Whole hot path: in NCHW fp32 (B,3,H,W) -> out NCHW fp32 (B,3,out_h,out_w) and, if non-NULL, the VQ index maps int64
 * of all codebooks back to back, map q = (B,1,idx_h[q],idx_w[q]).  Replaces FeMaSRNet.encode_and_decode
 * (femasr_arch.py:311-374) inside .test / .forward.  `ws` must be >= femasr_workspace_bytes and 256-byte aligned.
 * Batch size: the planner gives every conv the fastest form whose offset range holds its tensors (femasr_conv_args, size limits); a
 * batch whose activations pass 2^31 elements per tensor (x4: more than 101 tiles of 128^2, 25 windows of 272^2 in one call) still
 * computes every image, on the slower 64-bit forms (256 tiles of 128^2 in one call: the indices of calls of 16, the image within 1e-5 of
 * theirs; tests/test_gpu_product_anchor.py), so splitting it is faster,
 * never more correct.  Only B*Ho*Wo >= 2^31 - 256 pixels of one layer is refused (FEMASR_ERR_INVALID, before any launch).
 * Every entry point runs on the handle's device and restores the caller's current device before returning. */
int femasr_forward(femasr_handle *h, void *stream, const float *in_nchw, int B, int H, int W,
                   int pad_mode, float *out_nchw, int64_t *indices, void *ws, size_t ws_bytes);

/* The same forward on uint8 images, the step either side of the path fused into its first and last kernel: in (B,H,W,3)
 * uint8 HWC (swap_rb = 1: cv2's BGR) -> (float)u8 / 255.0f inside the mirror-pad kernel (img2tensor + `/255.`: basicsr/utils/img_util.py:9-35,
 * inference_femasr.py:54-56); out (B,out_h,out_w,3) uint8 HWC = clamp [0,1], x255, round half to even inside the crop kernel (tensor2img,
 * img_util.py:38-94, inference_femasr.py:64-67).  No fp32 NCHW image makes a pass of its own; same bits as femasr_image_u8_to_f32 ->
 * femasr_forward -> femasr_image_f32_to_u8. */
int femasr_forward_u8(femasr_handle *h, void *stream, const uint8_t *in_hwc, int B, int H, int W, int swap_rb, int pad_mode,
                      uint8_t *out_hwc, int64_t *indices, void *ws, size_t ws_bytes);
int femasr_pad_u8hwc_to_nhwc(void *stream, const uint8_t *in, int B, int H, int W, int swap_rb, int Hp, int Wp, float *out);
int femasr_crop_nhwc_to_u8hwc(void *stream, const float *in, int B, int Hs, int Ws, int Hc, int Wc, int swap_rb, uint8_t *out);

/* indices (B,1,h,w) int64 -> image NCHW (B,3,8h,8w).  Replaces FeMaSRNet.decode_indices
 * (femasr_arch.py:376-385) incl. VectorQuantizer.get_codebook_entry (:102-112). */
int femasr_decode_workspace_bytes(const femasr_handle *h, int B, int hq, int wq, size_t *bytes);
int femasr_decode_indices(femasr_handle *h, void *stream, const int64_t *indices, int B, int hq, int wq,
                          float *out_nchw, void *ws, size_t ws_bytes);

/* The network as an encoder (image -> VQ index maps, no decoder) and the code-usage histogram of index maps: declared in
 * femasr_hip_encode.h, which is part of this interface and is included here. */
#include "femasr_hip_encode.h"

/* Per-kernel timing (HIP events recorded on `stream` around every launch) while enabled.
 * Slots = one per conv_igemm instantiation + one per small-kernel family; femasr_profile_get
 * synchronises the recorded events and returns, for launches since the last reset, the summed
 * milliseconds, launch count and algorithmic FLOPs (0 for the HBM-bound families) / bytes. */
int femasr_profile_enable(femasr_handle *h, int on);
int femasr_profile_reset(femasr_handle *h);
int femasr_profile_slots(const femasr_handle *h);
const char *femasr_profile_name(const femasr_handle *h, int slot);
int femasr_profile_get(femasr_handle *h, int slot, double *ms, int64_t *launches, double *flops, double *bytes);

/* ---- per-kernel entry points (unit parity tests; same kernels femasr_forward launches) ---- */

/* test() pad + layout: NCHW (B,C,H,W) -> NHWC (B,Hp,Wp,C), mirror rows/cols (femasr_arch.py:454-460). */
int femasr_pad_nchw_to_nhwc(void *stream, const float *in, int B, int C, int H, int W, int Hp, int Wp, float *out);
/* crop + layout: NHWC (B,Hs,Ws,C) -> NCHW (B,C,Hc,Wc) top-left (femasr_arch.py:464-465). */
int femasr_crop_nhwc_to_nchw(void *stream, const float *in, int B, int Hs, int Ws, int C, int Hc, int Wc, float *out);

enum { FEMASR_PRO_NONE = 0, FEMASR_PRO_GN_SILU = 1, FEMASR_PRO_LN = 2 /* retired: LayerNorm is femasr_layernorm, a separate pass */ };
enum { FEMASR_ACT_NONE = 0, FEMASR_ACT_GELU = 1, FEMASR_ACT_RELU = 2 /* v > 0 ? v : +0 (LPIPS backbones; direct fp32 forms only) */ };

/* Convolution / linear on fp32 MFMA.  Replaces nn.Conv2d (femasr_arch.py:150,159,173,
 * 203,273,298; fema_utils.py:75,78,90; network_swinir.py:465), nn.Upsample(x2) fused on load
 * (femasr_arch.py:172,202), nn.Linear (network_swinir.py:19-21,105-112; ksz=1 on (1,rows,1,Cin)),
 * GroupNorm-apply+SiLU fused on load, bias / GELU / residual adds fused on store.
 * Kernel families: 3x3 stride-1 pad-1 with Cin % 32 == 0 -> halo kernels; 1x1 stride-1 with Cin % 32 == 0 (every
 * nn.Linear) -> the LDS-DMA GEMM; everything else -> the general implicit GEMM. */
typedef struct {
    const float *in;      /* (B,H,W,Cin) NHWC, pre-upsample size */
    int32_t B, H, W, Cin;
    const float *w;       /* packed weights as emitted by femasr_repack_oihw (fragment-major, see there) */
    const float *bias;    /* [Cout] */
    int32_t Cout, ksz, stride, pad, up2;
    int32_t prologue;     /* FEMASR_PRO_* */
    const float *pro_a;   /* GN: a[B][Cin] */
    const float *pro_b;   /* GN: b[B][Cin] */
    const float *pro_c;   /* unused (was LN beta) */
    int32_t act;          /* FEMASR_ACT_* (applied after bias, before residuals); RELU: the direct fp32 halo / implicit-GEMM forms only */
    const float *res1;    /* optional (B,Ho,Wo,Cout) added after act   */
    const float *res2;    /* optional second residual                   */
    float *out;           /* (B,Ho,Wo,Cout) */
    int32_t Ho, Wo;
    const void *w_bf16x3; /* optional: femasr_repack_oihw_bf16x3 weights.  When non-NULL and the layer is a 3x3
                             stride-1 pad-1 conv with Cin % 32 == 0 (no LN prologue / GELU) it runs on the bf16
                             matrix cores with the 3-term hi/lo split (NOT bit-exact: every output element is within
                             128 * 2^-24 * sum_k |t_k w_k| of the exact conv - t the activated input -, plus the fp32
                             roundings of bias / residuals and the prologue SiLU's 8 ulp; tests/fp64_ref.py
                             C_FORM['bf16x3'], tests/test_gpu_mode_anchor.py); NULL = exact fp32 */
    double *gn_part;      /* optional, 3x3 stride-1 halo convs (exact fp32 and bf16x3): per-(sample, 8x16 tile, group)
                             partial GroupNorm(32) moments (sum, sum of squares) of the OUTPUT,
                             [B][tilesY*tilesX][32][2] doubles, for femasr_gn_coeffs_from_partials (saves the separate
                             moments pass over the tensor).  fp32 path: exactly the partials of the specified
                             summation order (bit-identical coefficients to femasr_gn_coeffs); needs Cout/32 a power of
                             two <= 32 (bf16x3: <= 8); anything else is refused.  With up2 on the exact path (phase filters) the
                             partials are per HALF-resolution tile and phase: [B][4*ceil(H/8)*ceil(W/16)][32][2], index
                             tile*4 + 2a + b (oracle: orc_gn_coeffs(..., phases = 1)). */
    const float *w_up2;   /* up2 = 1 on a 3x3 stride-1 pad-1 conv with Cin % 32 == 0 (exact fp32 path): the four phase
                             matrices of femasr_repack_oihw_up2 -- nn.Upsample(x2, nearest) + Conv2d evaluated as four
                             2x2-tap filters on the low-resolution input (REQUIRED for that shape; other up2 shapes
                             read the upsampled image through `w`). */
    const float *w_wino;  /* optional: femasr_repack_oihw_wino weights.  When non-NULL the layer (3x3 stride-1 pad-1, no
                             x2, Cin % 32 == 0, Cout % 64 == 0, no GELU) runs in the Winograd F(4x4,3x3) form: fp32
                             throughout, 4x fewer multiplies, results within fp32 rounding (~1e-5 relative at worst) of the
                             direct form and bit-identical to oracle/femasr_oracle.c orc_conv3x3_winograd.  The model uses
                             it for the convs behind the codebook lookup only (they cannot move a VQ index).  With gn_part the
                             partials are per 16x16-pixel sub-block: [B][ceil(H/16)*ceil(W/16)][32][2] (orc_gn_coeffs mode 2).
                             With up2 = 1: femasr_repack_oihw_wino_up2 weights, the 25-product form of nearest-x2 + conv
                             (no prologue; partials per 16x16-pixel OUTPUT sub-block; orc_conv_up2_winograd). */
    int32_t fast_act;     /* Winograd convs with the GN+SiLU prologue only: 1 = SiLU through the hardware exp2 / rcp units
                             (v_exp_f32, v_rcp_f32: 1 ulp each) instead of the IEEE-exact polynomial + division - ~6x fewer
                             VALU instructions in the staging; output within ~1e-6 relative of the exact form (no longer
                             bit-identical to the oracle).  0 = exact. */
    const float *in_add;  /* optional second INPUT tensor of the same (B,H,W,Cin) shape: the conv reads in + in_add (one fp32 add per
                             element while staging).  Only the x2 Winograd-type form takes it (up2 = 1 with w_wino; anything else refuses):
                             FeMaSRNet's decoder adds the encoder's skip feature to a stage's input (`x = x + enc_feats[i]`,
                             femasr_arch.py:361-362) right in front of that stage's x2 conv, so the sum never makes a pass of its own. */
    const void *w_bf16s;  /* optional (struct version 101): femasr_repack_k1_bf16s weights.  When non-NULL the layer - a 1x1 stride-1 conv /
                             nn.Linear with Cin % 64 == 0, no prologue (network_swinir.py:19-21,105-107,121,143; femasr_arch.py:298), or (round 6, weights from
                             femasr_repack_oihw_bf16s) a 3x3 pad-1 conv of stride 1 or 2 with Cin % 64 == 0, no prologue, no activation - runs on
                             the bf16 matrix pipe as an fp32-GRADE product: both operands split exactly into three bf16 terms, the six
                             partial products of relative size >= 2^-16 accumulated in fp32 (two accumulators), ~3x closer to the fp64
                             result than the fp32 fmaf chain and bit-identical to oracle/femasr_oracle.c orc_linear_bf16s, which restates
                             the instruction's accumulation arithmetic from hardware probes (kernels_gemm_bf16.hip).  `w` is not read. */
    const void *w_f16;    /* optional (struct version 107): femasr_repack_oihw_f16 weights.  When non-NULL the layer - under the shape and size
                             rule of w_bf16x3: 3x3 stride-1 pad-1, Cin % 32 == 0, no LN prologue / activation, no prologue with up2 - runs on
                             the fp16 matrix cores in ONE pass (HALF-precision grade, NOT within the 1e-3 bound of the other forms):
                               t   = the activated input in fp32 (GroupNorm apply + SiLU on the hardware exp2 / rcp units as in the
                                     w_bf16x3 prologue, nearest-x2 folded in, zero outside the image)
                               t16 = fp16_rne(clamp(t, +-65504))      (a finite input never becomes Inf)
                               w16 = fp16_rne(w), packed once; fp16 subnormals of either operand take part with their value
                               out = bias + residuals + sum_k t16_k * w16_k: products exact in fp32 (11 + 11 bits), accumulated in fp32
                                     by v_mfma_f32_32x32x16_f16; bias and residuals added in fp32; the output is stored as fp32.
                             Every output element is within 128 * 2^-24 * sum_k |t16_k w16_k| of conv(t16, w16) evaluated exactly, plus
                             the fp32 roundings of bias / residuals and, with the prologue, one fp16 ulp of t_k times |w16_k| wherever the
                             SiLU's 8 fp32 ulp straddle an fp16 rounding boundary (tests/test_gpu_decoder_fp16.py).  gn_part as for
                             w_bf16x3 (Cout / 32 a power of two <= 8).  `w` is not read.
                             With ksz = 1 (the k1 meaning; weights from femasr_repack_k1_f16): a 1x1 stride-1 layer / nn.Linear under the k1 shape
                             rule of w_bf16s (Cin % 64 == 0, pad 0, no prologue, no up2) runs as ONE fp16 GEMM pass (kernels_gemm_f16.hip):
                               a16 = fp16_rne(clamp(a, +-65504)) of the fp32 input row, w16 = fp16_rne(w) (subnormals with their value)
                               out = epi(bias + sum_k a16_k * w16_k): products exact, accumulated in fp32 by v_mfma_f32_32x32x16_f16 with k
                                     ascending; bias (may be NULL = 0) in fp32; act = GELU by the split GEMM's device function; ONE residual
                                     (res1 or res2) added in fp32; stored as fp32.
                             Three epilogues exist - plain, GELU, one residual -; GELU with a residual, or two residuals, is refused.  Every
                             output element is within 128 * 2^-24 * sum_k |a16_k w16_k| + 2 * 2^-24 (|bias| + |res| + |ref|) of the exact value
                             (tests/test_gpu_linear_fp16.py).  FeMaSRNet's linear_math 'fp16' uses both meanings for the layers in FRONT of the
                             codebook lookup: VQ indices may then differ from the other modes (femasr_set_linear_math). */
} femasr_conv_args;
/* Size limits (each a shape rule evaluated before any launch; DESIGN.md 5.7, tests/test_gpu_product_anchor.py):
 *   rows B*Ho*Wo < 2^31 - 256 for every form, else FEMASR_ERR_INVALID;
 *   w_wino: < 2^31 elements per tensor and < 2^27 per image (32-bit byte offsets), else FEMASR_ERR_INVALID;
 *   w_bf16x3 and w_f16: B*H*W*Cin < 2^31 and B*Ho*Wo*Cout < 2^31 (tests/test_gpu_mode_anchor.py), the 3x3 form of w_bf16s: B*H*W*Cin < 2^31,
 *   else FEMASR_ERR_INVALID;
 *   the direct form (none of those weights given): the 3x3 stride-1 halo kernels and the Cout = 3 kernel hold the input patch
 *   offset as a 32-bit ELEMENT offset and are used while B*H*W*Cin < 2^31; a larger input - 2^32 elements and more included - runs
 *   on the generic implicit GEMM, whose offsets are 64-bit (slower; gn_part is then not accepted).  Nothing wraps silently. */
int femasr_conv2d(void *stream, const femasr_conv_args *a);

/* GroupNorm(32,eps) moments folded into per-(n,c) scale/shift: y = fmaf(x,a,b) (fema_utils.py:22).
 * scratch: >= femasr_gn_scratch_bytes(B,H,W,C,G) bytes. */
size_t femasr_gn_scratch_bytes(int B, int H, int W, int C, int G);
int femasr_gn_coeffs(void *stream, const float *x, int B, int H, int W, int C, int G,
                     const float *gamma, const float *beta, float eps, float *a, float *b, void *scratch);
/* Same as femasr_gn_coeffs, from the partial moments a halo conv wrote with femasr_conv_args.gn_part
 * (tiles = ceil(H/8)*ceil(W/16) of the producing conv's output). */
int femasr_gn_coeffs_from_partials(void *stream, const double *part, int B, int tiles, int H, int W, int C, int G,
                                   const float *gamma, const float *beta, float eps, float *a, float *b);
/* y = silu(fmaf(x, a[n][c], b[n][c])) on an NHWC tensor: the GroupNorm-apply + SiLU of a ResBlock conv (fema_utils.py:73-74,76-77) as a
 * pass of its own, in the arithmetic of the conv kernels' GN+SiLU prologue (IEEE-exact SiLU; oracle: orc_scale_shift_silu).  Used in
 * front of the 3x3 convs that run as the split-bf16 GEMM (w_bf16s with ksz = 3), which take their input without a prologue. */
int femasr_gn_silu_apply(void *stream, const float *x, int B, int H, int W, int C, const float *a, const float *b, float *y);
/* LayerNorm(C=256) row moments -> stats[rows][2] = (mean, rstd) (network_swinir.py:199,205). */
int femasr_ln_stats(void *stream, const float *x, int64_t rows, int C, float eps, float *stats);
/* y = LayerNorm(x) over the last dim (C = 256): the same moments, then fmaf((x-mean)*rstd, gamma, beta)
 * (network_swinir.py:243,277: norm1 / norm2 ahead of qkv / fc1). */
int femasr_layernorm(void *stream, const float *x, int64_t rows, int C, const float *gamma, const float *beta,
                     float eps, float *y);
/* 8x8 (shifted-)window multi-head attention incl. rel-pos bias and shift mask
 * (network_swinir.py:114-145, 216-237, 249-272).  qkv (B,H*W,3C) -> out (B,H*W,C), natural token order. */
int femasr_window_attention(void *stream, const float *qkv, int B, int H, int W, int C, int heads, int shift,
                            const float *table, float *out);
/* VectorQuantizer.forward (femasr_arch.py:35-38,50-100): z (M,D) rows; cbT = femasr_repack_oihw(cb, n_e, D, 1, 1);
 * ee[j] = |e_j|^2 (femasr_row_sqsum).  Writes idx (M) int64 first-min, zq (M,D) straight-through.
 * scratch: >= (M*(n_e/128)*2 + M + 64) floats. */
int femasr_vq(void *stream, const float *z, int64_t M, int D, const float *cb, const float *cbT,
              const float *ee, int n_e, int64_t *idx, float *zq, void *scratch);
int femasr_row_sqsum(void *stream, const float *x, int64_t rows, int D, float *out);
/* The same lookup as a two-pass EXACT search (kernels_vq.hip): a bf16-MFMA pass keeps, from a rigorous error bound, the
 * few codes per row that can be the fp32 first-min; the specified fp32 chain is then evaluated for those only.
 * Results are bit-identical to femasr_vq.  Shapes: e_dim a power of two in 64..512, n_e % 64 == 0, n_e <= 1024
 * (femasr_vq_twopass_ok); aux = femasr_vq_prepare(cb, ee) image of femasr_vq_aux_bytes bytes;
 * scratch >= femasr_vq_scratch_bytes(M, n_e) bytes (covers femasr_vq too).  femasr_vq_twopass is ONE launch that keeps its
 * candidate lists on chip: it requires a non-null `scratch` and never reads or writes it (the argument stays in the ABI). */
int femasr_vq_twopass_ok(int n_e, int D);
size_t femasr_vq_aux_bytes(int n_e, int D);
int femasr_vq_prepare(void *stream, const float *cb, const float *ee, int n_e, int D, void *aux);
size_t femasr_vq_scratch_bytes(int64_t M, int n_e);
int femasr_vq_twopass(void *stream, const float *z, int64_t M, int D, const float *cb, const void *aux, const float *ee,
                      int n_e, int64_t *idx, float *zq, void *scratch);
/* Pass 1 alone: cand (M,32) uint16 candidate codes, cnt (M) uint16 count (0xFFFF = every code).  Every one of the M * 32 slots is
 * written: a row's cnt codes in ascending order, then zeros (all 32 zero where cnt = 0xFFFF).  The list always holds the row's fp32
 * first-min, but WHICH other codes it holds may differ from run to run: a code is kept when it is under the row's threshold at the moment
 * its tile is scanned, and the waves that tighten the threshold run concurrently (a few more exact evaluations, never a lost minimum). */
int femasr_vq_candidates(void *stream, const float *z, int64_t M, int D, const void *aux, const float *ee, int n_e,
                         uint16_t *cand, uint16_t *cnt);
int femasr_codebook_gather(void *stream, const int64_t *idx, int64_t M, int D, const float *cb, int n_e, float *zq);
/* out (B,H,W,Ca+Cb) = cat(a (B,H,W,Ca), nearest-resize(b (B,Hb,Wb,Cb) -> H x W)) along channels: torch.cat((x, y), 1) of
 * femasr_arch.py:334 (Hb,Wb == H,W) and CombineQuantBlock's F.interpolate + cat (fema_utils.py:92-99; source index
 * floor(dst * Hb / H), exact for the integer ratios the architecture produces). */
int femasr_concat_resize(void *stream, const float *a, int Ca, const float *b, int Hb, int Wb, int Cb, int B, int H, int W,
                         float *out);
/* test_tile (femasr_arch.py:387-447) on the device.  extract: the n input windows of ONE shape class (th x tw, top-left corners
 * yx_dev[2k], yx_dev[2k+1], int32 on the device) of a (B,C,H,W) image -> a (n*B, C, th, tw) batch (tile-major, as
 * torch.cat of the reference's crops).  paste: the upscaled tile bodies -> the (B,C,Ho,Wo) canvas;
 * rects_dev[6k..] = (src_y, src_x, dst_y, dst_x, h, w) in upscaled pixels, hmax = max h.  Tiles of different ranks are pasted
 * after the all-gather, which stays in the host's torch.distributed (RCCL) group: see INTEGRATION.md. */
int femasr_extract_tiles(void *stream, const float *in, int B, int C, int H, int W, const int32_t *yx_dev, int n, int th, int tw,
                         float *out);
int femasr_paste_tiles(void *stream, const float *tiles, int B, int C, int n, int th, int tw, const int32_t *rects_dev, int hmax,
                       int Ho, int Wo, float *out);
/* The same on uint8 HWC images (3 channels): crops of a (B,H,W,3) image -> (n*B, th, tw, 3), ready for femasr_forward_u8; tile bodies of
 * (n*B, th, tw, 3) -> the (B,Ho,Wo,3) canvas.  FeMaSRNet.test_tile_u8 and the all-gather of the multi-GPU path move these bytes - a
 * quarter of the fp32 tiles' - and the CLI's tiled branch (inference_femasr.py:58-67) never holds an fp32 image. */
int femasr_extract_tiles_u8(void *stream, const uint8_t *in, int B, int H, int W, const int32_t *yx_dev, int n, int th, int tw, uint8_t *out);
int femasr_paste_tiles_u8(void *stream, const uint8_t *tiles, int B, int n, int th, int tw, const int32_t *rects_dev, int hmax,
                          int Ho, int Wo, uint8_t *out);
/* Overlap-blend paste (opt-in, FeMaSRNet.test_tile(..., blend=True); NOT the reference's arithmetic, which discards the halos): every
 * canvas pixel becomes the weighted mean of the upscaled WINDOWS that contain it,
 *   out[b,c,Y,X] = sum_k w_k(Y,X) v_k[b,c,Y-Ay_k,X-Ax_k] / sum_k w_k(Y,X),   w_k = wy_k(Y) wx_k(X),
 * over the covering tiles k in row-major order, with the 1-D weight of window coordinate i in [0, len) and margins lead / trail
 *   min(lead ? min(1, (2i+1) / (4 lead)) : 1,  trail ? min(1, (2(len-1-i)+1) / (4 trail)) : 1)
 * (a linear ramp across the overlap, centred on the body edge).  fp32, no contraction: w = (float)num / (float)(4 margin),
 * acc and den summed from 0 in tile order, out = acc / den; the uint8 form accumulates (float)byte and stores rintf of the quotient
 * clamped to [0, 255] (half to even, as tensor2img).  One launch per canvas, gather form: no atomics, every canvas element is written
 * exactly once and never read, so the canvas need not be initialised.
 *   tile_ptrs_dev[k]  device address of tile k (row-major tile number), image 0: fp32 (C, th, tw) / uint8 (th, tw, 3); image b of the
 *                     batch follows b * C*th*tw (3*th*tw) elements later - the tile-major layout of femasr_extract_tiles' batches
 *   geom_dev[8k..]    (window origin y, x on the canvas, th, tw, lead_y, trail_y, lead_x, trail_x) in upscaled pixels; margin 0 = image border
 *   tiles_y, tiles_x  the tile grid, n == tiles_y * tiles_x;  pitch = tile_size * scale, the body pitch; needs 2 tile_pad <= tile_size, so
 *                     that only a pixel's own cell and its +-1 neighbours can cover it
 * Refused with FEMASR_ERR_INVALID before any launch: a null pointer; n, B, C or a size <= 0; n != tiles_y * tiles_x; tiles_x > 65535;
 * B*C*Ho (uint8: B*Ho) >= 2^31 canvas rows.  The tables are the caller's (tiling.blend_table): the kernel only guarantees that a read
 * driven by them stays inside the th x tw tile they name (memory safety for a hand-made table, not validation; a pixel that no listed
 * window contains is written as 0). */
int femasr_blend_tiles(void *stream, const uint64_t *tile_ptrs_dev, const int32_t *geom_dev, int n, int tiles_y, int tiles_x, int pitch,
                       int B, int C, int Ho, int Wo, float *out);
int femasr_blend_tiles_u8(void *stream, const uint64_t *tile_ptrs_dev, const int32_t *geom_dev, int n, int tiles_y, int tiles_x, int pitch,
                          int B, int Ho, int Wo, uint8_t *out);

/* OIHW -> the packed FRAGMENT-MAJOR weight layout of femasr_conv_args.w (also nn.Linear (out,in) with kh=kw=1
 * and the codebook for femasr_vq):  out[q][ntile][lane][kk], zero padded, with
 *   K index k = ((ci/32)*kh*kw + ky*kw + kx)*32 + ci%32 when I % 32 == 0, else (ky*kw + kx)*I + ci;
 *   q = k/32, kk = (k%32)/2, lane = (k&1)*32 + o%32, ntile = o/32.
 * 1x1 layers with I % 32 == 0 (kh = kw = 1: nn.Linear, 1x1 convs, the codebook) get the GEMM layout instead:
 *   out[q][ntile][j][lane][t] = W[o = 32*ntile + lane%32][k = 32q + 8j + 4*(lane/32) + t]   (same size).
 * 3x3 layers with O <= 4 and I % 32 == 0 (out_conv) additionally carry a compact [k][4] copy behind the matrix (the
 * direct VALU kernel reads it through scalar loads); femasr_packed_weight_floats includes it.
 * `out` must hold femasr_packed_weight_floats(O,I,kh,kw) floats. */
size_t femasr_packed_weight_floats(int O, int I, int kh, int kw);
int femasr_repack_oihw(void *stream, const float *in, int O, int I, int kh, int kw, float *out);
/* 3x3 OIHW -> femasr_conv_args.w_up2: phase (a,b) of nearest-x2 + conv reads input rows {y-1+a, y+a} and columns
 * {x-1+b, x+b}; slot weights are the fp32 sums of the taps that land on the same input pixel (rows summed over kx first,
 * ascending; then over ky, ascending).  out: femasr_up2_weight_floats(O, I) floats = 4 x femasr_packed_weight_floats(O,I,2,2). */
size_t femasr_up2_weight_floats(int O, int I);
/* 3x3 OIHW -> femasr_conv_args.w_wino: U = G g G^T (6x6 per (o, i)) of F(4x4,3x3), down the columns then along the rows in
 * the operation order of oracle/femasr_oracle.c orc_g6, stored [Cin/8][36 components][Cout/32][lane][4] (the MFMA B fragments
 * of one 8-channel step: 1 KiB per wave load).  out: femasr_wino_weight_floats(O, I) floats = 36 * I * 32*ceil(O/32).
 * The layout is private to the library (pack and launch through it). */
size_t femasr_wino_weight_floats(int O, int I);
int femasr_repack_oihw_wino(void *stream, const float *in, int O, int I, float *out);
/* The same for the conv behind nn.Upsample(x2, nearest) (femasr_arch.py:172-173,202-203): a 4x4 output tile reads a 4x4 patch of
 * the low-resolution input, which leaves 5 products per dimension - 25 components per (o, i) instead of 36, layout
 * [Cin/8][25][Cout/32][lane][4].  Pass the result as femasr_conv_args.w_wino together with up2 = 1 (no prologue; Cin % 32 == 0,
 * Cout % 64 == 0).  GroupNorm partial moments (gn_part) come per 16x16-pixel OUTPUT sub-block, as for the F(4x4,3x3) form. */
size_t femasr_wino_up2_weight_floats(int O, int I);
int femasr_repack_oihw_wino_up2(void *stream, const float *w_oihw, int O, int I, float *out);
int femasr_repack_oihw_up2(void *stream, const float *in, int O, int I, float *out);

/* (out, in) fp32 -> femasr_conv_args.w_bf16s: the three bf16 planes of every weight (w = w1 + w2 + w3 exactly), packed
 * [Cin/16][ceil(Cout/32)][plane][lane][8 bf16] - the MFMA B fragments of one 16-channel step, 1 KiB per (column tile, plane). */
size_t femasr_packed_weight_bf16s_bytes(int O, int I);
int femasr_repack_k1_bf16s(void *stream, const float *w_oi, int O, int I, void *out);
/* The same for a 3x3 conv weight (O, I, 3, 3), I % 64 == 0: the planes of the (9 I x O) matrix of the conv's implicit GEMM, k = (3 ky + kx) I + c.
 * With such weights in w_bf16s a 3x3 pad-1 conv of stride 1 or 2 (no prologue, no activation; bias and residual operands as usual) runs as the
 * split-bf16 GEMM over K = 9 Cin: the same arithmetic as the linear layers (oracle: conv3x3_bf16s = im2col + orc_linear_bf16s).  FeMaSRNet
 * (linear_math 'bf16_split') uses it for the 3x3 convs in FRONT of the codebook lookup - the encoder's ResBlocks (femasr_arch.py:150-164,
 * fema_utils.py:65-84) and the conv behind every RSTB (network_swinir.py:465). */
size_t femasr_packed_weight_conv3x3_bf16s_bytes(int O, int I);
int femasr_repack_oihw_bf16s(void *stream, const float *w_oihw, int O, int I, void *out);
/* (out, in) fp32 -> femasr_conv_args.w_f16 of a 1x1 layer (ksz = 1): fp16 (round to nearest even), packed [Cin/16][ceil(Cout/32)][lane][8 halves] -
 * the MFMA B fragments of one 16-channel step, 1 KiB per column tile, zero padded in Cout.  Cin % 64 == 0 (bytes: 0 otherwise). */
size_t femasr_packed_weight_k1_f16_bytes(int O, int I);
int femasr_repack_k1_f16(void *stream, const float *w_oi, int O, int I, void *out);
/* The mode values of femasr_set_linear_math / femasr_set_decoder_math (described below), by name. */
enum { FEMASR_LINEAR_MATH_FP32 = 0, FEMASR_LINEAR_MATH_BF16_SPLIT = 1, FEMASR_LINEAR_MATH_FP16 = 2, FEMASR_LINEAR_MATH_COUNT };
enum { FEMASR_DECODER_MATH_FP32 = 0, FEMASR_DECODER_MATH_BF16X3 = 1, FEMASR_DECODER_MATH_FP32_DIRECT = 2, FEMASR_DECODER_MATH_FP32_STRICT = 3,
       FEMASR_DECODER_MATH_FP16 = 4, FEMASR_DECODER_MATH_COUNT };
/* Arithmetic of the network's 1x1 convs / nn.Linear layers (the Swin qkv / proj / fc1 / fc2 and before_quant) and of the 3x3 convs in front of
 * the codebook lookup:
 * 1 (default, 'bf16_split'): the fp32-grade product on the bf16 matrix pipe described at femasr_conv_args.w_bf16s;
 * 0 ('fp32'): one fp32 fmaf chain per output on the fp32 MFMA (kernels_gemm.hip), bit-identical to OracleNet(linear_math='fp32');
 * 2 ('fp16', opt-in): HALF-precision grade in front of the lookup.  Exactly the layers mode 1 sends to the split GEMM are taken: the 1x1
 *    stride-1 layers run as the one-pass fp16 GEMM (w_f16 with ksz = 1), the 3x3 stride-1 pad-1 convs that pass the w_f16 shape rule run in the
 *    one-pass fp16 halo form with its fused GroupNorm + SiLU prologue (hardware exp2 / rcp units) and fused GroupNorm partials - the
 *    stand-alone femasr_gn_silu_apply pass in front of them and the moments pass behind them disappear.  Everything else (stride-2 convs,
 *    in_conv, attention, LayerNorm, the lookup) runs as in mode 1.  Results are deterministic and bitwise independent of batch size, streams,
 *    graph replay and tiling within the mode, but VQ indices are NOT guaranteed equal to the other modes' and the image is NOT within their
 *    1e-3 bound: a token whose two nearest codes are nearly tied may flip, and the image changes locally by up to ~0.1 of unit range there
 *    (DESIGN.md 17 has the measured rates).  Orthogonal to femasr_set_decoder_math.  The fp16 weight images are built when the mode is first
 *    selected and kept current by femasr_set_weight from then on; a handle that never selects it allocates nothing for it. */
int femasr_set_linear_math(femasr_handle *h, int mode);

/* Split-bf16 (hi/lo) fragment-major weights for the opt-in bf16x3 conv path (3x3 convs behind the VQ lookup). */
size_t femasr_packed_weight_bf16x3_bytes(int O, int I, int kh, int kw);
int femasr_repack_oihw_bf16x3(void *stream, const float *in, int O, int I, int kh, int kw, void *out);
/* fp16 (round to nearest even) fragment-major weights for the opt-in one-pass fp16 conv path (femasr_conv_args.w_f16); I % 32 == 0. */
size_t femasr_packed_weight_f16_bytes(int O, int I, int kh, int kw);
int femasr_repack_oihw_f16(void *stream, const float *in, int O, int I, int kh, int kw, void *out);
/* 0 (default, 'fp32'): every layer fp32; in single-codebook networks the 3x3 convs that do NOT feed the codebook lookup
 *    (after_quant, DecoderBlocks, the LQ encoder's two up-blocks) run in the Winograd F(4x4,3x3) form (4x fewer multiplies)
 *    with the GroupNorm+SiLU prologue on the hardware exp2 / rcp units (femasr_conv_args.fast_act): same fp32 accuracy against
 *    the reference (~1e-5), VQ indices bit-exact (everything that feeds a lookup stays in the exact direct form), the image
 *    within ~1e-5 of the oracle.
 * 3 ('fp32_strict'): the same with the IEEE-exact SiLU: bit-identical to the oracle (OracleNet()).
 * 1: those convs (and the x2 convs) use the bf16x3 path instead: output within the north-star 1e-3 bound of the fp32 result
 *    (measured ~1e-4).
 * 2 ('fp32_direct'): fp32 with every conv in the direct form, bit-identical to OracleNet(winograd=False).
 * 4 ('fp16'): the convs that mode 1 sends to the bf16x3 path (behind every lookup, Cout > 4, the w_bf16x3 shape rule) run in the one-pass
 *    fp16 form of femasr_conv_args.w_f16 instead; every other layer runs as in mode 2 (out_conv: the exact VALU kernel).  VQ indices
 *    are bit-identical to every other mode (nothing in front of a lookup changes); the IMAGE is half-precision grade, about 5e-4 of the
 *    output range from the fp32 image - NOT within the 1e-3 bound of modes 0-3.  The fp16 weight images are built when the mode is first
 *    selected and rebuilt by femasr_set_weight from then on; a handle that never selects it allocates nothing for it. */
int femasr_set_decoder_math(femasr_handle *h, int mode);

/* ---- image pre / post-processing (the steps either side of the path) ---- */
/* uint8 HWC (3 channels; swap_rb=1 for cv2-style BGR input) -> fp32 CHW RGB in [0,1]: (float)u8 / 255.0f.
 * Replaces img2tensor(...)/255. (basicsr/utils/img_util.py:9-35, inference_femasr.py:54-56). */
int femasr_image_u8_to_f32(void *stream, const uint8_t *in_hwc, int H, int W, int swap_rb, float *out_chw);
/* fp32 CHW RGB -> clamp [0,1] -> (x*255).round() half-to-even -> uint8 HWC (swap_rb=1: BGR for cv2.imwrite).
 * Replaces tensor2img (basicsr/utils/img_util.py:38-94). */
int femasr_image_f32_to_u8(void *stream, const float *in_chw, int H, int W, int swap_rb, uint8_t *out_hwc);

/* ---- LPIPS v0.1 (inference): validation's key metric (pyiqa 'lpips' = AlexNet, 'lpips-vgg' = VGG16; femasr_model.py:27-34,262) ----
 * A handle holds one backbone and its five linear heads.  Weight keys are canonical: net.sliceK.I.weight / .bias (K = 1..5, I = the
 * torchvision `features` index: alex 0, 3, 6, 8, 10; vgg16 0, 2 | 5, 7 | 10, 12, 14 | 17, 19, 21 | 24, 26, 28) and linK.model.1.weight
 * (K = 0..4, shape (1, C_k, 1, 1)).  set_weight copies (conv weights repacked by femasr_repack_oihw) and synchronises.  Every conv has
 * a bias and a ReLU (FEMASR_ACT_RELU on the exact fp32 conv forms); the taps are the ReLU outputs of alex conv0/3/6/8/10 and vgg16
 * relu1_2/2_2/3_3/4_3/5_3.  Minimum input: H, W >= 31 (alex) / 16 (vgg16), below that FEMASR_ERR_INVALID and nothing is launched;
 * shapes whose largest feature tensor of the 2B-image batch reaches 2^31 elements are refused as well (split the batch). */
typedef struct femasr_lpips_handle femasr_lpips_handle;
int femasr_lpips_create(int net /* 0 alex, 1 vgg16 */, int device, femasr_lpips_handle **out);
void femasr_lpips_destroy(femasr_lpips_handle *h);
int femasr_lpips_set_weight(femasr_lpips_handle *h, const char *key, const float *dev_ptr, const int64_t *shape, int ndim);
int femasr_lpips_finalize_weights(femasr_lpips_handle *h);     /* FEMASR_ERR_WEIGHT names the first missing key */
int femasr_lpips_workspace_bytes(const femasr_lpips_handle *h, int B, int H, int W, size_t *bytes);
/* x0, x1: (B,3,H,W) fp32 NCHW RGB in [0,1].  out[B] = lpips.LPIPS.forward(x0, x1, normalize=True) per pair; per_layer [B][5] the five
 * spatially averaged tap terms (may be NULL).  `ws` >= femasr_lpips_workspace_bytes, 256-byte aligned. */
int femasr_lpips_forward(femasr_lpips_handle *h, void *stream, const float *x0_nchw, const float *x1_nchw, int B, int H, int W,
                         float *out, float *per_layer, void *ws, size_t ws_bytes);
/* Per-op units of the forward (the same kernels; unit tests compose them):
 * scale_input: x0, x1 (B,3,H,W) NCHW -> out (2B,H,W,3) NHWC, x0 in samples 0..B-1, x1 in B..2B-1; t = 2x - 1, then
 *   (t - shift) / scale, shift = (-.030, -.088, -.188), scale = (.458, .448, .450) as fp32.
 * tap: f (B2,H,W,C) NHWC ReLU features of the 2B-image batch (C % 64 == 0, 64..512), w_lin [C] the head.  For each pair b < B2/2 and
 *   pixel: n = f / (sqrt(sum_c f^2) + 1e-10) for f[b] and f[b + B2/2], value = sum_c w_lin[c] (n0 - n1)^2 in fp32; one fp64 partial
 *   sum per 32-pixel block: partials [B2/2][femasr_lpips_tap_partials(H, W)].  pool 1: max-pool 3x3 / 2, pool 2: 2x2 / 2 (no padding,
 *   floor) of f into pooled_out (B2, Hp, Wp, C) in the same launch; pool 0: pooled_out unused.  Refused (nothing launched):
 *   a map too small for the pool, more than 65535 pairs.
 * finalize: partials of ntaps taps back to back (tap k: [B][femasr_lpips_tap_partials(tap_hw[2k], tap_hw[2k+1])]), tap_hw a HOST array
 *   [ntaps][2] -> per_layer [B][ntaps] (sum / (H_k W_k) in fp64, rounded to fp32; may be NULL) and out[B] (the terms summed in tap
 *   order in fp32).  Fixed summation order throughout, no atomics: deterministic and batch-invariant. */
int femasr_lpips_scale_input(void *stream, const float *x0_nchw, const float *x1_nchw, int B, int H, int W, float *out_nhwc);
int femasr_lpips_tap_partials(int H, int W);
int femasr_lpips_tap(void *stream, const float *f, int B2, int H, int W, int C, const float *w_lin, int pool, float *pooled_out,
                     double *partials);
int femasr_lpips_finalize(void *stream, const double *partials, int B, int ntaps, const int32_t *tap_hw, float *out, float *per_layer);

/* ---- PSNR / SSIM: validation's 'psnr' / 'ssim' metrics (femasr_model.py:29-34,259-262; calculate_psnr_ssim.py) ----
 * a, b: B pairs of (H,W,3) uint8 RGB HWC images, (B,H,W,3) back to back.  crop_border c scores [c:H-c, c:W-c]; test_y = 1 scores the fp64
 * BT.601 luma Y = (x/255) . [65.481, 128.553, 24.966] + 16 (not rounded), test_y = 0 the three channels as fp64.  Per pair, fp64 on the
 * device (each output may be NULL, not all three):
 *   mse_out[B]   mean of (a - b)² over the cropped pixels (and channels); in RGB mode numpy's value bit for bit (integer terms, exact sum)
 *   psnr_out[B]  10 log10(255² / mse), +inf where mse == 0
 *   ssim_out[B]  mean of the SSIM map over the (H-2c-10) x (W-2c-10) valid positions of an 11x11 Gaussian window (sigma 1.5), C1 = (0.01*255)²,
 *                C2 = (0.03*255)²; RGB: the three channel SSIMs averaged in channel order.  The window sums are scipy.signal.convolve2d's
 *                (same products, same order), so on the same plane the map is _ssim_plane's bit for bit (in RGB mode always; Y may
 *                differ from numpy's by 1 ulp where a BLAS sums the dot product in another order).
 * The definitions are calculate_psnr / calculate_ssim in femasr_amd/models/femasr_model.py.  Two launches (the two metrics' partials in one,
 * a fixed-order per-pair finalize), no atomics, no host synchronisation, nothing allocated: deterministic and batch-invariant.
 * Refused with FEMASR_ERR_INVALID before any launch: B < 1, B > 65535, test_y not 0 / 1, crop_border < 0, 2 crop_border >= H or >= W,
 * B H W 3 >= 2^31 and, when ssim_out is set, a cropped size below 11x11.  workspace_bytes sizes for any of the outputs (it cannot refuse
 * the last case); `ws` >= that size, 256-byte aligned.  femasr_ssim_window writes the 121 window weights (row-major, a HOST array). */
int femasr_psnr_ssim_workspace_bytes(int B, int H, int W, int crop_border, int test_y, size_t *bytes);
int femasr_psnr_ssim(void *stream, const uint8_t *a, const uint8_t *b, int B, int H, int W, int crop_border, int test_y, double *psnr_out,
                     double *ssim_out, double *mse_out, void *ws, size_t ws_bytes);
int femasr_ssim_window(double *win);

/* ---- imresize: MATLAB-style bicubic resize (basicsr/utils/matlab_functions.py:86), two passes over host-built tables ----
 * in: N planes of (H,W), float32 (is_f64 = 0) or float64 (1), back to back; out: (N,Ho,Wo) of the same type.  The H pass runs first, then the
 * W pass.  w_h, idx_h: (Ho,taps_h) weights and 0-based source rows of every output row, the symmetric padding already folded into the
 * indices (femasr_amd.models.femasr_model.imresize_tables builds them in fp64 for any scale and both antialiasing settings, and refuses a
 * length whose reflected index leaves the image); w_w, idx_w: (Wo,taps_w) likewise.  All four are DEVICE arrays.  Each output is one fp64
 * accumulator over its taps in ascending order from 0.0, no fma: the float64 output is the definition's (femasr_model.imresize) bit for bit,
 * the float32 output that value rounded once.  An index outside [0, n) is clamped (memory safety for a bad table; the result is then not
 * the definition's).  Refused with FEMASR_ERR_INVALID before any launch: an empty shape, N > 65535, a plane or a table of 2^31 elements or
 * more.  `ws` >= workspace_bytes (the fp64 intermediate, N Ho W), 256-byte aligned.  Two launches on `stream`, nothing allocated. */
int femasr_imresize_workspace_bytes(int N, int H, int W, int Ho, int Wo, size_t *bytes);
int femasr_imresize(void *stream, const void *in, int is_f64, int N, int H, int W, int Ho, int Wo, const double *w_h, const int32_t *idx_h,
                    int taps_h, const double *w_w, const int32_t *idx_w, int taps_w, void *out, void *ws, size_t ws_bytes);

/* ---- NIQE features: validation's no-reference 'niqe' metric (scripts/metrics/calculate_niqe.py) ----
 * img: B (H,W,3) uint8 RGB HWC images back to back.  crop_border c keeps [c:H-c, c:W-c]; of that the top-left 96 nh x 96 nw pixels
 * (nh = (H-2c) / 96, nw likewise) are scored.  All fp64 on the device, the definition being femasr_model.niqe_features:
 *   y = rint(((65.481 R + 128.553 G) + 24.966 B) / 255 + 16); per scale mu, sigma over the 7x7 `window` (49 fp64, row-major, as given:
 *   scipy.ndimage.convolve(mode='nearest') order) and z = (y - mu) / (sigma + 1); the second scale's plane is imresize(y / 255, 0.5) * 255
 *   through the tables w_h, idx_h (48 nh, taps_h) and w_w, idx_w (48 nw, taps_w) of femasr_imresize.  y and z of both scales are the
 *   definition's bits (femasr_niqe_plane_offsets: byte offsets of y, z, y2, z2 in `ws` after a call).
 *   features[B][nh nw][36]: per block (index iw nh + ih) and scale the 18 AGGD features; positions[B][nh nw][10]: per scale the grid
 *   position of each of the 5 alphas in arange(0.2, 10.001, 0.001).  `tables`: 5 x 9801 fp64: r_gam, gamma(1/gam), gamma(2/gam),
 *   gamma(3/gam), gam (femasr_model.aggd_tables).  Moments are summed in a fixed order that depends only on the block's own pixels: the
 *   features agree with the definition to rounding (1e-10 relative), are run-to-run deterministic and batch-invariant.
 * window, tables and the resize tables are DEVICE arrays.  Six launches on `stream`, no atomics, no host synchronisation, nothing
 * allocated.  Refused with FEMASR_ERR_INVALID before any launch: B < 1, B > 65535, crop_border < 0 or leaving nothing, fewer than one
 * 96x96 block after the crop, B H W 3 >= 2^31.  `ws` >= workspace_bytes (32 bytes per scored pixel), 256-byte aligned. */
int femasr_niqe_workspace_bytes(int B, int H, int W, int crop_border, size_t *bytes);
int femasr_niqe_plane_offsets(int B, int H, int W, int crop_border, size_t offsets[4]);
int femasr_niqe_features(void *stream, const uint8_t *img, int B, int H, int W, int crop_border, const double *window, const double *tables,
                         const double *w_h, const int32_t *idx_h, int taps_h, const double *w_w, const int32_t *idx_w, int taps_w,
                         double *features, int32_t *positions, void *ws, size_t ws_bytes);

/* ---- wavelet colour fix (opt-in, femasr_amd.colorfix / FeMaSRNet.test*(..., color_fix=True); NOT the reference's arithmetic) ----
 * The coarse bands of a super-resolved canvas are taken from its bicubically upsampled input:
 *   up = imresize(lq, s) (femasr_imresize's float32 result);  d = up - sr;  for i = 0 .. levels-1, r = 2^i, indices clamped to the plane:
 *   t[y,x] = (d[y,cl(x-r)]/4 + d[y,x]/2) + d[y,cl(x+r)]/4;  d'[y,x] = (t[cl(y-r),x]/4 + t[y,x]/2) + t[cl(y+r),x]/4;   out = sr + d.
 * Every step after the resize is one IEEE fp32 operation in the order written (tests/colorfix_ref.py restates it bit for bit).
 *   femasr_color_fix     sr, out: `planes` fp32 planes of (sH,sW) back to back ((B,C,sH,sW)); lq: as many planes of (H,W)
 *   femasr_color_fix_u8  sr, out: B uint8 (sH,sW,3) images; lq: B uint8 (H,W,3) images.  Planes are (float)byte / 255.0f (IEEE division); the
 *                        result is stored as rint(clamp(out, 0, 1) * 255), half to even (tensor2img's rounding).  It fixes the BYTES the
 *                        canvas holds, it is not the quantised fp32 fix.
 * `out` may be `sr` (in place).  w_h, idx_h: (sH,taps_h) and w_w, idx_w: (sW,taps_w): femasr_imresize's DEVICE tables for scale s, no
 * antialiasing.  `ws`: 256-byte aligned; femasr_color_fix_workspace_bytes(planes, ...) is what a group of `planes` planes needs (two fp32
 * buffers of (planes,sH,sW) and the resize's fp64 intermediate (planes,sH,W)).  The call works through its planes in groups of as many
 * planes as `ws_bytes` holds (a uint8 image is three planes: channel c of image b is plane 3 b + c), so a caller bounds the peak by sizing
 * the workspace for fewer planes than it passes - down to one, also for uint8: no canvas is ever held in fp32.  levels + 3 launches per group on `stream`; no atomics, no allocation, no synchronisation (capture-safe).
 * Refused with FEMASR_ERR_INVALID before any launch: a null pointer, a count or size <= 0, sH != s H or sW != s W, levels outside 1..12,
 * a plane of 2^31 elements or more, a workspace smaller than one plane's or not 256-byte aligned. */
int femasr_color_fix_workspace_bytes(int planes, int H, int W, int sH, int sW, int s, size_t *bytes);
int femasr_color_fix(void *stream, const float *sr, const float *lq, int planes, int H, int W, int sH, int sW, int s, int levels,
                     const double *w_h, const int32_t *idx_h, int taps_h, const double *w_w, const int32_t *idx_w, int taps_w, float *out,
                     void *ws, size_t ws_bytes);
int femasr_color_fix_u8(void *stream, const uint8_t *sr, const uint8_t *lq, int B, int H, int W, int sH, int sW, int s, int levels,
                        const double *w_h, const int32_t *idx_h, int taps_h, const double *w_w, const int32_t *idx_w, int taps_w, uint8_t *out,
                        void *ws, size_t ws_bytes);

/* ---- x8 geometric self-ensemble (opt-in, femasr_amd.ensemble / FeMaSRNet.test*(..., self_ensemble=True); NOT the reference's arithmetic) ----
 * The data movement around the eight forwards.  Variant k = 0..7: v = k & 1 flips rows, h = (k >> 1) & 1 flips columns,
 * t = (k >> 2) & 1 transposes, x_k = T^t(H^h(V^v(x))) per image and channel:
 *   expand  x (H,W) ->  k = 0..3 (H,W): x_k[i,j] = x[v ? H-1-i : i, h ? W-1-j : j];   k = 4..7 (W,H): x_k[i,j] = x[v ? H-1-j : j, h ? W-1-i : i]
 *   merge   z_k[i,j] = y_k[v ? H-1-i : i, h ? W-1-j : j] (k = 0..3, y_k of (H,W));   z_k[i,j] = y_k[h ? W-1-j : j, v ? H-1-i : i] (k = 4..7, y_k of
 *           (W,H));  H, W: the OUTPUT's.  fp32: out = 0.125f * (((((((z_0 + z_1) + z_2) + z_3) + z_4) + z_5) + z_6) + z_7), one IEEE fp32 add per
 *           step in this order.  uint8: S = sum_k z_k per byte, out = (S + 3 + ((S >> 3) & 1)) >> 3 (S / 8, half to even): the mean of the
 *           BYTES, not the quantised fp32 mean.
 * Buffers are variant-major: straight (4,B,C,H,W) / (4,B,H,W,3) holds k = 0..3, transposed (4,B,C,W,H) / (4,B,W,H,3) holds k = 4..7.  With H == W
 * a caller may pass transposed = straight + 4 B C H W elements and treat all eight variants as one batch.  No buffer of a call may overlap
 * another otherwise.  One launch per call on `stream`; no atomics, no allocation, no synchronisation (capture-safe); 64-bit offsets.
 * Refused with FEMASR_ERR_INVALID before any launch: a null pointer, a count or size <= 0, a plane of 2^31 elements or more, more than
 * 2^31 - 1 tiles of 64x64 in all. */
int femasr_dihedral_expand(void *stream, const float *x, int B, int C, int H, int W, float *straight, float *transposed);
int femasr_dihedral_expand_u8(void *stream, const uint8_t *x, int B, int H, int W, uint8_t *straight, uint8_t *transposed);
int femasr_dihedral_merge(void *stream, const float *straight, const float *transposed, int B, int C, int H, int W, float *out);
int femasr_dihedral_merge_u8(void *stream, const uint8_t *straight, const uint8_t *transposed, int B, int H, int W, uint8_t *out);

/* ---- PNG row filters (opt-in, femasr_amd.pngio: the GPU stage of the fast PNG output; changes no pixel) ----
 * img: uint8 (B,H,W,3) -> out: uint8 (B,H,1 + 3W), the byte stream PNG deflates for colour type 2, bit depth 8, no interlace.
 * Per row y of an image, n = 3W, raw[y] its n bytes, and per byte i with x = raw[y][i]:
 *   a = raw[y][i-3] (0 if i < 3),  b = raw[y-1][i] (0 if y == 0),  c = raw[y-1][i-3] (0 if either is outside)
 *   f0 = x,  f1 = x - a,  f2 = x - b,  f3 = x - ((a + b) >> 1),  f4 = x - paeth(a, b, c)   (mod 256)
 *   paeth: p = a + b - c, pa = |p - a|, pb = |p - b|, pc = |p - c|: a if pa <= pb and pa <= pc, else b if pb <= pc, else c
 *   cost_t = sum_i min(f_t[i], 256 - f_t[i]);   out[y] = [t, f_t[0], ..., f_t[n-1]]
 * filter = 0..4: t = filter for every row; filter = 5 (adaptive): per row the smallest t of least cost.  Integer work: the result is
 * bit-identical to femasr_amd.pngio.filter_rows.  img and out need no alignment and must not overlap.  One launch on `stream`; no
 * workspace, no atomics, no allocation, no synchronisation (capture-safe); 64-bit offsets between rows and images.
 * Refused with FEMASR_ERR_INVALID before any launch: a null pointer, B, H or W <= 0, filter outside 0..5, W > 2^22 (offsets and cost sums
 * inside a row are 32-bit), more than 2^31 - 1 rows in all. */
int femasr_png_filter_rgb8(void *stream, const uint8_t *img, int B, int H, int W, int filter, uint8_t *out);
/* The same for any 8-bit pixel size: img uint8 (B,H,W,C), C = 1 (gray, colour type 0), 2 (gray + alpha, 4), 3 (RGB, 2), 4 (RGBA, 6) -> out
 * uint8 (B,H,1 + C W); the left neighbour of byte i is byte i - C and n = C W (femasr_amd.pngio.filter_image).  C = 3 is the entry above, bit
 * for bit.  Refused as above, with C outside 1..4 and C W > 3 * 2^22 in place of the limit on W. */
int
femasr_png_filter_u8(void *stream, const uint8_t *img, int B, int H, int W, int C, int filter, uint8_t *out);

/* ---- gray, gray + alpha and RGBA images around the 3-channel network (opt-in, femasr_amd.channels) ----
 * split: img uint8 (B,H,W,C), C = 1, 2, 4 -> rgb uint8 (B,H,W,3) (gray replicated) and, for C = 2, 4, alpha uint8 (B,H,W) (the last channel);
 *   `alpha` is given exactly when C is 2 or 4.
 * merge: the final interleaved image out uint8 (s H, s W, channels) from rgb, the network's uint8 (s H, s W, 3) result, and ONE alpha source:
 *     alpha_lr   uint8 (H,W), the input's alpha plane: out's alpha is rint(clip(imresize(alpha_lr, s), 0, 255)), the bicubic evaluated inside
 *                the kernel in fp64 from w_h, idx_h (s H, taps_h) and w_w, idx_w (s W, taps_w), the DEVICE tables of the imresize entry for
 *                scale s without antialiasing: H pass, then W pass, one accumulator per output over its taps in ascending order from 0.0,
 *                no fma - the byte femasr_amd.channels.alpha_up_ref gives;
 *     alpha_rgb  uint8 (s H, s W, 3), the network's result for the alpha plane: out's alpha is its gray;
 *   gray = (19595 R + 38470 G + 7471 B + 32768) >> 16.  channels 1: gray(rgb), no alpha source; 2: gray(rgb), alpha; 4: rgb, alpha.
 *   channels 1 with rgb == NULL and alpha_lr: the bicubic alpha alone, (s H, s W).  The tables are read only with alpha_lr.
 * No buffer of a call may overlap another; none needs any alignment.  One launch each on `stream`; no workspace (no plane of the output's
 * size other than `out` exists), no atomics, no allocation, no synchronisation (capture-safe); 64-bit offsets between rows and images.
 * Refused with FEMASR_ERR_INVALID before any launch: a missing or surplus pointer, C / channels outside {1, 2, 4}, a count or size <= 0,
 * s H or s W reaching 2^31, more than 2^31 - 1 blocks of 1024 pixels. */
int femasr_channels_split_u8(void *stream, const uint8_t *img, int B, int H, int W, int C, uint8_t *rgb, uint8_t *alpha);
int femasr_channels_merge_u8(void *stream, const uint8_t *rgb, const uint8_t *alpha_lr, const uint8_t *alpha_rgb, int H, int W, int s,
                             int channels, const double *w_h, const int32_t *idx_h, int taps_h, const double *w_w, const int32_t *idx_w,
                             int taps_w, uint8_t *out);

/* Bicubic resample of an interleaved uint8 image (C = 1..4) to an arbitrary size, each axis at its own ratio (opt-in, femasr_amd.resample,
 * DESIGN.md 23): declared in femasr_hip_resample.h, which is part of this interface and is included here. */
#include "femasr_hip_resample.h"

/* Fast JPEG output (opt-in, femasr_amd.jpegio): colour, DCT and quantisation of a uint8 image in one launch, and the host-side
 * Huffman coder of its restart intervals: declared in femasr_hip_jpeg.h, which is part of this interface and is included here. */
#include "femasr_hip_jpeg.h"

/* Synthesis of low-quality inputs (opt-in, femasr_amd.degrade): blur, resample, noise and quantisation of a float32 image and
 * the decoder of the JPEG coefficient planes: declared in femasr_hip_degrade.h, which is part of this interface and is included here. */
#include "femasr_hip_degrade.h"

/* DISTS, the full-reference metric reported beside LPIPS (femasr_amd.dists): handle, forward and the pool / moments units:
 * declared in femasr_hip_dists.h, which is part of this interface and is included here. */
#include "femasr_hip_dists.h"

/* ---- measurement support ---- */
/* Sustained-clock probe: FEMASR_CLOCK_PROBE_BLOCKS blocks of 4 waves stream `mfmas_per_wave` back-to-back fp32 MFMAs (the load
 * of the hot kernels; 64 shader cycles each) and write the s_memtime ticks of their loop to ticks[blocks*4].  ticks / wall time
 * of the launch = the clock the chip sustains under MFMA load at that moment (bench.py reports it before and after the timed
 * region: the network's kernels are clock-bound, so a throttling box shows up here and not as a kernel regression). */
#define FEMASR_CLOCK_PROBE_BLOCKS 256
int femasr_clock_probe(void *stream, int mfmas_per_wave, unsigned long long *ticks);
int femasr_clock_probe_entries(void);      /* number of 64-bit entries femasr_clock_probe writes (size the buffer from this) */
/* Test / tuning hooks (process-global block-shape overrides, the per-handle Winograd size limit, the MFMA probe) are declared in
 * include/femasr_hip_debug.h: they are exported by the library but are not part of the drop-in interface. */
#ifdef __cplusplus
}
#endif
#endif /* FEMASR_HIP_H */

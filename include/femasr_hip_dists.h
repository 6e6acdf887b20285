/* femasr_hip_dists.h - DISTS (pyiqa 'dists'), the full-reference metric reported beside LPIPS (csrc/dists.hip).  Part of
 * the drop-in interface of libfemasr_hip.so: femasr_hip.h includes this file (inside its extern "C" block, behind the types it needs);
 * include that one.  Additive: femasr_version() stays 107.  Bound by femasr_amd/_lib.py as DISTS_SIGNATURES. */
#ifndef FEMASR_HIP_DISTS_H
#define FEMASR_HIP_DISTS_H

/* The handle holds the 13 VGG16 convs (repacked by femasr_repack_oihw) and the learned vectors alpha, beta.  Keys of set_weight:
 * stageK.I.weight (Cout,Cin,3,3) and stageK.I.bias (Cout) with I the torchvision `features` index (stage1: 0 2, stage2: 5 7, stage3: 10 12 14,
 * stage4: 17 19 21, stage5: 24 26 28), alpha and beta (1,1475,1,1); dev_ptr is float32 device memory.  create only records the device;
 * set_weight allocates on it.  finalize_weights names the first missing key with FEMASR_ERR_WEIGHT and sums w = sum(alpha) + sum(beta)
 * in fp64 in index order. */
typedef struct femasr_dists_handle femasr_dists_handle;
int femasr_dists_create(int device, femasr_dists_handle **out);
void femasr_dists_destroy(femasr_dists_handle *h);
int femasr_dists_set_weight(femasr_dists_handle *h, const char *key, const float *dev_ptr, const int64_t *shape, int ndim);
int femasr_dists_finalize_weights(femasr_dists_handle *h);

/* x, y: (B,3,H,W) fp32 NCHW RGB in [0,1].  scores[B]: 1 - sum_k sum_c (alpha S1 + beta S2) / w per pair, fp64.  terms (may be NULL):
 * [B][6][2], the sums over the channels of map k of alpha S1 and of beta S2, before the division by w.  `ws` >=
 * femasr_dists_workspace_bytes, 256-byte aligned.  Allocates nothing, synchronises nothing, every launch on `stream`: capture-safe.
 * Refused with FEMASR_ERR_INVALID before any launch: a null pointer, B, H or W < 1, H or W < 8, B > 65535, a feature tensor of 2B images
 * that reaches 2^31 elements (2 B H W 64), a misaligned or short workspace, weights that are not finalized.
 * femasr_dists_features runs the backbone only and writes the five stage maps, NHWC (2B,H_k,W_k,C_k) with x in images 0..B-1 and y in
 * B..2B-1, back to back into `features` (the maps femasr_dists_forward takes its moments of, for the tests). */
int femasr_dists_workspace_bytes(const femasr_dists_handle *h, int B, int H, int W, size_t *bytes);
int femasr_dists_forward(femasr_dists_handle *h, void *stream, const float *x_nchw, const float *y_nchw, int B, int H, int W, void *ws,
                         size_t ws_bytes, double *scores, double *terms);
int femasr_dists_features(femasr_dists_handle *h, void *stream, const float *x_nchw, const float *y_nchw, int B, int H, int W, void *ws,
                          size_t ws_bytes, float *features);

/* The units (the kernels the forward launches).
 * l2pool: f (B2,H,W,C) NHWC, C a multiple of 64 in 64..512 -> out (B2,ceil(H/2),ceil(W/2),C) = sqrtf(acc + 1e-12f), acc the fmaf chain
 *   of g[ky][kx] * (f * f) over ky, kx ascending with the padded taps skipped, g = (1 2 1)^T (1 2 1) / 16.
 * moments: f (2B,H,W,C) NHWC, pair b = images b and b + B -> sums [B][5][C] fp64: Sx, Sy, Sxx, Syy, Sxy over the H W pixels; the
 *   order of the additions depends on (H, W) alone.  moments_input: the same of x, y (B,3,H,W) NCHW -> sums [B][5][3].
 *   `ws` >= femasr_dists_moments_workspace_bytes(B, H, W, C) (C = 3: the input form), 256-byte aligned. */
int femasr_dists_l2pool(void *stream, const float *f, int B2, int H, int W, int C, float *out);
int femasr_dists_moments_workspace_bytes(int B, int H, int W, int C, size_t *bytes);
int femasr_dists_moments(void *stream, const float *f, int B, int H, int W, int C, void *ws, size_t ws_bytes, double *sums);
int femasr_dists_moments_input(void *stream, const float *x_nchw, const float *y_nchw, int B, int H, int W, void *ws, size_t ws_bytes,
                               double *sums);

#endif /* FEMASR_HIP_DISTS_H */

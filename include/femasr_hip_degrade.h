/* femasr_hip_degrade.h - synthesis of low-quality inputs (opt-in, femasr_amd.degrade): the operations of the BSRGAN
 * degradation chain on a float32 (H, W, 3) RGB image in [0, 1] on the device, and the decoder half of the JPEG round trip.  Part of the
 * drop-in interface of libfemasr_hip.so: femasr_hip.h includes this file (inside its extern "C" block, behind the types it needs); include
 * that one.  Additive: femasr_version() stays 107.  Bound by femasr_amd/_lib.py as DEGRADE_SIGNATURES.
 * Every entry is ONE launch on `stream`: no workspace, no atomics, no scratch, no allocation, no synchronisation (capture-safe); 64-bit
 * offsets.  Every refusal is FEMASR_ERR_INVALID before any launch: the outputs are not touched. */
#ifndef FEMASR_HIP_DEGRADE_H
#define FEMASR_HIP_DEGRADE_H

/* dst[Y][X][c] = sum_i sum_j kernel[i][j] src[m(Y stride + k/2 - i)][m(X stride + k/2 - j)][c] (femasr_amd.degrade.blur_ref): a true
 * convolution, m the reflection about the edge pixel centres (any image size, 1 x 1 included), one float32 accumulator per channel from 0, i
 * ascending outside and j inside, multiply and add rounded separately.  src (H, W, 3), kernel (k, k) and dst (ceil(H / stride),
 * ceil(W / stride), 3) are float32 on the device.  Refused: a null or misaligned pointer, H or W outside 1..2^24, k even or outside 3..25,
 * a stride other than 1, 2, 4, more than 65535 tiles of output rows. */
int femasr_degrade_blur_f32(void *stream, const float *src, int H, int W, const float *kernel, int k, int stride, float *dst);

/* Separable resample of src (H, W, 3) to dst (out_h, out_w, 3) from tap tables (femasr_amd.degrade.resize_ref): w_h / idx_h of
 * (out_h, taps_h) and w_w / idx_w of (out_w, taps_w) entries, float32 weights and int32 source indices, on the DEVICE.  H pass, then W
 * pass; every sum is one float32 accumulator from 0 over its taps in ascending order, multiply and add rounded separately; the result is
 * clipped to [0, 1].  idx_h_host / idx_w_host: the same two index tables in HOST memory - the kernel's tables live on the device, where
 * the entry cannot read them without a synchronisation, so it checks the caller's host copies (a few thousand integers) and refuses an
 * index outside the source; the kernel also clamps every index into the image, so that a device copy that differs cannot send an access
 * outside src.  Refused: a null or misaligned pointer, a size below 1, tap counts outside 1..4096, a source row of 2^31 floats (3 W) or
 * more, an index below 0 or at or above H (idx_h_host) / W (idx_w_host), tables too wide to stage one output pixel in 64 KiB of LDS. */
int femasr_degrade_resize_f32(void *stream, const float *src, int H, int W, float *dst, int out_h, int out_w, const float *w_h,
                              const int32_t *idx_h, int taps_h, const float *w_w, const int32_t *idx_w, int taps_w,
                              const int32_t *idx_h_host, const int32_t *idx_w_host);

/* Gaussian noise (femasr_amd.degrade.noise_ref): pixel p = pixel_offset + its index in src draws the standard normals 3p, 3p+1, 3p+2 of the
 * stream of `seed` (splitmix64 counters, Box-Muller in fp64).  mode 0 (colour): x_c + factor[0] n_c; 1 (gray): x_c + factor[0] n_0;
 * 2 (correlated): x_c + sum_k factor[3 c + k] n_k.  fp64, rounded to float32 once, clipped to [0, 1].  factor: 9 doubles in HOST memory.
 * src, dst: `pixels` x 3 float32 on the device; dst may be src.  The result depends on (seed, pixel index) alone, never on the launch.
 * Refused: a null or misaligned pointer, pixels outside 1..2^40, an offset above 2^60, another mode, a factor outside -16..16 or NaN. */
int femasr_degrade_noise_f32(void *stream, const float *src, float *dst, long long pixels, unsigned long long pixel_offset, int mode,
                             const double *factor, unsigned long long seed);

/* dst[i] = uint8(rint(clip(src[i], 0, 1) * 255.0f)), the product in float32, ties to even (single2uint of the reference).  n elements.
 * Refused: a null pointer, a misaligned src, n outside 1..2^42. */
int femasr_degrade_quantize_u8(void *stream, const float *src, uint8_t *dst, long long n);

/* dst[y][x][c] = (float)src[y][x][c] / 255.0f (uint2single of the reference; the divide is correctly rounded) for the top-left H x W pixels
 * of a uint8 RGB image whose rows are `pitch` pixels apart: a mod-crop needs no copy.  dst: float32 (H, W, 3), contiguous.
 * Refused: a null pointer, a misaligned dst, H or W below 1, pitch below W. */
int femasr_degrade_unit_f32(void *stream, const uint8_t *src, int H, int W, int pitch, float *dst);

/* The pixels of the coefficient planes femasr_jpeg_coefficients_u8 writes (femasr_amd.jpegio.decode_ref, integers only, bit for bit):
 * F = clip(k Q, -2047, 2047); column pass (sum_w T[w][y] F[w][u] + 512) >> 10, row pass (sum_u T[u][x] C[y][u] + 32768) >> 16, + 128,
 * clip; 4:2:0 chroma by the (9, 3, 3, 1) / 16 triangle with replicated edges, (sum + 8) >> 4; JFIF inverse colour in 16-bit fixed point
 * (91881, 22554, 46802, 116130; (v + 32768) >> 16); cropped to H x W.  y, cb, cr, C, subsampling, qtab_y, qtab_c: as for
 * femasr_jpeg_coefficients_u8 (only the 64 quantisers of a table are read).  out: (H, W, C) on the device - uint8, or with out_f32 = 1
 * float32 holding u8 / 255.  Refused: what femasr_jpeg_coefficients_u8 refuses, out_f32 other than 0 / 1, a misaligned float output. */
int femasr_jpeg_decode_u8(void *stream, const int16_t *y, const int16_t *cb, const int16_t *cr, int C, int subsampling, int H, int W,
                          const uint32_t *qtab_y, const uint32_t *qtab_c, void *out, int out_f32);

#endif /* FEMASR_HIP_DEGRADE_H */

/* femasr_hip_resample.h - bicubic resample of an interleaved uint8 image to an arbitrary size.  Part of the drop-in interface of
 * libfemasr_hip.so: femasr_hip.h includes this file (inside its extern "C" block, behind the types it needs); include that one.
 * Additive: femasr_version() stays 107.  Bound by femasr_amd/_lib.py as RESAMPLE_SIGNATURES. */
#ifndef FEMASR_HIP_RESAMPLE_H
#define FEMASR_HIP_RESAMPLE_H

/* MATLAB-style bicubic resample (csrc/resample.hip; the definition is femasr_amd.resample.resample_ref): src uint8 (H, W, C), C = 1..4
 * interleaved channels, -> dst uint8 (out_h, out_w, C).  Every channel on its own (alpha is a channel like any other); the H pass, then the
 * W pass, each output ONE fp64 accumulator over its taps in ascending order from 0.0 on float64(byte) samples, multiply and add rounded
 * separately; the byte is rint(clip(v, 0, 255)), ties to even.  The tables are the caller's: w_h / idx_h (out_h, taps_h) and
 * w_w / idx_w (out_w, taps_w), float64 weights and int32 0-based source rows / columns - femasr_model.imresize_tables(in, out, out / in);
 * the two axes are independent, any ratio that can be staged runs (1/8 .. 8 and far beyond with such tables; the Python layer draws the
 * line).  Indices are clamped to the image, so no table can send an access outside src.
 * ONE launch on `stream`: a block takes one output row and a tile of at most femasr_resample_tile() output columns, sized by the host so
 * that the tile's slice of the W tables and the H-pass sums of the source columns it taps fit 64 KiB of LDS.  No plane of the image in
 * floating point exists, no workspace, no atomics, no scratch, no allocation, no synchronisation (capture-safe); 64-bit offsets.
 * Refused with FEMASR_ERR_INVALID before any launch: C outside 1..4, a null pointer, a size or tap count < 1, W C or out_w reaching 2^31,
 * taps_w so large that not even one output column can be staged, more than 2^31 - 1 blocks. */
int femasr_resample_u8(void *stream, const uint8_t *src, int H, int W, int C, uint8_t *dst, int out_h, int out_w, const double *w_h,
                       const int32_t *idx_h, int taps_h, const double *w_w, const int32_t *idx_w, int taps_w);
/* Output columns per block at most (the tile of wide images at moderate ratios; tests stand on both sides of it). */
int femasr_resample_tile(void);

#endif /* FEMASR_HIP_RESAMPLE_H */

/* femasr_hip_jpeg.h - the two halves of the fast JPEG output (opt-in, femasr_amd.jpegio): colour, DCT and quantisation on the
 * GPU, baseline Huffman coding of restart intervals on the host.  Part of the drop-in interface of libfemasr_hip.so: femasr_hip.h includes this
 * file (inside its extern "C" block, behind the types it needs); include that one.  Additive: femasr_version() stays 107.  Bound by
 * femasr_amd/_lib.py as JPEG_SIGNATURES. */
#ifndef FEMASR_HIP_JPEG_H
#define FEMASR_HIP_JPEG_H

/* Quantised DCT coefficients of an image (csrc/jpeg_dct.hip; the definition is femasr_amd.jpegio.coefficients_ref, integers only, and the
 * result is that function's bit for bit).  img: uint8 (H, W, C) on the device, C = 1 (gray) or 3 (RGB), 1 <= H, W <= 65535, no alignment
 * asked.  subsampling: 444 or 420 for C = 3, ignored for C = 1.  JFIF full-range YCbCr in 16-bit fixed point; last column and row
 * replicated up to a whole MCU (8x8 pixels; 16x16 for 420); 420 chroma is the rounded mean of each 2x2 cell; 8x8 DCT with a 13-bit table,
 * row pass (sum + 512) >> 10, column pass (sum + 32768) >> 16; k = sign(F) ((|F| + (Q >> 1)) / Q).
 * qtab_y, qtab_c: DEVICE arrays of 128 uint32 each (femasr_amd.jpegio.device_tables): [k] the quantiser Q (1..255) of zigzag position k,
 * [64 + k] its reciprocal multiplier ceil(2^24 / Q); qtab_c is read only for C = 3.  The kernel trusts them.
 * out_y, out_cb, out_cr: int16 (Hb, Wb, 64) per component on the device, 16-byte aligned, block (by, bx) of the padded plane, zigzag order:
 *   C = 1: out_y of (ceil(H/8), ceil(W/8)) blocks, out_cb = out_cr = NULL;  444: three planes of that size;
 *   420: out_y of (2 ceil(H/16), 2 ceil(W/16)) blocks, out_cb and out_cr of (ceil(H/16), ceil(W/16)).
 * ONE launch on `stream`: a block takes one MCU row and a run of 256 pixel columns; every block of coefficients is written as one whole
 * 128-byte line.  No workspace, no atomics, no scratch, no allocation, no synchronisation (capture-safe); 64-bit offsets.
 * Refused with FEMASR_ERR_INVALID before any launch: C not 1 or 3, subsampling not 444 / 420 with C = 3, H or W outside 1..65535, a missing
 * or surplus pointer, an output plane that is not 16-byte aligned. */
int femasr_jpeg_coefficients_u8(const uint8_t *img, int H, int W, int C, int subsampling, const uint32_t *qtab_y, const uint32_t *qtab_c,
                                int16_t *out_y, int16_t *out_cb, int16_t *out_cr, void *stream);

/* Baseline Huffman coding (Annex K tables) of MCU rows row0 .. row1 - 1 of coefficient planes in HOST memory; host code, needs no GPU and
 * touches none.  y, cb, cr: the planes femasr_jpeg_coefficients_u8 writes (components = 1: cb = cr = NULL, subsampling ignored; components = 3:
 * subsampling 444 or 420), for an image of mcu_rows x mcus_per_row MCUs.  One restart interval per MCU row: DC predictors start at 0, the
 * interval is padded with 1-bits to a byte, 0xFF is followed by 0x00, and every row but row mcu_rows - 1 is followed by RSTm, m = row mod 8:
 * the bytes of femasr_amd.jpegio.entropy_ref, so that ranges coded by different threads concatenate to the scan.
 * Returns the number of bytes written to out (at most `capacity`), or a negative status (femasr_last_error() says why) - FEMASR_ERR_INVALID
 * for a bad argument, for a buffer that turns out too small (nothing is written past it) and for a coefficient outside baseline JPEG (a DC
 * difference beyond 11 bits, an AC value beyond 10).  Reentrant: any number of threads may code disjoint ranges at once. */
long long femasr_jpeg_entropy_rows(const int16_t *y, const int16_t *cb, const int16_t *cr, int components, int subsampling, int mcu_rows,
                                   int mcus_per_row, int row0, int row1, uint8_t *out, size_t capacity);
/* Bytes that `rows` MCU rows can need at most (every coefficient at its longest code, every byte stuffed, a marker per row); 0 for
 * arguments femasr_jpeg_entropy_rows would refuse. */
size_t femasr_jpeg_entropy_bound(int mcus_per_row, int components, int subsampling, int rows);

#endif /* FEMASR_HIP_JPEG_H */

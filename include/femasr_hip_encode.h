/* femasr_hip_encode.h - the network as an encoder and the code usage of its index maps.  Part of the drop-in interface of
 * libfemasr_hip.so: femasr_hip.h includes this file (inside its extern "C" block, behind the types it needs); include that one.
 * Additive: femasr_version() stays 107.  Bound by femasr_amd/_lib.py as ENCODE_SIGNATURES. */
#ifndef FEMASR_HIP_ENCODE_H
#define FEMASR_HIP_ENCODE_H

/* The network as an encoder: image -> VQ index maps, nothing else (the reference's two callers: the frozen HQ net that turns a GT batch
 * into gt_indices, basicsr/models/femasr_model.py:145-146, and vis_codebook.py:20-83).  femasr_forward's launch schedule, cut directly
 * behind the lookup of the LAST codebook scale: no after_quant conv of that scale, no decoder stage behind it, no out_conv, no crop, no
 * image.  Several codebooks: the decoder stages BETWEEN the lookups run as in femasr_forward.  Encoder features are computed and kept only
 * where something in front of the last lookup reads them (LQ nets: the up-blocks that only feed decoder skips are not launched).  Every
 * launch in front of a lookup is femasr_forward's, so the indices are its bits.
 * in: in_u8 = 0: fp32 NCHW (B,3,H,W); in_u8 = 1: uint8 HWC (B,H,W,3) through the fused pad kernel of femasr_forward_u8 (swap_rb = 1: BGR;
 * ignored for fp32).  `indices` (required): the layout of femasr_forward, all maps back to back; shapes from femasr_forward_shapes.
 * `ws`: 256-byte aligned, >= femasr_encode_workspace_bytes, which is exact (a smaller one is refused with FEMASR_ERR_WORKSPACE before any
 * launch) and not above femasr_workspace_bytes of the same arguments.  Sub-batch streams, profiling slots and capture safety (no host
 * synchronisation, no allocation) as femasr_forward. */
int femasr_encode_workspace_bytes(const femasr_handle *h, int B, int H, int W, int pad_mode, size_t *bytes);
int femasr_encode(femasr_handle *h, void *stream, const void *in, int in_u8, int swap_rb, int B, int H, int W, int pad_mode,
                  int64_t *indices, void *ws, size_t ws_bytes);

/* Code usage of index maps (csrc/codebook_stats.hip): indices int64 (G, M) - G groups (images, classes) of M tokens - ->
 * counts int64 (G, n_e) and invalid int64 (G): the number of indices outside [0, n_e), compared on all 64 bits (2^32 + 5 is invalid, not
 * code 5); counts[g].sum() + invalid[g] == M.  Per-block integer LDS counters, per-block partials in `ws`, a second launch that sums
 * them in a fixed order: exact, no global atomics, no memset - every element of counts and invalid is written.  n_e up to 2^20 (bins are
 * walked in chunks of 4096; the tokens are read once per chunk), G up to 65535.  Refused with FEMASR_ERR_INVALID before any launch:
 * G, M or n_e < 1, a larger n_e or G, a null pointer, a workspace below femasr_index_histogram_workspace_bytes.  Capture-safe. */
int femasr_index_histogram_workspace_bytes(int G, int64_t M, int n_e, size_t *bytes);
int femasr_index_histogram(void *stream, const int64_t *indices, int G, int64_t M, int n_e, int64_t *counts, int64_t *invalid,
                           void *ws, size_t ws_bytes);

#endif /* FEMASR_HIP_ENCODE_H */

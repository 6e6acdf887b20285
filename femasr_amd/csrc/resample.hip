// resample.hip — MATLAB-bicubic resample of an interleaved uint8 image to an arbitrary size (femasr_amd/resample.py) on gfx950:
// bytes in, bytes out, C = 1..4 channels, each axis with its own ratio (tables from imresize_tables(in, out, out / in)).
//
// Definition (resample.resample_ref; the loops of femasr_model.imresize on float64(byte) samples, every channel on its own):
//   H pass, then W pass; every output is ONE fp64 accumulator over its taps in ascending order from 0.0, multiply and add rounded separately
//   (the library is built with -ffp-contract=off); the byte is rint(fmin(fmax(v, 0), 255)) - half to even, as numpy's rint.
//
// One launch, the frame of channels_merge_kernel: a block owns ONE output row and a tile of at most RS_TILE output columns, a thread one
// pixel of it (all its channels).
//   1. the tile's slice of the W tables - `n * taps_w` consecutive entries of w_w / idx_w - goes to LDS in one coalesced sweep (the merge
//      kernel read them per thread from L2 and was bound by that: profiles/channels_bench.txt); rows are padded to an odd number of
//      entries so that the threads of a wave, one table row each, read different banks.  The sweep also finds the source columns the tile
//      taps (minimum and maximum index: wave shuffles, one LDS word per wave);
//   2. the H pass of output row Y for those columns: the window is `columns * C` consecutive bytes of every tapped source row, a thread
//      takes four of them at a time (one dword load, no alignment asked) and keeps four fp64 accumulators; the row's own table entries
//      are block-uniform.  The sums go to LDS as doubles - this is the only place the image exists in floating point;
//   3. the W pass from LDS, clip, round, and the C bytes of a pixel in one store where `dst` allows it (C = 2, 4).
// The host sizes the tile so that the table slice and the window fit RS_LDS_BYTES: the window grows with in / out and with the taps
// (34 at ratio 1/8).  Table indices are clamped to the image; a table entry outside the staged window (none in tables from
// imresize_tables) takes its H pass straight from memory, so no table can send an access outside `src`.
// No workspace, no atomics, no scratch, no allocation, no synchronisation: capture-safe, on the caller's stream.  Offsets are 64-bit.
#include "common.h"

#include <limits.h>

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_WAVES = RS_THREADS / 64;
constexpr int RS_TILE = RS_THREADS;                  // output pixels per block at most (femasr_resample_tile, resample.TILE)
constexpr size_t RS_LDS_BYTES = 64 * 1024;           // dynamic LDS a launch may ask for without raising the kernel's limit

// LDS of a block: w_w slice [tile][P1] and H-pass sums [cols][C] as doubles, then the idx_w slice [tile][P1] and the 2 RS_WAVES words of
// the index range as int32; P1 = taps_w | 1
__host__ __device__ inline size_t rs_lds_bytes(int tile, int taps_w, int cols, int C)
{
    const size_t ent = (size_t)tile * (size_t)(taps_w | 1);
    return 8 * (ent + (size_t)cols * C) + 4 * (ent + 2 * RS_WAVES);
}

// The H pass of output row Y for four consecutive bytes of the window (FULL) or its last `have` < 4 bytes: base points at them in source row
// 0, rows are `pitch` bytes apart; sums[i] is the definition's sum for byte i.  A dword load asks for no alignment here.
template <bool FULL>
__device__ __forceinline__ void rs_hgroup(const uint8_t *__restrict__ base, size_t pitch, int H, int have, const double *__restrict__ w_h,
                                          const int32_t *__restrict__ idx_h, int Ph, double *__restrict__ sums)
{
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll 4
    for (int k = 0; k < Ph; ++k) {
        const uint8_t *p = base + (size_t)clampi(idx_h[k], 0, H - 1) * pitch;      // (the clamp keeps a bad table in bounds)
        const double wk = w_h[k];
        uint32_t v = 0u;
        if (FULL) {
            __builtin_memcpy(&v, p, 4);
        } else {
            v = p[0];
            if (have > 1) v |= (uint32_t)p[1] << 8;
            if (have > 2) v |= (uint32_t)p[2] << 16;
        }
        a0 = a0 + wk * (double)(v & 255u);
        a1 = a1 + wk * (double)((v >> 8) & 255u);
        a2 = a2 + wk * (double)((v >> 16) & 255u);
        a3 = a3 + wk * (double)(v >> 24);
    }
    sums[0] = a0;
    if (FULL || have > 1) sums[1] = a1;
    if (FULL || have > 2) sums[2] = a2;
    if (FULL) sums[3] = a3;
}

// The H pass of output row Y at source column x, channel ch, straight from memory: the definition's sum over the row's taps
__device__ __forceinline__ double rs_hpass(const uint8_t *__restrict__ src, int H, int W, int C, int Y, int x, int ch,
                                           const double *__restrict__ w_h, const int32_t *__restrict__ idx_h, int Ph)
{
    double acc = 0.0;
    for (int k = 0; k < Ph; ++k) {
        const int j = clampi(idx_h[(size_t)Y * Ph + k], 0, H - 1);
        acc = acc + w_h[(size_t)Y * Ph + k] * (double)src[((size_t)j * W + x) * C + ch];
    }
    return acc;
}

// src (H,W,C) -> dst (out_h,out_w,C).  grid: tiles * out_h blocks, block -> (row Y, `tile` output columns from X0); cap: columns of LDS window
template <int C>
__global__ __launch_bounds__(RS_THREADS) void resample_u8_kernel(const uint8_t *__restrict__ src, int H, int W, uint8_t *__restrict__ dst,
                                                                  int out_w, const double *__restrict__ w_h,
                                                                  const int32_t *__restrict__ idx_h, int Ph, const double *__restrict__ w_w,
                                                                  const int32_t *__restrict__ idx_w, int Pw, int tile, int tiles, int cap)
{
    extern __shared__ double rs_lds[];
    const int P1 = Pw | 1;
    double *ww_s = rs_lds;
    double *col = ww_s + (size_t)tile * P1;
    int32_t *iw_s = reinterpret_cast<int32_t *>(col + (size_t)cap * C);
    int32_t *range = iw_s + (size_t)tile * P1;
    const int tid = (int)threadIdx.x;
    const int Y = (int)(blockIdx.x / (unsigned)tiles);
    const int X0 = (int)(blockIdx.x - (unsigned)Y * (unsigned)tiles) * tile;
    const int n = out_w - X0 < tile ? out_w - X0 : tile;

    // 1. the W tables of pixels X0 .. X0 + n - 1, and the source columns they tap
    int lo = INT_MAX, hi = -1;
    const size_t t0 = (size_t)X0 * Pw;
    for (int g = tid; g < n * Pw; g += RS_THREADS) {
        const int r = g / Pw, k = g - r * Pw;
        const int xi = clampi(idx_w[t0 + g], 0, W - 1);      // (tables from imresize_tables are in range; the clamp keeps a bad table in bounds)
        ww_s[r * P1 + k] = w_w[t0 + g];
        iw_s[r * P1 + k] = xi;
        lo = xi < lo ? xi : lo;
        hi = xi > hi ? xi : hi;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int l = __shfl_xor(lo, off), h = __shfl_xor(hi, off);
        lo = l < lo ? l : lo;
        hi = h > hi ? h : hi;
    }
    if ((tid & 63) == 0) {
        range[tid >> 6] = lo;
        range[RS_WAVES + (tid >> 6)] = hi;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < RS_WAVES; ++w) {
        lo = range[w] < lo ? range[w] : lo;
        hi = range[RS_WAVES + w] > hi ? range[RS_WAVES + w] : hi;
    }
    const int c0 = lo;
    const int nc = hi - lo + 1 < cap ? hi - lo + 1 : cap;

    // 2. the H pass of row Y for columns c0 .. c0 + nc - 1: nc * C consecutive bytes of every tapped row, four per thread and step
    const int E = nc * C;
    const uint8_t *win = src + (size_t)c0 * C;
    for (int e = 4 * tid; e < E; e += 4 * RS_THREADS) {
        if (E - e >= 4)
            rs_hgroup<true>(win + e, (size_t)W * C, H, 4, w_h + (size_t)Y * Ph, idx_h + (size_t)Y * Ph, Ph, col + e);
        else
            rs_hgroup<false>(win + e, (size_t)W * C, H, E - e, w_h + (size_t)Y * Ph, idx_h + (size_t)Y * Ph, Ph, col + e);
    }
    __syncthreads();

    // 3. the W pass of pixel X0 + tid
    if (tid >= n) return;
    const double *wr = ww_s + tid * P1;
    const int32_t *ir = iw_s + tid * P1;
    double acc[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) acc[ch] = 0.0;
    for (int k = 0; k < Pw; ++k) {
        const int xi = ir[k];
        const double wk = wr[k];
        if (xi - c0 < nc) {
#pragma unroll
            for (int ch = 0; ch < C; ++ch) acc[ch] = acc[ch] + wk * col[(xi - c0) * C + ch];
        } else {
#pragma unroll
            for (int ch = 0; ch < C; ++ch) acc[ch] = acc[ch] + wk * rs_hpass(src, H, W, C, Y, xi, ch, w_h, idx_h, Ph);
        }
    }
    uint32_t px = 0u;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) px |= (uint32_t)rint(fmin(fmax(acc[ch], 0.0), 255.0)) << (8 * ch);      // half to even, as numpy's rint
    uint8_t *d = dst + ((size_t)Y * (size_t)out_w + (size_t)(X0 + tid)) * C;
    if (C == 4 && ((uintptr_t)dst & 3u) == 0) {
        *reinterpret_cast<uint32_t *>(d) = px;
    } else if (C == 2 && ((uintptr_t)dst & 1u) == 0) {
        *reinterpret_cast<uint16_t *>(d) = (uint16_t)px;
    } else {
#pragma unroll
        for (int ch = 0; ch < C; ++ch) d[ch] = (uint8_t)(px >> (8 * ch));
    }
}

// source columns that `t` consecutive output pixels can tap: their first taps lie floor((t - 1) in / out) + 1 columns apart at most, every
// pixel has `taps` of them, and the reflection at the borders only folds indices back inside; + 2 for out / in rounded as a double
inline int rs_window(int t, int W, int out_w, int taps)
{
    const long long c = (long long)(t - 1) * W / out_w + 1 + taps + 2;
    return (int)(c < W ? c : W);
}

}  // namespace

extern "C" int femasr_resample_tile(void) { return RS_TILE; }

extern "C" int femasr_resample_u8(void *stream, const uint8_t *src, int H, int W, int C, uint8_t *dst, int out_h, int out_w, const double *w_h,
                                  const int32_t *idx_h, int taps_h, const double *w_w, const int32_t *idx_w, int taps_w)
{
    FEMASR_REQUIRE(C >= 1 && C <= 4, "resample_u8: C = %d is not in 1..4", C);
    FEMASR_REQUIRE(src && dst && w_h && idx_h && w_w && idx_w, "resample_u8: null argument");
    FEMASR_REQUIRE(H >= 1 && W >= 1 && out_h >= 1 && out_w >= 1, "resample_u8: empty shape: %dx%d -> %dx%d", H, W, out_h, out_w);
    FEMASR_REQUIRE(taps_h >= 1 && taps_w >= 1, "resample_u8: empty table: %d and %d taps", taps_h, taps_w);
    FEMASR_REQUIRE((long long)W * C <= INT_MAX && out_w <= INT_MAX - RS_TILE, "resample_u8: a row of %d or %d pixels reaches 2^31", W, out_w);
    int tile = out_w < RS_TILE ? out_w : RS_TILE;
    while (tile > 1 && rs_lds_bytes(tile, taps_w, rs_window(tile, W, out_w, taps_w), C) > RS_LDS_BYTES) --tile;
    const int cap = rs_window(tile, W, out_w, taps_w);
    const size_t lds = rs_lds_bytes(tile, taps_w, cap, C);
    FEMASR_REQUIRE(lds <= RS_LDS_BYTES && (long long)tile * taps_w <= INT_MAX / 2,
                   "resample_u8: %d taps per output column (width %d -> %d) cannot be staged in %zu bytes of LDS", taps_w, W, out_w, RS_LDS_BYTES);
    const int tiles = (out_w + tile - 1) / tile;
    FEMASR_REQUIRE((long long)tiles * out_h <= (1ll << 31) - 1, "resample_u8: %dx%d has more than 2^31 - 1 blocks of %d pixels", out_h, out_w, tile);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((long long)tiles * out_h)), block(RS_THREADS);
#define RS_LAUNCH(CH)                                                                                                                        \
    hipLaunchKernelGGL(resample_u8_kernel<CH>, grid, block, lds, st, src, H, W, dst, out_w, w_h, idx_h, taps_h, w_w, idx_w, taps_w, tile, \
                       tiles, cap)
    if (C == 1)
        RS_LAUNCH(1);
    else if (C == 2)
        RS_LAUNCH(2);
    else if (C == 3)
        RS_LAUNCH(3);
    else
        RS_LAUNCH(4);
#undef RS_LAUNCH
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

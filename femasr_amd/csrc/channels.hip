// channels.hip — takes a gray / gray+alpha / RGBA uint8 image apart in front of the network and puts the result together behind it
// (femasr_amd/channels.py) on gfx950.  The network only ever sees 3-channel images.
//
// Definitions (channels.split_ref, gray_ref, alpha_up_ref, merge_ref; integers, the bicubic in fp64):
//   split   (B,H,W,C), C = 1, 2, 4  ->  rgb (B,H,W,3) and, C = 2, 4, alpha (B,H,W): gray is replicated into R, G, B; the last channel is alpha
//   gray    (19595 R + 38470 G + 7471 B + 32768) >> 16
//   alpha   'bicubic': rint(clip(imresize(alpha, s), 0, 255)) of the LR alpha plane - H pass, then W pass, one fp64 accumulator per output
//           over its taps in ascending order from 0.0, multiply and add rounded separately (the library is built with -ffp-contract=off);
//           'network': gray of the network's RGB image of the alpha plane
//   merge   channels 1: gray(rgb); 2: gray(rgb), alpha; 4: rgb, alpha - interleaved, (sH,sW,channels)
//
// split: one launch, a thread owns four consecutive pixels of the flat pixel array: 4 C bytes in, 12 + 4 bytes out, as whole dwords where the
// three arrays start on a dword (whatever torch allocates does), byte by byte otherwise and for the last pixels.
// merge: one launch, a block owns CH_TILE consecutive pixels of ONE output row, a thread four of them: the canvas is read once (12 bytes) and
// the output written once (4 channels bytes, one store where the address allows it).  The bicubic alpha never exists as a plane: the block
// first evaluates the H pass of its row for the LR columns its pixels reach (at most CH_TILE / s + 8 fp64 values, in LDS), then every pixel
// runs its W pass over them - the very sums of the definition, so the byte is the definition's.  A table entry outside that window (there
// is none in tables from imresize_tables; indices are clamped to the plane besides) takes the H pass straight from memory instead.
// No workspace, no atomics, no scratch, no allocation, no synchronisation: capture-safe, on the caller's stream.  Offsets between rows and
// images are 64-bit.
#include "common.h"

namespace {

constexpr int CH_THREADS = 256;
constexpr int CH_PX = 4;                             // pixels per thread
constexpr int CH_TILE = CH_THREADS * CH_PX;          // pixels per block
constexpr int CH_COLS = CH_TILE + 8;                 // LR columns a block's pixels can reach: (CH_TILE - 1) / s + 1 + 3 in front + 3 behind, s >= 1

enum { CH_ALPHA_NONE = 0, CH_ALPHA_BICUBIC = 1, CH_ALPHA_NETWORK = 2 };

__device__ __forceinline__ bool ch_aligned(const void *p, unsigned a) { return ((uintptr_t)p & (uintptr_t)(a - 1u)) == 0; }
__device__ __forceinline__ uint32_t ch_gray(uint32_t r, uint32_t g, uint32_t b) { return (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16; }
// byte e of a little-endian dword array
template <int N>
__device__ __forceinline__ uint32_t ch_byte(const uint32_t (&w)[N], int e) { return (w[e >> 2] >> (8 * (e & 3))) & 255u; }

// NB bytes at p -> dwords; `whole`: all of them exist and p is on a dword, else the first `have` bytes are read one by one (the rest: 0)
template <int NB>
__device__ __forceinline__ void ch_load(const uint8_t *p, bool whole, int have, uint32_t (&w)[NB / 4])
{
    if (whole) {
#pragma unroll
        for (int m = 0; m < NB / 4; ++m) w[m] = reinterpret_cast<const uint32_t *>(p)[m];
    } else {
#pragma unroll
        for (int m = 0; m < NB / 4; ++m) w[m] = 0u;
#pragma unroll
        for (int e = 0; e < NB; ++e) {
            if (e < have) w[e >> 2] |= (uint32_t)p[e] << (8 * (e & 3));
        }
    }
}
// the counterpart; a whole store is one instruction where p is aligned to NB bytes (at most 16), dwords otherwise
template <int NB>
__device__ __forceinline__ void ch_store(uint8_t *p, bool whole, int have, const uint32_t (&w)[NB / 4])
{
    if (whole) {
        if constexpr (NB == 16) {
            if (ch_aligned(p, 16)) {
                *reinterpret_cast<uint4 *>(p) = make_uint4(w[0], w[1], w[2], w[3]);
                return;
            }
        } else if constexpr (NB == 8) {
            if (ch_aligned(p, 8)) {
                *reinterpret_cast<uint2 *>(p) = make_uint2(w[0], w[1]);
                return;
            }
        }
#pragma unroll
        for (int m = 0; m < NB / 4; ++m) reinterpret_cast<uint32_t *>(p)[m] = w[m];
    } else {
#pragma unroll
        for (int e = 0; e < NB; ++e) {
            if (e < have) p[e] = (uint8_t)ch_byte(w, e);
        }
    }
}

// img (npix, C) -> rgb (npix, 3), alpha (npix) for C = 2, 4
template <int C>
__global__ __launch_bounds__(CH_THREADS) void channels_split_kernel(const uint8_t *__restrict__ img, long long npix, uint8_t *__restrict__ rgb,
                                                                     uint8_t *__restrict__ alpha)
{
    const long long p0 = ((long long)blockIdx.x * CH_THREADS + threadIdx.x) * CH_PX;
    if (p0 >= npix) return;
    const int cnt = npix - p0 < CH_PX ? (int)(npix - p0) : CH_PX;
    const bool full = cnt == CH_PX;
    const uint8_t *src = img + (size_t)p0 * C;
    uint32_t in[C], c3[3] = {0u, 0u, 0u}, a1[1] = {0u};
    ch_load<4 * C>(src, full && ch_aligned(src, 4), cnt * C, in);
#pragma unroll
    for (int i = 0; i < CH_PX; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int e = 3 * i + k;
            c3[e >> 2] |= ch_byte(in, i * C + (C == 4 ? k : 0)) << (8 * (e & 3));
        }
        if (C != 1) a1[0] |= ch_byte(in, i * C + C - 1) << (8 * i);
    }
    uint8_t *d3 = rgb + (size_t)p0 * 3;
    ch_store<12>(d3, full && ch_aligned(d3, 4), 3 * cnt, c3);
    if (C != 1) {
        uint8_t *d1 = alpha + (size_t)p0;
        ch_store<4>(d1, full && ch_aligned(d1, 4), cnt, a1);
    }
}

// The H pass of output row Y at LR column x: the definition's sum over the row's taps
__device__ __forceinline__ double ch_hpass(const uint8_t *__restrict__ a, int H, int W, int Y, int x, const double *__restrict__ w_h,
                                           const int32_t *__restrict__ idx_h, int Ph)
{
    double acc = 0.0;
    for (int k = 0; k < Ph; ++k) {
        const int j = clampi(idx_h[(size_t)Y * Ph + k], 0, H - 1);      // (tables from imresize_tables are in range; the clamp keeps a bad table in bounds)
        acc = acc + w_h[(size_t)Y * Ph + k] * (double)a[(size_t)j * W + x];
    }
    return acc;
}

// rgb: (sH,sW,3) canvas (RGB: read at all).  MODE 1: alpha_lr (H,W) and the tables; MODE 2: alpha_rgb (sH,sW,3).  out: (sH,sW,CH).
// RGB = false (CH = 1, MODE 1): the alpha alone.  grid: tiles * sH blocks, block -> (row Y, tile of CH_TILE pixels)
template <int MODE, int CH, bool RGB>
__global__ __launch_bounds__(CH_THREADS) void channels_merge_kernel(const uint8_t *__restrict__ rgb, const uint8_t *__restrict__ alpha_lr,
                                                                     const uint8_t *__restrict__ alpha_rgb, int H, int W, int sW, int s,
                                                                     const double *__restrict__ w_h, const int32_t *__restrict__ idx_h, int Ph,
                                                                     const double *__restrict__ w_w, const int32_t *__restrict__ idx_w, int Pw,
                                                                     int tiles, uint8_t *__restrict__ out)
{
    __shared__ double col[MODE == CH_ALPHA_BICUBIC ? CH_COLS : 1];
    const int Y = (int)(blockIdx.x / (unsigned)tiles);
    const int X0 = (int)(blockIdx.x - (unsigned)Y * (unsigned)tiles) * CH_TILE;
    int c0 = 0, nc = 0;
    if (MODE == CH_ALPHA_BICUBIC) {
        const int xe = (X0 + CH_TILE < sW ? X0 + CH_TILE : sW) - 1;      // the block's last pixel
        c0 = X0 / s - 3 > 0 ? X0 / s - 3 : 0;
        const int c1 = xe / s + 4 < W ? xe / s + 4 : W;
        nc = c1 - c0 < CH_COLS ? c1 - c0 : CH_COLS;
        for (int c = (int)threadIdx.x; c < nc; c += CH_THREADS) col[c] = ch_hpass(alpha_lr, H, W, Y, c0 + c, w_h, idx_h, Ph);
        __syncthreads();
    }
    const int X = X0 + CH_PX * (int)threadIdx.x;
    if (X >= sW) return;
    const int cnt = sW - X < CH_PX ? sW - X : CH_PX;
    const bool full = cnt == CH_PX;
    const size_t pix = (size_t)Y * (size_t)sW + (size_t)X;
    uint32_t c3[3] = {0u, 0u, 0u}, a[CH_PX] = {0u, 0u, 0u, 0u};
    if (RGB) {
        const uint8_t *src = rgb + pix * 3;
        ch_load<12>(src, full && ch_aligned(src, 4), 3 * cnt, c3);
    }
    if (MODE == CH_ALPHA_BICUBIC) {
#pragma unroll
        for (int i = 0; i < CH_PX; ++i) {
            if (i < cnt) {
                const size_t t0 = (size_t)(X + i) * Pw;
                double acc = 0.0;
                for (int k = 0; k < Pw; ++k) {
                    const int xi = clampi(idx_w[t0 + k], 0, W - 1);
                    const double v = (xi >= c0 && xi < c0 + nc) ? col[xi - c0] : ch_hpass(alpha_lr, H, W, Y, xi, w_h, idx_h, Ph);
                    acc = acc + w_w[t0 + k] * v;
                }
                a[i] = (uint32_t)rint(fmin(fmax(acc, 0.0), 255.0));      // half to even, as numpy's rint
            }
        }
    } else if (MODE == CH_ALPHA_NETWORK) {
        const uint8_t *src = alpha_rgb + pix * 3;
        uint32_t n3[3];
        ch_load<12>(src, full && ch_aligned(src, 4), 3 * cnt, n3);
#pragma unroll
        for (int i = 0; i < CH_PX; ++i) a[i] = ch_gray(ch_byte(n3, 3 * i), ch_byte(n3, 3 * i + 1), ch_byte(n3, 3 * i + 2));
    }
    uint32_t o[CH];
#pragma unroll
    for (int m = 0; m < CH; ++m) o[m] = 0u;
#pragma unroll
    for (int i = 0; i < CH_PX; ++i) {
        const uint32_t r = ch_byte(c3, 3 * i), g = ch_byte(c3, 3 * i + 1), b = ch_byte(c3, 3 * i + 2);
        if constexpr (CH == 4) {
            o[i] = r | (g << 8) | (b << 16) | (a[i] << 24);
        } else if constexpr (CH == 2) {
            o[i >> 1] |= (ch_gray(r, g, b) | (a[i] << 8)) << (16 * (i & 1));
        } else {
            o[0] |= (RGB ? ch_gray(r, g, b) : a[i]) << (8 * i);
        }
    }
    uint8_t *dst = out + pix * CH;
    ch_store<4 * CH>(dst, full && ch_aligned(dst, 4), CH * cnt, o);
}

}  // namespace

extern "C" int femasr_channels_split_u8(void *stream, const uint8_t *img, int B, int H, int W, int C, uint8_t *rgb, uint8_t *alpha)
{
    FEMASR_REQUIRE(C == 1 || C == 2 || C == 4, "channels_split_u8: C = %d is not 1 (gray), 2 (gray + alpha) or 4 (RGBA)", C);
    FEMASR_REQUIRE(img && rgb && (alpha != nullptr) == (C != 1), "channels_split_u8: null argument (alpha is given exactly when C is 2 or 4)");
    FEMASR_REQUIRE(B >= 1 && H >= 1 && W >= 1, "channels_split_u8: empty shape: %d images of %dx%d", B, H, W);
    const long long npix = (long long)B * H * W;
    const long long blocks = (npix + CH_TILE - 1) / CH_TILE;
    FEMASR_REQUIRE(blocks <= (1ll << 31) - 1, "channels_split_u8: %d images of %dx%d are more than 2^31 - 1 blocks of %d pixels", B, H, W, CH_TILE);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)blocks), block(CH_THREADS);
    if (C == 1)
        hipLaunchKernelGGL(channels_split_kernel<1>, grid, block, 0, st, img, npix, rgb, alpha);
    else if (C == 2)
        hipLaunchKernelGGL(channels_split_kernel<2>, grid, block, 0, st, img, npix, rgb, alpha);
    else
        hipLaunchKernelGGL(channels_split_kernel<4>, grid, block, 0, st, img, npix, rgb, alpha);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

extern "C" int femasr_channels_merge_u8(void *stream, const uint8_t *rgb, const uint8_t *alpha_lr, const uint8_t *alpha_rgb, int H, int W, int s,
                                        int channels, const double *w_h, const int32_t *idx_h, int taps_h, const double *w_w,
                                        const int32_t *idx_w, int taps_w, uint8_t *out)
{
    FEMASR_REQUIRE(channels == 1 || channels == 2 || channels == 4, "channels_merge_u8: channels = %d is not 1, 2 or 4", channels);
    FEMASR_REQUIRE(out, "channels_merge_u8: null argument");
    FEMASR_REQUIRE(!(alpha_lr && alpha_rgb), "channels_merge_u8: two alpha sources (the LR plane and the network's image)");
    const int mode = alpha_lr ? CH_ALPHA_BICUBIC : (alpha_rgb ? CH_ALPHA_NETWORK : CH_ALPHA_NONE);
    if (channels == 1)
        FEMASR_REQUIRE(rgb ? mode == CH_ALPHA_NONE : mode == CH_ALPHA_BICUBIC,
                       "channels_merge_u8: channels = 1 is the gray of rgb (no alpha source) or, without rgb, the bicubic alpha alone");
    else
        FEMASR_REQUIRE(rgb && mode != CH_ALPHA_NONE, "channels_merge_u8: channels = %d needs rgb and one alpha source", channels);
    FEMASR_REQUIRE(H >= 1 && W >= 1 && s >= 1, "channels_merge_u8: empty shape: %dx%d at scale %d", H, W, s);
    FEMASR_REQUIRE((long long)s * H <= (1ll << 31) - 1 && (long long)s * W <= (1ll << 31) - 1 - CH_TILE,
                   "channels_merge_u8: %dx%d at scale %d reaches 2^31 in a dimension", H, W, s);
    if (mode == CH_ALPHA_BICUBIC)
        FEMASR_REQUIRE(w_h && idx_h && w_w && idx_w && taps_h >= 1 && taps_w >= 1, "channels_merge_u8: the bicubic alpha needs both tables");
    const int sH = s * H, sW = s * W;
    const int tiles = (sW + CH_TILE - 1) / CH_TILE;
    FEMASR_REQUIRE((long long)tiles * sH <= (1ll << 31) - 1, "channels_merge_u8: %dx%d has more than 2^31 - 1 blocks of %d pixels", sH, sW, CH_TILE);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((long long)tiles * sH)), block(CH_THREADS);
#define CH_LAUNCH(MODE, CH, RGB)                                                                                                              \
    hipLaunchKernelGGL((channels_merge_kernel<MODE, CH, RGB>), grid, block, 0, st, rgb, alpha_lr, alpha_rgb, H, W, sW, s, w_h, idx_h, taps_h, \
                       w_w, idx_w, taps_w, tiles, out)
    if (channels == 1 && rgb)
        CH_LAUNCH(CH_ALPHA_NONE, 1, true);
    else if (channels == 1)
        CH_LAUNCH(CH_ALPHA_BICUBIC, 1, false);
    else if (channels == 2 && mode == CH_ALPHA_BICUBIC)
        CH_LAUNCH(CH_ALPHA_BICUBIC, 2, true);
    else if (channels == 2)
        CH_LAUNCH(CH_ALPHA_NETWORK, 2, true);
    else if (mode == CH_ALPHA_BICUBIC)
        CH_LAUNCH(CH_ALPHA_BICUBIC, 4, true);
    else
        CH_LAUNCH(CH_ALPHA_NETWORK, 4, true);
#undef CH_LAUNCH
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

// degrade.hip — synthesis of low-quality inputs on gfx950 (femasr_amd/degrade.py): the operations of the BSRGAN degradation
// chain on a float32 (H,W,3) RGB image in [0,1], and the decoder half of the JPEG round trip (femasr_amd/jpegio.py decode_ref).
//   femasr_degrade_blur_f32      dense k x k convolution, mirror border, optional output stride
//   femasr_degrade_resize_f32    separable resample from host-built tap tables, clipped to [0,1]
//   femasr_degrade_noise_f32     counter-based Gaussian noise (splitmix64, Box-Muller in fp64) through a 3x3 factor, clipped
//   femasr_degrade_quantize_u8   single2uint: clip, x255, round half to even;  femasr_degrade_unit_f32: uint2single, u8 / 255
//   femasr_jpeg_decode_u8        the int16 planes of femasr_jpeg_coefficients_u8 back to pixels: dequantise, IDCT, 4:2:0 upsample, colour
// Every entry is ONE launch on the caller's stream: no workspace, no atomics, no scratch, no allocation, no synchronisation (capture-safe);
// offsets into the images are 64-bit.  The library is built with -ffp-contract=off: every multiply and every add below rounds on its own,
// which is what the numpy restatements of tests/degrade_ref.py model.
#include "common.h"

#include <limits.h>

namespace {

constexpr int DG_THREADS = 256;
constexpr size_t DG_LDS_BYTES = 64 * 1024;           // LDS a launch may ask for without raising the kernel's limit

// ---------------------------------------------------------------------------------------------------------------- blur
// Reflection about the edge pixel centres (d c b | a b c d | c b a), period 2 (n - 1); valid for every i and every n >= 1
__device__ __forceinline__ int dg_mirror(int i, int n)
{
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int t = i % p;
    if (t < 0) t += p;
    return t < n ? t : p - t;
}

// out[Y][X][c] = sum_i sum_j k[i][j] * img[m(Y s + r - i)][m(X s + r - j)][c], r = K / 2 (true convolution: the kernel is flipped), one
// float32 accumulator per channel from 0.0f, i ascending outside, j ascending inside, multiply and add rounded separately.
// A block owns a tile of tx x ty kept pixels (tx ty <= 256, a thread one pixel) and stages the (ty - 1) s + K rows by (tx - 1) s + K columns
// of the interleaved image it taps, mirror index applied on the load.  The weights are indexed by the loop counters alone: scalar loads.
// A thread's reads of the staged image are 3 s floats from its neighbour's: conflict-free at s = 1, 2-way at s = 2, 4-way at s = 4.
__global__ __launch_bounds__(DG_THREADS) void degrade_blur_kernel(const float *__restrict__ src, int H, int W, const float *__restrict__ kern, int K,
                                                                   int s, float *__restrict__ dst, int out_h, int out_w, int tx, int ty)
{
    extern __shared__ float dg_tile[];
    const int tid = (int)threadIdx.x;
    const int X0 = (int)blockIdx.x * tx, Y0 = (int)blockIdx.y * ty;
    const int fw = (tx - 1) * s + K, fh = (ty - 1) * s + K;
    const int r = K / 2;
    const int ox = X0 * s - r, oy = Y0 * s - r;
    for (int e = tid; e < fh * fw; e += DG_THREADS) {
        const int fy = e / fw, fx = e - fy * fw;
        const float *p = src + ((size_t)dg_mirror(oy + fy, H) * (size_t)W + (size_t)dg_mirror(ox + fx, W)) * 3;
        dg_tile[3 * e] = p[0], dg_tile[3 * e + 1] = p[1], dg_tile[3 * e + 2] = p[2];
    }
    __syncthreads();
    const int lx = tid % tx, ly = tid / tx;
    const int X = X0 + lx, Y = Y0 + ly;
    if (ly >= ty || X >= out_w || Y >= out_h) return;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
    for (int i = 0; i < K; ++i) {
        const float *row = dg_tile + ((ly * s + (K - 1 - i)) * fw + lx * s + (K - 1)) * 3;
        for (int j = 0; j < K; ++j) {
            const float w = kern[i * K + j];
            const float *v = row - 3 * j;
            a0 = a0 + w * v[0];
            a1 = a1 + w * v[1];
            a2 = a2 + w * v[2];
        }
    }
    float *d = dst + ((size_t)Y * (size_t)out_w + (size_t)X) * 3;
    d[0] = a0, d[1] = a1, d[2] = a2;
}

// ---------------------------------------------------------------------------------------------------------------- resize
constexpr int DR_TILE = DG_THREADS;                  // output pixels per block at most
constexpr int DR_WAVES = DG_THREADS / 64;

// LDS of a block: the w_w slice [tile][P1] and the H-pass sums [cols][3] as floats, the idx_w slice [tile][P1] and the 2 DR_WAVES words of
// the index range as int32; P1 = taps_w | 1
__host__ __device__ inline size_t dr_lds_bytes(int tile, int taps_w, int cols)
{
    const size_t ent = (size_t)tile * (size_t)(taps_w | 1);
    return 4 * (ent + (size_t)cols * 3) + 4 * (ent + 2 * DR_WAVES);
}

// source columns that `t` consecutive output pixels can tap (the rule of resample.hip: first taps floor((t - 1) in / out) + 1 apart at
// most, `taps` each, + 2 for rounding); a table that taps outside this window is still served, from memory (dr_hpass)
inline int dr_window(int t, int W, int out_w, int taps)
{
    const long long c = (long long)(t - 1) * W / out_w + 1 + taps + 2;
    return (int)(c < W ? c : W);
}

// The H pass of output row Y at source column x, channel ch: one float32 accumulator from 0.0f over the row's taps in ascending order
__device__ __forceinline__ float dr_hpass(const float *__restrict__ src, int H, int W, int x, int ch, const float *__restrict__ w_h,
                                          const int32_t *__restrict__ idx_h, int Ph)
{
    float acc = 0.0f;
    for (int k = 0; k < Ph; ++k) acc = acc + w_h[k] * src[((size_t)clampi(idx_h[k], 0, H - 1) * W + x) * 3 + ch];
    return acc;
}

// src (H,W,3) -> dst (out_h,out_w,3), the frame of resample_u8_kernel: a block owns ONE output row and `tile` output columns.  1. its slice
// of the W tables goes to LDS and yields the source columns it taps; 2. the H pass of those columns (3 consecutive floats each) to LDS;
// 3. the W pass from LDS, clip to [0,1], store.  The entry refuses host copies of the tables that index outside the image; the kernel
// clamps the device tables as well, so no table can send an access outside `src`.
__global__ __launch_bounds__(DG_THREADS) void degrade_resize_kernel(const float *__restrict__ src, int H, int W, float *__restrict__ dst, int out_w,
                                                                     const float *__restrict__ w_h, const int32_t *__restrict__ idx_h, int Ph,
                                                                     const float *__restrict__ w_w, const int32_t *__restrict__ idx_w, int Pw,
                                                                     int tile, int tiles, int cap)
{
    extern __shared__ float dr_lds[];
    const int P1 = Pw | 1;
    float *ww_s = dr_lds;
    float *col = ww_s + (size_t)tile * P1;
    int32_t *iw_s = reinterpret_cast<int32_t *>(col + (size_t)cap * 3);
    int32_t *range = iw_s + (size_t)tile * P1;
    const int tid = (int)threadIdx.x;
    const int Y = (int)(blockIdx.x / (unsigned)tiles);
    const int X0 = (int)(blockIdx.x - (unsigned)Y * (unsigned)tiles) * tile;
    const int n = out_w - X0 < tile ? out_w - X0 : tile;

    int lo = INT_MAX, hi = -1;
    const size_t t0 = (size_t)X0 * Pw;
    for (int g = tid; g < n * Pw; g += DG_THREADS) {
        const int r = g / Pw, k = g - r * Pw;
        const int xi = clampi(idx_w[t0 + g], 0, W - 1);
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
        range[DR_WAVES + (tid >> 6)] = hi;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < DR_WAVES; ++w) {
        lo = range[w] < lo ? range[w] : lo;
        hi = range[DR_WAVES + w] > hi ? range[DR_WAVES + w] : hi;
    }
    const int c0 = lo;
    const int nc = hi - lo + 1 < cap ? hi - lo + 1 : cap;

    const float *wh = w_h + (size_t)Y * Ph;
    const int32_t *ih = idx_h + (size_t)Y * Ph;
    const int E = nc * 3;
    for (int e = tid; e < E; e += DG_THREADS) {
        float acc = 0.0f;
        for (int k = 0; k < Ph; ++k) acc = acc + wh[k] * src[((size_t)clampi(ih[k], 0, H - 1) * W + c0) * 3 + e];
        col[e] = acc;
    }
    __syncthreads();

    if (tid >= n) return;
    const float *wr = ww_s + tid * P1;
    const int32_t *ir = iw_s + tid * P1;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int k = 0; k < Pw; ++k) {
        const int xi = ir[k];
        const float wk = wr[k];
        if (xi - c0 < nc) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) acc[ch] = acc[ch] + wk * col[(xi - c0) * 3 + ch];
        } else {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) acc[ch] = acc[ch] + wk * dr_hpass(src, H, W, xi, ch, wh, ih, Ph);
        }
    }
    float *d = dst + ((size_t)Y * (size_t)out_w + (size_t)(X0 + tid)) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) d[ch] = fminf(fmaxf(acc[ch], 0.0f), 1.0f);
}

// ---------------------------------------------------------------------------------------------------------------- noise
__device__ __forceinline__ uint64_t dn_splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// Standard normal number j of the stream `base` (degrade.normal_ref): u1 = ((h(base + 2j) >> 11) + 1) 2^-53 in (0,1],
// u2 = (h(base + 2j + 1) >> 11) 2^-53 in [0,1), n = sqrt(-2 log u1) cos(2 pi u2), all fp64
__device__ __forceinline__ double dn_normal(uint64_t base, uint64_t j)
{
    const double u1 = (double)((dn_splitmix64(base + 2ull * j) >> 11) + 1ull) * 0x1p-53;
    const double u2 = (double)(dn_splitmix64(base + 2ull * j + 1ull) >> 11) * 0x1p-53;
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

struct dn_factor {
    double a[9];
};

// pixel p (global index offset + local index) draws normals 3p, 3p + 1, 3p + 2.  mode 0 (colour): x_c + a[0] n_c; 1 (gray): x_c + a[0] n_0;
// 2 (correlated): ((x_c + a[3c] n_0) + a[3c+1] n_1) + a[3c+2] n_2.  fp64, rounded to float32 once, then clipped to [0,1].  src may be dst.
__global__ __launch_bounds__(DG_THREADS) void degrade_noise_kernel(const float *src, float *dst, size_t pixels, uint64_t offset, int mode, dn_factor f,
                                                                    uint64_t base)
{
    for (size_t p = (size_t)blockIdx.x * DG_THREADS + threadIdx.x; p < pixels; p += (size_t)gridDim.x * DG_THREADS) {
        const uint64_t j = 3ull * (offset + (uint64_t)p);
        const double x0 = (double)src[3 * p], x1 = (double)src[3 * p + 1], x2 = (double)src[3 * p + 2];
        const double n0 = dn_normal(base, j);
        double v0, v1, v2;
        if (mode == 1) {
            v0 = x0 + f.a[0] * n0, v1 = x1 + f.a[0] * n0, v2 = x2 + f.a[0] * n0;
        } else {
            const double n1 = dn_normal(base, j + 1), n2 = dn_normal(base, j + 2);
            if (mode == 0) {
                v0 = x0 + f.a[0] * n0, v1 = x1 + f.a[0] * n1, v2 = x2 + f.a[0] * n2;
            } else {
                v0 = ((x0 + f.a[0] * n0) + f.a[1] * n1) + f.a[2] * n2;
                v1 = ((x1 + f.a[3] * n0) + f.a[4] * n1) + f.a[5] * n2;
                v2 = ((x2 + f.a[6] * n0) + f.a[7] * n1) + f.a[8] * n2;
            }
        }
        dst[3 * p] = fminf(fmaxf((float)v0, 0.0f), 1.0f);
        dst[3 * p + 1] = fminf(fmaxf((float)v1, 0.0f), 1.0f);
        dst[3 * p + 2] = fminf(fmaxf((float)v2, 0.0f), 1.0f);
    }
}

// ---------------------------------------------------------------------------------------------------------------- quantise
// uint8(rint(clip(x, 0, 1) * 255.0f)): the product in float32, ties to even
__global__ __launch_bounds__(DG_THREADS) void degrade_quantize_kernel(const float *__restrict__ src, uint8_t *__restrict__ dst, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * DG_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * DG_THREADS)
        dst[i] = (uint8_t)__float2int_rn(fminf(fmaxf(src[i], 0.0f), 1.0f) * 255.0f);
}

// uint2single: (float)u8 / 255.0f (the correctly rounded divide) of the top-left H x W pixels of an image whose rows are `pitch` pixels apart
__global__ __launch_bounds__(DG_THREADS) void degrade_unit_kernel(const uint8_t *__restrict__ src, int W, size_t pitch, float *__restrict__ dst, size_t n)
{
    const size_t row = (size_t)W * 3;
    for (size_t i = (size_t)blockIdx.x * DG_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * DG_THREADS) {
        const size_t y = i / row;
        dst[i] = (float)src[y * pitch * 3 + (i - y * row)] / 255.0f;
    }
}

// ---------------------------------------------------------------------------------------------------------------- JPEG decode
// Definition (jpegio.decode_ref; integers only, >> is the arithmetic shift).  Per 8x8 block of a plane, k its coefficients:
//   F[w][u] = clip(k Q, -2047, 2047)                          (zigzag position of 8 w + u; what the encoder writes stays below 1154)
//   C[y][u] = (sum_w T[w][y] F[w][u] + 512) >> 10             |sum| <= 21641 * 2047 < 2^26, |C| <= 43261
//   p[y][x] = clip(((sum_u T[u][x] C[y][u] + 32768) >> 16) + 128, 0, 255)          |sum| <= 21641 * 43261 < 2^30
//   4:2:0 chroma at pixel (y, x): (9 c[i][j] + 3 c[i'][j] + 3 c[i][j'] + c[i'][j'] + 8) >> 4, i = y >> 1, i' = i - 1 (y even) / i + 1 (y odd)
//   clamped to the padded chroma plane, j likewise;  R = clip(Y + ((91881 cr + 32768) >> 16)), G = clip(Y + ((-22554 cb - 46802 cr + 32768) >> 16)),
//   B = clip(Y + ((116130 cb + 32768) >> 16)) with cb = Cb - 128, cr = Cr - 128; cropped to H x W.
// The kernel.  A block of 256 threads takes one MCU row and a strip of 128 pixel columns.  Per plane it needs a REGION of plane pixels: the
// strip itself, for 4:2:0 chroma the strip's half-size rectangle and one pixel around it (the triangle filter's neighbours).
//   1. the coefficient blocks that cover the regions go to LDS as whole 128-byte lines (16 bytes a lane);
//   2. column pass: a lane takes column u of a block, dequantises its eight coefficients through the zigzag table and writes C (int32; the
//      72-word block pitch puts the four blocks of a 32-lane half on different banks) - only the rows y inside the region: ONE of the
//      eight of a neighbouring chroma block row, whose pixels another block decodes in full (one launch without a workspace cannot fetch them);
//   3. row pass of the same rows: eight pixels to a byte plane in LDS;
//   4. a thread per pixel: chroma upsample from the byte planes, colour, store (uint8, or float32 u8 / 255 with the correctly rounded divide).
constexpr int JD_STRIP = 128;
constexpr int JD_MAX_BLOCKS = 92;                    // 4:2:0: 2 x 16 Y blocks, 3 x 10 per chroma plane; 4:4:4: 3 x 16
constexpr int JD_C_PITCH = 72;
constexpr int JD_PIX_ROWS = 16, JD_PIX_PITCH = 136;  // Y of 4:2:0: 16 rows x 128; chroma of 4:2:0: 10 rows x 80

__device__ constexpr int JD_T[8][8] = {{2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},     {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},
                                       {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784}, {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},
                                       {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896}, {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
                                       {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567}, {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};
// zigzag position of natural index 8 w + u
__constant__ uint8_t JD_ZZ_OF_NAT[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                         10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

struct jd_args {
    const int16_t *coef[3];
    int hb[3], wb[3];        // blocks of each plane
    const uint32_t *qtab[2];
    int H, W;
    void *out;
};

template <int C, bool SUB, bool F32>
__global__ __launch_bounds__(DG_THREADS) void jpeg_decode_kernel(jd_args a)
{
    constexpr int M = SUB ? 16 : 8;
    __shared__ uint4 cz16[JD_MAX_BLOCKS * 8];                       // coefficients, zigzag order, 64 int16 a block
    __shared__ int32_t cs[JD_MAX_BLOCKS * JD_C_PITCH];              // C[y][u] at [block][8 y + u]
    __shared__ uint32_t pix32[C * JD_PIX_ROWS * JD_PIX_PITCH / 4];
    __shared__ uint32_t qt[2][64];
    const int16_t *cz = reinterpret_cast<const int16_t *>(cz16);
    uint8_t *pix = reinterpret_cast<uint8_t *>(pix32);
    const int tid = (int)threadIdx.x;
    const int x0 = (int)blockIdx.x * JD_STRIP, y0 = (int)blockIdx.y * M;

    // the regions and the blocks that cover them
    int ry0[C], ry1[C], bx0[C], by0[C], nbx[C], cnt[C];
    int total = 0;
#pragma unroll
    for (int p = 0; p < C; ++p) {
        const int f = (SUB && p > 0) ? 2 : 1, h = f - 1;
        ry0[p] = max(y0 / f - h, 0);
        ry1[p] = min((y0 + M) / f + h, 8 * a.hb[p]);
        const int rx0 = max(x0 / f - h, 0), rx1 = min((x0 + JD_STRIP) / f + h, 8 * a.wb[p]);
        by0[p] = ry0[p] >> 3, bx0[p] = rx0 >> 3;
        nbx[p] = ((rx1 - 1) >> 3) - bx0[p] + 1;
        cnt[p] = (((ry1[p] - 1) >> 3) - by0[p] + 1) * nbx[p];
        total += cnt[p];
    }
    // block b of the list: its plane, block row and block column
    auto locate = [&](int b, int &p, int &by, int &bx) {
        p = 0;
        if (C == 3 && b >= cnt[0]) {
            b -= cnt[0], p = 1;
            if (b >= cnt[1]) b -= cnt[1], p = 2;
        }
        const int n = C == 3 ? (p == 0 ? nbx[0] : (p == 1 ? nbx[1] : nbx[C - 1])) : nbx[0];
        const int r = b / n;
        by = (C == 3 ? (p == 0 ? by0[0] : (p == 1 ? by0[1] : by0[C - 1])) : by0[0]) + r;
        bx = (C == 3 ? (p == 0 ? bx0[0] : (p == 1 ? bx0[1] : bx0[C - 1])) : bx0[0]) + (b - r * n);
    };

    if (tid < 64) qt[0][tid] = a.qtab[0][tid];
    else if (C == 3 && tid < 128) qt[1][tid - 64] = a.qtab[1][tid - 64];

    // 1. whole 128-byte lines
    for (int i = tid; i < total * 8; i += DG_THREADS) {
        int p, by, bx;
        locate(i >> 3, p, by, bx);
        cz16[i] = *reinterpret_cast<const uint4 *>(a.coef[p] + ((size_t)by * (size_t)a.wb[p] + (size_t)bx) * 64 + (size_t)(i & 7) * 8);
    }
    __syncthreads();

    // rows of plane p inside its region
    auto rows_of = [&](int p, int &lo, int &hi) {
        lo = C == 3 ? (p == 0 ? ry0[0] : (p == 1 ? ry0[1] : ry0[C - 1])) : ry0[0];
        hi = C == 3 ? (p == 0 ? ry1[0] : (p == 1 ? ry1[1] : ry1[C - 1])) : ry1[0];
    };

    // 2. dequantisation and column pass, only for the rows y of a block inside the region (step 3 reads no other): of a neighbouring chroma
    //    block row that is one y of eight
    for (int i = tid; i < total * 8; i += DG_THREADS) {
        const int b = i >> 3, u = i & 7;
        int p, by, bx, lo, hi;
        locate(b, p, by, bx);
        rows_of(p, lo, hi);
        const uint32_t *q = qt[p > 0 ? 1 : 0];
        int F[8];
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            const int z = JD_ZZ_OF_NAT[8 * w + u];
            F[w] = clampi((int)cz[b * 64 + z] * (int)q[z], -2047, 2047);
        }
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            if (8 * by + y < lo || 8 * by + y >= hi) continue;
            int acc = 512;
#pragma unroll
            for (int w = 0; w < 8; ++w) acc += JD_T[w][y] * F[w];
            cs[b * JD_C_PITCH + 8 * y + u] = acc >> 10;
        }
    }
    __syncthreads();

    // 3. row pass of the rows inside the region
    for (int i = tid; i < total * 8; i += DG_THREADS) {
        const int b = i >> 3, y = i & 7;
        int p, by, bx, lo, hi;
        locate(b, p, by, bx);
        rows_of(p, lo, hi);
        const int row = 8 * by + y;
        if (row < lo || row >= hi) continue;
        const int cb0 = C == 3 ? (p == 0 ? bx0[0] : (p == 1 ? bx0[1] : bx0[C - 1])) : bx0[0];
        const int32_t *c = cs + b * JD_C_PITCH + 8 * y;
        uint32_t o[2] = {0u, 0u};
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            int acc = 32768;
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += JD_T[u][x] * c[u];
            o[x >> 2] |= (uint32_t)clampi((acc >> 16) + 128, 0, 255) << (8 * (x & 3));
        }
        uint32_t *d = pix32 + ((p * JD_PIX_ROWS + (row - lo)) * JD_PIX_PITCH + 8 * (bx - cb0)) / 4;
        d[0] = o[0], d[1] = o[1];
    }
    __syncthreads();

    // 4. pixels
    for (int i = tid; i < M * JD_STRIP; i += DG_THREADS) {
        const int gy = y0 + (i >> 7), gx = x0 + (i & 127);
        if (gy >= a.H || gx >= a.W) continue;
        const int Y = pix[(gy - ry0[0]) * JD_PIX_PITCH + gx - 8 * bx0[0]];
        int px[3] = {Y, Y, Y};
        if (C == 3) {
            int cv[2];
#pragma unroll
            for (int p = 1; p < C; ++p) {
                const uint8_t *pl = pix + p * JD_PIX_ROWS * JD_PIX_PITCH;
                if (!SUB) {
                    cv[p - 1] = pl[(gy - ry0[p]) * JD_PIX_PITCH + gx - 8 * bx0[p]];
                } else {
                    const int cy = gy >> 1, cx = gx >> 1;
                    const int ny = clampi(cy + ((gy & 1) ? 1 : -1), 0, 8 * a.hb[p] - 1), nx = clampi(cx + ((gx & 1) ? 1 : -1), 0, 8 * a.wb[p] - 1);
                    const uint8_t *r0 = pl + (cy - ry0[p]) * JD_PIX_PITCH - 8 * bx0[p], *r1 = pl + (ny - ry0[p]) * JD_PIX_PITCH - 8 * bx0[p];
                    cv[p - 1] = (9 * r0[cx] + 3 * r1[cx] + 3 * r0[nx] + r1[nx] + 8) >> 4;
                }
            }
            const int cb = cv[0] - 128, cr = cv[1] - 128;
            px[0] = clampi(Y + ((91881 * cr + 32768) >> 16), 0, 255);
            px[1] = clampi(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0, 255);
            px[2] = clampi(Y + ((116130 * cb + 32768) >> 16), 0, 255);
        }
        const size_t at = ((size_t)gy * (size_t)a.W + (size_t)gx) * C;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            if (F32) static_cast<float *>(a.out)[at + ch] = (float)px[ch] / 255.0f;
            else static_cast<uint8_t *>(a.out)[at + ch] = (uint8_t)px[ch];
        }
    }
}

template <int C, bool SUB>
int jd_launch(hipStream_t st, const jd_args &a, int f32)
{
    constexpr int M = SUB ? 16 : 8;
    const dim3 grid((unsigned)((a.W + JD_STRIP - 1) / JD_STRIP), (unsigned)((a.H + M - 1) / M));
    if (f32) hipLaunchKernelGGL((jpeg_decode_kernel<C, SUB, true>), grid, dim3(DG_THREADS), 0, st, a);
    else hipLaunchKernelGGL((jpeg_decode_kernel<C, SUB, false>), grid, dim3(DG_THREADS), 0, st, a);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

}  // namespace

extern "C" int femasr_degrade_blur_f32(void *stream, const float *src, int H, int W, const float *kernel, int k, int stride, float *dst)
{
    FEMASR_REQUIRE(src && kernel && dst, "degrade_blur_f32: null argument");
    FEMASR_REQUIRE((((uintptr_t)src | (uintptr_t)kernel | (uintptr_t)dst) & 3u) == 0, "degrade_blur_f32: a pointer is not 4-byte aligned");
    FEMASR_REQUIRE(H >= 1 && W >= 1 && H <= (1 << 24) && W <= (1 << 24), "degrade_blur_f32: %dx%d is outside 1..2^24 pixels a side", H, W);
    FEMASR_REQUIRE(k >= 3 && k <= 25 && (k & 1), "degrade_blur_f32: kernel size %d is not odd in 3..25", k);
    FEMASR_REQUIRE(stride == 1 || stride == 2 || stride == 4, "degrade_blur_f32: stride %d is not 1, 2 or 4", stride);
    const int out_h = (H + stride - 1) / stride, out_w = (W + stride - 1) / stride;
    const int tx = 16;
    int ty = 16;
    auto lds = [&](int t) { return (size_t)((t - 1) * stride + k) * (size_t)((tx - 1) * stride + k) * 12; };
    while (ty > 1 && lds(ty) > DG_LDS_BYTES) ty >>= 1;
    const unsigned gy = (unsigned)((out_h + ty - 1) / ty);
    FEMASR_REQUIRE(lds(ty) <= DG_LDS_BYTES && gy <= 65535u, "degrade_blur_f32: %d rows of output are more than 65535 tiles of %d", out_h, ty);
    hipLaunchKernelGGL(degrade_blur_kernel, dim3((unsigned)((out_w + tx - 1) / tx), gy), dim3(DG_THREADS), lds(ty), (hipStream_t)stream, src, H, W,
                       kernel, k, stride, dst, out_h, out_w, tx, ty);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

extern "C" int femasr_degrade_resize_f32(void *stream, const float *src, int H, int W, float *dst, int out_h, int out_w, const float *w_h,
                                         const int32_t *idx_h, int taps_h, const float *w_w, const int32_t *idx_w, int taps_w, const int32_t *idx_h_host,
                                         const int32_t *idx_w_host)
{
    FEMASR_REQUIRE(src && dst && w_h && idx_h && w_w && idx_w && idx_h_host && idx_w_host, "degrade_resize_f32: null argument");
    FEMASR_REQUIRE((((uintptr_t)src | (uintptr_t)dst | (uintptr_t)w_h | (uintptr_t)idx_h | (uintptr_t)w_w | (uintptr_t)idx_w) & 3u) == 0,
                   "degrade_resize_f32: a pointer is not 4-byte aligned");
    FEMASR_REQUIRE(H >= 1 && W >= 1 && out_h >= 1 && out_w >= 1, "degrade_resize_f32: empty shape: %dx%d -> %dx%d", H, W, out_h, out_w);
    FEMASR_REQUIRE(taps_h >= 1 && taps_w >= 1 && taps_h <= 4096 && taps_w <= 4096, "degrade_resize_f32: %d and %d taps are outside 1..4096", taps_h, taps_w);
    FEMASR_REQUIRE((long long)W * 3 <= INT_MAX && out_w <= INT_MAX - DR_TILE, "degrade_resize_f32: a row of %d or %d pixels reaches 2^31", W, out_w);
    for (size_t i = 0; i < (size_t)out_h * taps_h; ++i)
        FEMASR_REQUIRE(idx_h_host[i] >= 0 && idx_h_host[i] < H, "degrade_resize_f32: idx_h[%zu] = %d is outside the source rows 0..%d", i, idx_h_host[i], H - 1);
    for (size_t i = 0; i < (size_t)out_w * taps_w; ++i)
        FEMASR_REQUIRE(idx_w_host[i] >= 0 && idx_w_host[i] < W, "degrade_resize_f32: idx_w[%zu] = %d is outside the source columns 0..%d", i, idx_w_host[i], W - 1);
    int tile = out_w < DR_TILE ? out_w : DR_TILE;
    while (tile > 1 && dr_lds_bytes(tile, taps_w, dr_window(tile, W, out_w, taps_w)) > DG_LDS_BYTES) --tile;
    const int cap = dr_window(tile, W, out_w, taps_w);
    const size_t lds = dr_lds_bytes(tile, taps_w, cap);
    FEMASR_REQUIRE(lds <= DG_LDS_BYTES, "degrade_resize_f32: %d taps per output column (width %d -> %d) cannot be staged in %zu bytes of LDS", taps_w,
                   W, out_w, DG_LDS_BYTES);
    const int tiles = (out_w + tile - 1) / tile;
    FEMASR_REQUIRE((long long)tiles * out_h <= (1ll << 31) - 1, "degrade_resize_f32: %dx%d has more than 2^31 - 1 blocks of %d pixels", out_h, out_w, tile);
    hipLaunchKernelGGL(degrade_resize_kernel, dim3((unsigned)((long long)tiles * out_h)), dim3(DG_THREADS), lds, (hipStream_t)stream, src, H, W, dst,
                       out_w, w_h, idx_h, taps_h, w_w, idx_w, taps_w, tile, tiles, cap);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

extern "C" int femasr_degrade_noise_f32(void *stream, const float *src, float *dst, long long pixels, unsigned long long pixel_offset, int mode,
                                        const double *factor, unsigned long long seed)
{
    FEMASR_REQUIRE(src && dst && factor, "degrade_noise_f32: null argument");
    FEMASR_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & 3u) == 0, "degrade_noise_f32: a pointer is not 4-byte aligned");
    FEMASR_REQUIRE(pixels >= 1 && pixels <= (1ll << 40), "degrade_noise_f32: %lld pixels are outside 1..2^40", pixels);
    FEMASR_REQUIRE(pixel_offset <= (1ull << 60), "degrade_noise_f32: pixel offset %llu is above 2^60", pixel_offset);
    FEMASR_REQUIRE(mode >= 0 && mode <= 2, "degrade_noise_f32: mode %d is not 0 (colour), 1 (gray) or 2 (correlated)", mode);
    dn_factor f;
    for (int i = 0; i < 9; ++i) {
        FEMASR_REQUIRE(factor[i] == factor[i] && factor[i] >= -16.0 && factor[i] <= 16.0, "degrade_noise_f32: factor[%d] = %g is outside -16..16", i, factor[i]);
        f.a[i] = factor[i];
    }
    // the stream of an operation: base = splitmix64(seed) (degrade.noise_base)
    unsigned long long b = seed + 0x9E3779B97F4A7C15ull;
    b = (b ^ (b >> 30)) * 0xBF58476D1CE4E5B9ull;
    b = (b ^ (b >> 27)) * 0x94D049BB133111EBull;
    b ^= b >> 31;
    hipLaunchKernelGGL(degrade_noise_kernel, dim3(grid_for((size_t)pixels)), dim3(DG_THREADS), 0, (hipStream_t)stream, src, dst, (size_t)pixels,
                       (uint64_t)pixel_offset, mode, f, (uint64_t)b);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

extern "C" int femasr_degrade_quantize_u8(void *stream, const float *src, uint8_t *dst, long long n)
{
    FEMASR_REQUIRE(src && dst, "degrade_quantize_u8: null argument");
    FEMASR_REQUIRE(((uintptr_t)src & 3u) == 0, "degrade_quantize_u8: src is not 4-byte aligned");
    FEMASR_REQUIRE(n >= 1 && n <= (1ll << 42), "degrade_quantize_u8: %lld elements are outside 1..2^42", n);
    hipLaunchKernelGGL(degrade_quantize_kernel, dim3(grid_for((size_t)n)), dim3(DG_THREADS), 0, (hipStream_t)stream, src, dst, (size_t)n);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

extern "C" int femasr_degrade_unit_f32(void *stream, const uint8_t *src, int H, int W, int pitch, float *dst)
{
    FEMASR_REQUIRE(src && dst, "degrade_unit_f32: null argument");
    FEMASR_REQUIRE(((uintptr_t)dst & 3u) == 0, "degrade_unit_f32: dst is not 4-byte aligned");
    FEMASR_REQUIRE(H >= 1 && W >= 1 && pitch >= W, "degrade_unit_f32: %dx%d pixels at a pitch of %d", H, W, pitch);
    const size_t n = (size_t)H * (size_t)W * 3;
    hipLaunchKernelGGL(degrade_unit_kernel, dim3(grid_for(n)), dim3(DG_THREADS), 0, (hipStream_t)stream, src, W, (size_t)pitch, dst, n);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

extern "C" int femasr_jpeg_decode_u8(void *stream, const int16_t *y, const int16_t *cb, const int16_t *cr, int C, int subsampling, int H, int W,
                                     const uint32_t *qtab_y, const uint32_t *qtab_c, void *out, int out_f32)
{
    FEMASR_REQUIRE(C == 1 || C == 3, "jpeg_decode_u8: C = %d is not 1 (gray) or 3 (RGB)", C);
    FEMASR_REQUIRE(C == 1 || subsampling == 444 || subsampling == 420, "jpeg_decode_u8: subsampling %d is not 444 or 420", subsampling);
    FEMASR_REQUIRE(H >= 1 && W >= 1 && H <= 65535 && W <= 65535, "jpeg_decode_u8: %dx%d is outside 1..65535 pixels a side", H, W);
    FEMASR_REQUIRE(y && qtab_y && out, "jpeg_decode_u8: null argument");
    FEMASR_REQUIRE(C == 3 ? (qtab_c && cb && cr) : (!cb && !cr), "jpeg_decode_u8: C = %d takes %s", C, C == 3 ? "qtab_c, cb and cr" : "neither cb nor cr");
    FEMASR_REQUIRE((((uintptr_t)y | (uintptr_t)cb | (uintptr_t)cr) & 15u) == 0, "jpeg_decode_u8: the coefficient planes must be 16-byte aligned");
    FEMASR_REQUIRE(out_f32 == 0 || out_f32 == 1, "jpeg_decode_u8: out_f32 = %d is not 0 or 1", out_f32);
    FEMASR_REQUIRE(!out_f32 || ((uintptr_t)out & 3u) == 0, "jpeg_decode_u8: a float32 output must be 4-byte aligned");
    const bool sub = C == 3 && subsampling == 420;
    const int m = sub ? 16 : 8;
    const int my = (H + m - 1) / m, mx = (W + m - 1) / m;
    jd_args a;
    a.coef[0] = y, a.coef[1] = cb, a.coef[2] = cr;
    a.hb[0] = sub ? 2 * my : my, a.wb[0] = sub ? 2 * mx : mx;
    a.hb[1] = a.hb[2] = my, a.wb[1] = a.wb[2] = mx;
    a.qtab[0] = qtab_y, a.qtab[1] = qtab_c;
    a.H = H, a.W = W, a.out = out;
    hipStream_t st = (hipStream_t)stream;
    if (C == 1) return jd_launch<1, false>(st, a, out_f32);
    return sub ? jd_launch<3, true>(st, a, out_f32) : jd_launch<3, false>(st, a, out_f32);
}

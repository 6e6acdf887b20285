// psnr_ssim.hip — PSNR and SSIM of uint8 RGB image pairs in fp64 on gfx950: the 'psnr' / 'ssim' metrics of validation
// (options/train_FeMaSR_LQ_stage.yml: crop_border, test_y_channel) and of scripts/metrics/calculate_psnr_ssim.py.  The definitions are
// femasr_amd/models/femasr_model.py (_to_y, calculate_psnr, _ssim_plane, calculate_ssim).
//
// Schedule of one femasr_psnr_ssim (a, b: (B,H,W,3) uint8 HWC; cropped plane Hc x Wc = (H - 2c) x (W - 2c); P = 1 plane (Y) or 3 (R, G, B)):
//   psnr_ssim_kernel<Y>         grid (nssim + npsnr, B, P), two block roles in one launch:
//     SSIM tile (x < nssim)     32 x 16 outputs of the valid map, (Hc - 10) x (Wc - 10), of one (pair, plane).  Stages the 42 x 26 input
//                               patch of both images as fp64 in LDS (Y computed from the RGB triple), then each thread computes the five
//                               window sums of a, b, a², b², ab for two outputs of one column and their SSIM map values.
//     PSNR chunk (the others)   16 x 256 cropped pixels of one (pair, plane) in raster order: the sum of (a - b)².
//     Each block writes ONE fp64 partial: part[pair][plane][x] (x < nssim: SSIM tiles, then the PSNR chunks).
//   psnr_ssim_finalize_kernel   one block per pair: per plane thread t over partials t, t + 256, .. then an LDS tree; ssim = mean of the map
//                               (per plane, then the planes in channel order / 3), mse = sum / (Hc Wc P), psnr = 10 log10(255² / mse).
//
// Arithmetic.  Each window sum is ONE fp64 accumulator over the 121 products in the order scipy.signal.convolve2d(x, win, 'valid') adds
// them (window row j ascending, then column k, product win[j][k] * x[m + 10 - j][n + 10 - k], from 0.0; no fma anywhere: the library is
// built with -ffp-contract=off), win = outer(g, g) with numpy's g.  On the same plane the sums, and so every value of the SSIM map, are
// _ssim_plane's bits (always in RGB mode, where the plane is the integer channel); only the mean is summed in another order.  A separable
// pass (11 + 11 taps) is cheaper, but it differs from scipy's sums in the last bits, and on a bright, flat 11 x 11 window that moves a map
// value by up to 3e-12: with a one-pixel map that is the whole SSIM.
// Y = fma(b, 24.966, fma(r, 65.481, g * 128.553)) + 16 with r = R / 255 ...: the order in which numpy's `x @ [65.481, 128.553, 24.966]`
// evaluated the dot product with the x86-64 OpenBLAS dgemv it was checked against; another BLAS may round Y 1 ulp apart.
// In RGB mode every PSNR term is an integer <= 65025: the sum is exact, and mse equals numpy's np.mean((a - b) ** 2) bit for bit.
// Reduction order (no atomics): per thread in a fixed order, a 64-lane xor butterfly (every lane ends with the same bits), the four waves in
// order, then finalize as above.  Every sum depends only on the pair's own pixels and on (H, W, crop, mode): run-to-run deterministic and
// batch-invariant; a <-> b only swaps operands of commutative operations, so ssim(a, b) == ssim(b, a), psnr likewise, and ssim(x, x) == 1.
#include "common.h"
#include <math.h>

namespace {

constexpr int PS_THREADS = 256;
constexpr int SS_TW = 32;                        // SSIM tile: 32 output columns (one per lane of a half wave)
constexpr int SS_TH = 16;                        //   x 16 output rows (two per thread)
constexpr int SS_IW = SS_TW + 10, SS_IH = SS_TH + 10;      // staged patch: 42 x 26 fp64 per image = 17.5 KiB of LDS for both
constexpr int PS_PIX = 16 * PS_THREADS;          // PSNR chunk: cropped pixels per block
constexpr int PS_MAX_PAIRS = 65535;              // grid.y

// _ssim_plane's window: g = exp(-((i - 5)²) / (2 * 1.5²)) / its sum, as numpy computes it (these are its fp64 values; the host test holds
// femasr_ssim_window to the definition bit for bit), win = outer(g, g): each entry one IEEE product, folded by the compiler
constexpr double kG[11] = {0x1.0d956b52a1d70p-10, 0x1.f1fe01ae5a5b8p-8, 0x1.26eb175d83f67p-5, 0x1.bff0fe8e98418p-4, 0x1.b43c3f52b19f2p-3,
                           0x1.106560aa892c0p-2,  0x1.b43c3f52b19f2p-3, 0x1.bff0fe8e98418p-4, 0x1.26eb175d83f67p-5, 0x1.f1fe01ae5a5b8p-8,
                           0x1.0d956b52a1d70p-10};
constexpr double kC1 = (0.01 * 255) * (0.01 * 255), kC2 = (0.03 * 255) * (0.03 * 255);

struct Window {
    double w[121];      // row-major
};

constexpr Window make_window()
{
    Window r{};
    for (int j = 0; j < 11; ++j)
        for (int k = 0; k < 11; ++k) r.w[j * 11 + k] = kG[j] * kG[k];
    return r;
}

constexpr Window kWinHost = make_window();
__constant__ Window kWin = make_window();      // read with wave-uniform indices: scalar loads

// value of one cropped pixel in the plane: Y (fp64, not rounded) or channel ch as fp64
template <bool Y>
__device__ __forceinline__ double plane_value(const uint8_t *px, int ch)
{
    if (Y) {
        const double r = (double)px[0] / 255.0, g = (double)px[1] / 255.0, b = (double)px[2] / 255.0;
        return __builtin_fma(b, 24.966, __builtin_fma(r, 65.481, g * 128.553)) + 16.0;
    }
    return (double)px[ch];
}

// sum over the block (256 threads) of v: xor butterfly per wave, the four waves in order; every thread returns the same bits
__device__ __forceinline__ double block_sum(double v, double *red)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// a, b: (B,H,W,3).  Blocks x < ssim_blocks: SSIM tile x (tiles_x per row of tiles); the others: PSNR chunk x - ssim_blocks.  Partials:
// part[(pair * P + plane) * (nssim + npsnr) + slot], slot = x for a tile, nssim + chunk for a chunk.
template <bool Y>
__global__ __launch_bounds__(PS_THREADS) void psnr_ssim_kernel(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, int H, int W,
                                                               int crop, int ssim_blocks, int tiles_x, int nssim, int npsnr,
                                                               double *__restrict__ part)
{
    __shared__ double sa[SS_IH * SS_IW], sb[SS_IH * SS_IW];
    __shared__ double red[PS_THREADS / 64];
    const int pair = blockIdx.y, plane = blockIdx.z, t = threadIdx.x;
    const int Hc = H - 2 * crop, Wc = W - 2 * crop;
    const size_t first = ((size_t)pair * H * W + (size_t)crop * W + crop) * 3;      // top-left cropped pixel of the pair
    const uint8_t *pa = a + first, *pb = b + first;
    double *row = part + ((size_t)pair * gridDim.z + plane) * (size_t)(nssim + npsnr);
    double acc = 0.0;
    int slot;
    if ((int)blockIdx.x < ssim_blocks) {     // (uniform) SSIM tile
        const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
        const int oy0 = ty * SS_TH, ox0 = tx * SS_TW;
        for (int i = t; i < SS_IH * SS_IW; i += PS_THREADS) {
            const int r = i / SS_IW, c = i - r * SS_IW;
            const int y = oy0 + r, x = ox0 + c;
            double va = 0.0, vb = 0.0;       // outside the cropped plane: feeds only outputs past the valid map
            if (y < Hc && x < Wc) {
                const size_t off = ((size_t)y * W + x) * 3;
                va = plane_value<Y>(pa + off, plane);
                vb = plane_value<Y>(pb + off, plane);
            }
            sa[i] = va;
            sb[i] = vb;
        }
        __syncthreads();
        // outputs (r0, c) and (r0 + 1, c) of the tile; window row j of output e meets patch row r0 + e + 10 - j, so walking the patch rows
        // r0 + 11 .. r0 upwards visits j ascending for both outputs (row r0 + 11 is output 1's j = 0, row r0 output 0's j = 10)
        const int c = t & (SS_TW - 1), r0 = 2 * (t / SS_TW);
        double m0[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, m1[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
        for (int i = 11; i >= 0; --i) {
            const double *ra = sa + (r0 + i) * SS_IW + c + 10, *rb = sb + (r0 + i) * SS_IW + c + 10;
#pragma unroll
            for (int kk = 0; kk < 11; ++kk) {
                const double x = ra[-kk], y = rb[-kk];
                const double xx = x * x, yy = y * y, xy = x * y;
                if (i <= 10) {      // (uniform)
                    const double w = kWin.w[(10 - i) * 11 + kk];
                    m0[0] = m0[0] + w * x;
                    m0[1] = m0[1] + w * y;
                    m0[2] = m0[2] + w * xx;
                    m0[3] = m0[3] + w * yy;
                    m0[4] = m0[4] + w * xy;
                }
                if (i >= 1) {
                    const double w = kWin.w[(11 - i) * 11 + kk];
                    m1[0] = m1[0] + w * x;
                    m1[1] = m1[1] + w * y;
                    m1[2] = m1[2] + w * xx;
                    m1[3] = m1[3] + w * yy;
                    m1[4] = m1[4] + w * xy;
                }
            }
        }
        const int Ho = Hc - 10, Wo = Wc - 10;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const double *m = e == 0 ? m0 : m1;
            if (oy0 + r0 + e < Ho && ox0 + c < Wo) {
                const double mu1 = m[0], mu2 = m[1];
                const double s1 = m[2] - mu1 * mu1, s2 = m[3] - mu2 * mu2, s12 = m[4] - mu1 * mu2;
                acc = acc + ((2.0 * mu1 * mu2 + kC1) * (2.0 * s12 + kC2)) / ((mu1 * mu1 + mu2 * mu2 + kC1) * (s1 + s2 + kC2));
            }
        }
        slot = blockIdx.x;
    } else {     // (uniform) PSNR chunk
        const int chunk = blockIdx.x - ssim_blocks;
        const int n = Hc * Wc;               // < 2^31 (B H W 3 < 2^31)
        for (int i = 0; i < PS_PIX / PS_THREADS; ++i) {
            const int p = chunk * PS_PIX + i * PS_THREADS + t;
            if (p < n) {
                const int y = p / Wc, x = p - y * Wc;
                const size_t off = ((size_t)y * W + x) * 3;
                const double d = plane_value<Y>(pa + off, plane) - plane_value<Y>(pb + off, plane);
                acc = acc + d * d;
            }
        }
        slot = nssim + chunk;
    }
    const double s = block_sum(acc, red);
    if (t == 0) row[slot] = s;
}

// sum of p[0..n) by the block: thread t over t, t + 256, .. in order, then an LDS tree; every thread returns the same value
__device__ double tree_sum(const double *p, int n, double *red)
{
    const int t = threadIdx.x;
    double s = 0.0;
    for (int i = t; i < n; i += 256) s = s + p[i];
    red[t] = s;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (t < w) red[t] = red[t] + red[t + w];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void psnr_ssim_finalize_kernel(const double *__restrict__ part, int P, int nssim, int npsnr, double n_map,
                                                                 double n_pix, double *__restrict__ psnr, double *__restrict__ ssim,
                                                                 double *__restrict__ mse)
{
    __shared__ double red[256];
    const int b = blockIdx.x;
    double ss = 0.0, sq = 0.0;
    for (int p = 0; p < P; ++p) {
        const double *row = part + ((size_t)b * P + p) * (size_t)(nssim + npsnr);
        if (ssim) {
            const double s = tree_sum(row, nssim, red) / n_map;
            ss = p == 0 ? s : ss + s;
        }
        if (psnr || mse) {
            const double s = tree_sum(row + nssim, npsnr, red);
            sq = p == 0 ? s : sq + s;
        }
    }
    if (threadIdx.x == 0) {
        if (ssim) ssim[b] = P == 1 ? ss : ss / P;
        const double m = sq / n_pix;
        if (mse) mse[b] = m;
        if (psnr) psnr[b] = m == 0.0 ? (double)INFINITY : 10.0 * log10(65025.0 / m);
    }
}

struct PsPlan {
    int Hc, Wc, P, tiles_x, nssim, npsnr;
};

int make_plan(int B, int H, int W, int crop, int test_y, bool want_ssim, PsPlan *pl)
{
    FEMASR_REQUIRE(B >= 1 && H >= 1 && W >= 1, "psnr_ssim: empty shape B=%d H=%d W=%d", B, H, W);
    FEMASR_REQUIRE(B <= PS_MAX_PAIRS, "psnr_ssim: B = %d pairs per call exceeds %d (split the batch)", B, PS_MAX_PAIRS);
    FEMASR_REQUIRE(test_y == 0 || test_y == 1, "psnr_ssim: test_y must be 0 or 1, got %d", test_y);
    FEMASR_REQUIRE(crop >= 0 && 2 * (long long)crop < H && 2 * (long long)crop < W,
                   "psnr_ssim: crop_border %d leaves nothing of a %dx%d image", crop, H, W);
    const long long px = (long long)H * W;       // (the product of three ints can overflow 64 bits; this one cannot)
    FEMASR_REQUIRE(px < (1ll << 31) && px * 3 * B < (1ll << 31), "psnr_ssim: %d pairs of %dx%dx3 reach 2^31 bytes (split the batch)", B, H, W);
    pl->Hc = H - 2 * crop;
    pl->Wc = W - 2 * crop;
    FEMASR_REQUIRE(!want_ssim || (pl->Hc >= 11 && pl->Wc >= 11),
                   "psnr_ssim: SSIM needs a cropped size of at least 11x11 (its Gaussian window), got %dx%d", pl->Hc, pl->Wc);
    pl->P = test_y ? 1 : 3;
    const int Ho = pl->Hc - 10, Wo = pl->Wc - 10;
    pl->tiles_x = Ho >= 1 && Wo >= 1 ? (Wo + SS_TW - 1) / SS_TW : 0;
    pl->nssim = Ho >= 1 && Wo >= 1 ? pl->tiles_x * ((Ho + SS_TH - 1) / SS_TH) : 0;
    pl->npsnr = (int)(((long long)pl->Hc * pl->Wc + PS_PIX - 1) / PS_PIX);
    return FEMASR_OK;
}

size_t ws_bytes_of(const PsPlan &pl, int B)
{
    const size_t n = (size_t)B * pl.P * (size_t)(pl.nssim + pl.npsnr) * sizeof(double);
    return (n + 255) & ~(size_t)255;
}

}  // namespace

extern "C" {

int femasr_psnr_ssim_workspace_bytes(int B, int H, int W, int crop_border, int test_y, size_t *bytes)
{
    FEMASR_REQUIRE(bytes, "psnr_ssim_workspace_bytes: null argument");
    PsPlan pl;
    const int rc = make_plan(B, H, W, crop_border, test_y, false, &pl);
    if (rc) return rc;
    *bytes = ws_bytes_of(pl, B);
    return FEMASR_OK;
}

int femasr_psnr_ssim(void *stream, const uint8_t *a, const uint8_t *b, int B, int H, int W, int crop_border, int test_y, double *psnr_out,
                     double *ssim_out, double *mse_out, void *ws, size_t ws_bytes)
{
    FEMASR_REQUIRE(a && b && ws, "psnr_ssim: null argument");
    FEMASR_REQUIRE(psnr_out || ssim_out || mse_out, "psnr_ssim: nothing requested (psnr_out, ssim_out and mse_out are all NULL)");
    FEMASR_REQUIRE(((uintptr_t)ws & 255) == 0, "psnr_ssim: workspace must be 256-byte aligned");
    PsPlan pl;
    const int rc = make_plan(B, H, W, crop_border, test_y, ssim_out != nullptr, &pl);
    if (rc) return rc;
    const size_t need = ws_bytes_of(pl, B);
    if (ws_bytes < need) return femasr_set_error(FEMASR_ERR_WORKSPACE, "psnr_ssim: workspace %zu bytes < %zu needed", ws_bytes, need);
    const hipStream_t s = (hipStream_t)stream;
    double *part = (double *)ws;
    const int ssim_blocks = ssim_out ? pl.nssim : 0;
    const int gx = ssim_blocks + (psnr_out || mse_out ? pl.npsnr : 0);
    const dim3 grid((unsigned)gx, (unsigned)B, (unsigned)pl.P);
    if (test_y)
        hipLaunchKernelGGL(psnr_ssim_kernel<true>, grid, dim3(PS_THREADS), 0, s, a, b, H, W, crop_border, ssim_blocks, pl.tiles_x, pl.nssim,
                           pl.npsnr, part);
    else
        hipLaunchKernelGGL(psnr_ssim_kernel<false>, grid, dim3(PS_THREADS), 0, s, a, b, H, W, crop_border, ssim_blocks, pl.tiles_x, pl.nssim,
                           pl.npsnr, part);
    FEMASR_CHECK_HIP(hipGetLastError());
    const double n_map = (double)(pl.Hc - 10) * (double)(pl.Wc - 10), n_pix = (double)pl.Hc * pl.Wc * pl.P;
    hipLaunchKernelGGL(psnr_ssim_finalize_kernel, dim3((unsigned)B), dim3(256), 0, s, part, pl.P, pl.nssim, pl.npsnr, n_map, n_pix, psnr_out,
                       ssim_out, mse_out);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

int femasr_ssim_window(double *win)
{
    FEMASR_REQUIRE(win, "ssim_window: null argument");
    for (int i = 0; i < 121; ++i) win[i] = kWinHost.w[i];
    return FEMASR_OK;
}

}  // extern "C"

// niqe.hip — NIQE features of uint8 RGB images and MATLAB-style bicubic imresize in fp64 on gfx950: validation's no-reference 'niqe'
// metric and the counterpart of scripts/metrics/calculate_niqe.py.  The definitions are femasr_amd/models/femasr_model.py (_niqe_y,
// _convolve_nearest, imresize / imresize_tables, _aggd, niqe_features); the tail (nanmean, cov, pinv, the quadratic form) works on 36
// numbers per block and stays on the host (niqe_score_from_features).
//
// Schedule of one femasr_niqe_features (img: (B,H,W,3) uint8 HWC; cropped Hc x Wc; nh x nw blocks of 96 x 96; plane Hb x Wb = 96 nh x 96 nw):
//   niqe_y_kernel          one thread per pixel of the plane: y = rint(((65.481 R + 128.553 G) + 24.966 B) / 255 + 16), and yn = y / 255
//   niqe_mscn_kernel       32 x 32 outputs per block from a 38 x 38 LDS tile of y (3-pixel halo, clamped at the plane's border: scipy's
//                          mode='nearest'); each thread: 4 outputs of one column, their 49-term sums of w y and of w (y y), then
//                          mu, sigma = sqrt(|sum(w y²) - mu²|), z = (y - mu) / (sigma + 1).  Runs once per scale.
//   imresize_h / _w        y2 = imresize(yn, 0.5) * 255: the H pass into an fp64 intermediate, then the W pass; one thread per output, the
//                          taps of the host-built weight / index tables in ascending order
//   niqe_block_kernel      one block of 256 threads per (image, scale, 96 >> scale block): the five maps (z and z times its four circular
//                          shifts INSIDE the block) of every pixel, six moments per map, the AGGD solve, 18 features + 5 grid positions
//
// Arithmetic.  All fp64, no fma (the library is built with -ffp-contract=off), every sum ONE accumulator from 0.0 in the definition's
// order: the 7 x 7 sums walk the flipped window in raster order as scipy.ndimage.convolve does, the resize sums their taps ascending.
// fp64 sqrt and divide are IEEE, so y, z (both scales) and the resized plane are the definition's bits.  The block moments are summed in
// another order than numpy's pairwise mean (below), so the features agree to rounding (<= 9216 terms); the grid search is the definition's
// first minimum of (r_gam - rn)² with NaN objectives selecting position 0, and gamma values come from the host's tables: no device gamma.
// Reduction order (no atomics): thread t over the block's pixels t, t + 256, .. in raster order, a 64-lane xor butterfly (every lane ends
// with the same bits), the four waves in order.  Every sum depends only on the block's own pixels and on the scale: run-to-run
// deterministic, independent of B and of the image's place in the batch.
#include "common.h"
#include <math.h>

namespace {

constexpr int NQ_THREADS = 256;
constexpr int NQ_BLOCK = 96;                     // NIQE's block size at scale 1 (48 at scale 2)
constexpr int NQ_GAM = 9801;                     // arange(0.2, 10.001, 0.001)
constexpr int NQ_MAX_IMAGES = 65535;             // grid.y / grid.z
constexpr int MS_TW = 32, MS_TH = 32;            // MSCN tile: 32 columns (one per lane of a half wave) x 32 rows (four per thread)
constexpr int MS_IW = MS_TW + 6, MS_IH = MS_TH + 6;      // staged tile: 38 x 38 fp64 = 11.3 KiB of LDS
constexpr int NQ_SUMS = 30;                      // per block: 5 maps x (n<0, sum x² | x<0, n>0, sum x² | x>0, sum |x|, sum x²)

// img: (B,H,W,3); y, yn: (B,Hb,Wb), the top-left Hb x Wb of the cropped image
__global__ __launch_bounds__(NQ_THREADS) void niqe_y_kernel(const uint8_t *__restrict__ img, int H, int W, int crop, int Hb, int Wb,
                                                            double *__restrict__ y, double *__restrict__ yn)
{
    const int b = blockIdx.y, n = Hb * Wb;
    const int p = blockIdx.x * NQ_THREADS + threadIdx.x;
    if (p >= n) return;
    const int r = p / Wb, c = p - r * Wb;
    const uint8_t *px = img + ((size_t)b * H * W + (size_t)(r + crop) * W + (c + crop)) * 3;
    const double R = (double)px[0], G = (double)px[1], B = (double)px[2];
    const double v = rint(((65.481 * R + 128.553 * G) + 24.966 * B) / 255.0 + 16.0);      // round half to even, as np.round
    y[(size_t)b * n + p] = v;
    yn[(size_t)b * n + p] = v / 255.0;
}

// y, z: (B,Hs,Ws); win: the 7 x 7 window as given (row-major); tile blockIdx.x of tiles_x per row of tiles
__global__ __launch_bounds__(NQ_THREADS) void niqe_mscn_kernel(const double *__restrict__ y, int Hs, int Ws, int tiles_x,
                                                               const double *__restrict__ win, double *__restrict__ z)
{
    __shared__ double sy[MS_IH * MS_IW];
    const int t = threadIdx.x, b = blockIdx.y;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int oy0 = ty * MS_TH, ox0 = tx * MS_TW;
    const double *src = y + (size_t)b * Hs * Ws;
    for (int i = t; i < MS_IH * MS_IW; i += NQ_THREADS) {
        const int r = i / MS_IW, c = i - r * MS_IW;
        const int gy = clampi(oy0 + r - 3, 0, Hs - 1), gx = clampi(ox0 + c - 3, 0, Ws - 1);
        sy[i] = src[(size_t)gy * Ws + gx];
    }
    __syncthreads();
    // outputs (r0 + e, c), e = 0..3.  scipy sums wf[a][k] * y[i + a - 3][j + k - 3] over a, then k, ascending, with wf the flipped window:
    // output e meets tile row r0 + i with a = i - e, so walking the rows i = 0..9 visits a ascending for each of the four accumulators
    const int c = t & (MS_TW - 1), r0 = 4 * (t / MS_TW);
    double m[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 10; ++i) {
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const double x = sy[(r0 + i) * MS_IW + c + k];
            const double xx = x * x;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int a = i - e;
                if (a >= 0 && a < 7) {      // (compile time)
                    const double w = win[(6 - a) * 7 + (6 - k)];      // wave-uniform index: scalar loads
                    m[e] = m[e] + w * x;
                    q[e] = q[e] + w * xx;
                }
            }
        }
    }
    double *dst = z + (size_t)b * Hs * Ws;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int oy = oy0 + r0 + e, ox = ox0 + c;
        if (oy < Hs && ox < Ws) {
            const double mu = m[e];
            const double sigma = sqrt(fabs(q[e] - mu * mu));
            dst[(size_t)oy * Ws + ox] = (sy[(r0 + e + 3) * MS_IW + c + 3] - mu) / (sigma + 1.0);
        }
    }
}

// H pass: in (N,H,W) -> out (N,Ho,W) fp64; w, idx: (Ho,P) weights and 0-based source rows (reflected by the host), taps ascending
template <typename Tin>
__global__ __launch_bounds__(NQ_THREADS) void imresize_h_kernel(const Tin *__restrict__ in, int H, int W, int Ho, const double *__restrict__ w,
                                                                const int32_t *__restrict__ idx, int P, double *__restrict__ out)
{
    const int n = blockIdx.y;
    const int p = blockIdx.x * NQ_THREADS + threadIdx.x;
    if (p >= Ho * W) return;
    const int i = p / W, x = p - i * W;
    const Tin *src = in + (size_t)n * H * W + x;
    double acc = 0.0;
    for (int k = 0; k < P; ++k) {
        const int j = clampi(idx[i * P + k], 0, H - 1);      // (tables from imresize_tables are in range; the clamp keeps a bad table in bounds)
        acc = acc + w[i * P + k] * (double)src[(size_t)j * W];
    }
    out[(size_t)n * Ho * W + p] = acc;
}

// W pass: in (N,Ho,W) fp64 -> out (N,Ho,Wo); the result times out_mul (1.0 leaves the bits) in Tout
template <typename Tout>
__global__ __launch_bounds__(NQ_THREADS) void imresize_w_kernel(const double *__restrict__ in, int Ho, int W, int Wo, const double *__restrict__ w,
                                                                const int32_t *__restrict__ idx, int P, double out_mul, Tout *__restrict__ out)
{
    const int n = blockIdx.y;
    const int p = blockIdx.x * NQ_THREADS + threadIdx.x;
    if (p >= Ho * Wo) return;
    const int yy = p / Wo, j = p - yy * Wo;
    const double *src = in + (size_t)n * Ho * W + (size_t)yy * W;
    double acc = 0.0;
    for (int k = 0; k < P; ++k) {
        const int x = clampi(idx[j * P + k], 0, W - 1);
        acc = acc + w[j * P + k] * src[x];
    }
    out[(size_t)n * Ho * Wo + p] = (Tout)(acc * out_mul);
}

// z1: (B,Hb,Wb), z2: (B,Hb/2,Wb/2).  grid (nh nw, 2, B); block index iw * nh + ih (the definition's order: columns of blocks first).
// tab: five tables of 9801 fp64: r_gam, gamma(1/gam), gamma(2/gam), gamma(3/gam), gam.  feat: (B, nh nw, 36), pos: (B, nh nw, 10).
__global__ __launch_bounds__(NQ_THREADS) void niqe_block_kernel(const double *__restrict__ z1, const double *__restrict__ z2, int Hb, int Wb,
                                                                int nh, const double *__restrict__ tab, double *__restrict__ feat,
                                                                int32_t *__restrict__ pos)
{
    __shared__ double red[4 * NQ_SUMS];
    __shared__ double redv[4];
    __shared__ int redi[4];
    const int t = threadIdx.x, blk = blockIdx.x, scale = blockIdx.y, b = blockIdx.z;
    const int iw = blk / nh, ih = blk - iw * nh;
    const int n = NQ_BLOCK >> scale, Hs = Hb >> scale, Ws = Wb >> scale;
    const double *zp = (scale ? z2 : z1) + (size_t)b * Hs * Ws + (size_t)(ih * n) * Ws + iw * n;
    double s[NQ_SUMS];
#pragma unroll
    for (int j = 0; j < NQ_SUMS; ++j) s[j] = 0.0;
    for (int p = t; p < n * n; p += NQ_THREADS) {
        const int r = p / n, c = p - r * n;
        const int rm = r == 0 ? n - 1 : r - 1, cm = c == 0 ? n - 1 : c - 1, cp = c == n - 1 ? 0 : c + 1;
        const double x = zp[(size_t)r * Ws + c];
        // np.roll(block, (s0, s1), axis=(0, 1))[r][c] = block[(r - s0) % n][(c - s1) % n] for the shifts (0,1), (1,0), (1,1), (1,-1)
        const double v[5] = {x, x * zp[(size_t)r * Ws + cm], x * zp[(size_t)rm * Ws + c], x * zp[(size_t)rm * Ws + cm],
                             x * zp[(size_t)rm * Ws + cp]};
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            const double xx = v[m] * v[m];
            const bool neg = v[m] < 0.0, ps = v[m] > 0.0;
            s[m * 6 + 0] = s[m * 6 + 0] + (neg ? 1.0 : 0.0);      // counts: exact in fp64
            s[m * 6 + 1] = s[m * 6 + 1] + (neg ? xx : 0.0);
            s[m * 6 + 2] = s[m * 6 + 2] + (ps ? 1.0 : 0.0);
            s[m * 6 + 3] = s[m * 6 + 3] + (ps ? xx : 0.0);
            s[m * 6 + 4] = s[m * 6 + 4] + fabs(v[m]);
            s[m * 6 + 5] = s[m * 6 + 5] + xx;
        }
    }
#pragma unroll
    for (int j = 0; j < NQ_SUMS; ++j) {
        double v = s[j];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, 64);
        if ((t & 63) == 0) red[(t >> 6) * NQ_SUMS + j] = v;
    }
    __syncthreads();
    const double npix = (double)(n * n);
    const double *r_gam = tab, *g1 = tab + NQ_GAM, *g2 = tab + 2 * NQ_GAM, *g3 = tab + 3 * NQ_GAM, *gam = tab + 4 * NQ_GAM;
    double *f = feat + ((size_t)b * gridDim.x + blk) * 36 + scale * 18;
    int32_t *pp = pos + ((size_t)b * gridDim.x + blk) * 10 + scale * 5;
    for (int m = 0; m < 5; ++m) {
        double u[6];      // the same bits in every thread
#pragma unroll
        for (int j = 0; j < 6; ++j)
            u[j] = ((red[m * 6 + j] + red[NQ_SUMS + m * 6 + j]) + red[2 * NQ_SUMS + m * 6 + j]) + red[3 * NQ_SUMS + m * 6 + j];
        const double l = sqrt(u[1] / u[0]), r = sqrt(u[3] / u[2]);      // an empty side: 0 / 0 = NaN, as numpy's mean of nothing
        const double g = l / r;
        const double ma = u[4] / npix;
        const double rhat = ma * ma / (u[5] / npix);
        const double gg = g * g;
        const double rn = rhat * (gg * g + 1.0) * (g + 1.0) / ((gg + 1.0) * (gg + 1.0));
        // first minimum of (r_gam - rn)²; a NaN rn makes every objective NaN and numpy's argmin returns 0
        double best = INFINITY;
        int best_i = 0;
        if (rn == rn) {      // (uniform)
            for (int i = t; i < NQ_GAM; i += NQ_THREADS) {
                const double d = r_gam[i] - rn;
                const double o = d * d;
                if (o < best) {
                    best = o;
                    best_i = i;
                }
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const double ob = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(best_i, o, 64);
            if (ob < best || (ob == best && oi < best_i)) {
                best = ob;
                best_i = oi;
            }
        }
        __syncthreads();      // (the previous map's redv / redi have been read)
        if ((t & 63) == 0) {
            redv[t >> 6] = best;
            redi[t >> 6] = best_i;
        }
        __syncthreads();
        if (t == 0) {
            best = redv[0];
            best_i = redi[0];
            for (int w = 1; w < 4; ++w)
                if (redv[w] < best || (redv[w] == best && redi[w] < best_i)) {
                    best = redv[w];
                    best_i = redi[w];
                }
            const double k = sqrt(g1[best_i] / g3[best_i]);
            const double bl = l * k, br = r * k;
            pp[m] = best_i;
            if (m == 0) {
                f[0] = gam[best_i];
                f[1] = (bl + br) / 2.0;
            } else {
                double *fm = f + 2 + 4 * (m - 1);
                fm[0] = gam[best_i];
                fm[1] = (br - bl) * (g2[best_i] / g1[best_i]);
                fm[2] = bl;
                fm[3] = br;
            }
        }
    }
}

struct NqPlan {
    int Hb, Wb, nh, nw;
    size_t n1;      // B Hb Wb
};

int make_plan(int B, int H, int W, int crop, NqPlan *pl)
{
    FEMASR_REQUIRE(B >= 1 && H >= 1 && W >= 1, "niqe: empty shape B=%d H=%d W=%d", B, H, W);
    FEMASR_REQUIRE(B <= NQ_MAX_IMAGES, "niqe: B = %d images per call exceeds %d (split the batch)", B, NQ_MAX_IMAGES);
    FEMASR_REQUIRE(crop >= 0 && 2 * (long long)crop < H && 2 * (long long)crop < W, "niqe: crop_border %d leaves nothing of a %dx%d image",
                   crop, H, W);
    const long long px = (long long)H * W;       // (the product of three ints can overflow 64 bits; this one cannot)
    FEMASR_REQUIRE(px < (1ll << 31) && px * 3 * B < (1ll << 31), "niqe: %d images of %dx%dx3 reach 2^31 bytes (split the batch)", B, H, W);
    pl->nh = (H - 2 * crop) / NQ_BLOCK;
    pl->nw = (W - 2 * crop) / NQ_BLOCK;
    FEMASR_REQUIRE(pl->nh >= 1 && pl->nw >= 1, "niqe: a cropped size of %dx%d holds no 96x96 block", H - 2 * crop, W - 2 * crop);
    pl->Hb = pl->nh * NQ_BLOCK;
    pl->Wb = pl->nw * NQ_BLOCK;
    pl->n1 = (size_t)B * pl->Hb * pl->Wb;
    return FEMASR_OK;
}

// workspace planes in doubles, each a multiple of 32 doubles (256 bytes): y, yn, z1 (n1), the H-pass intermediate (n1 / 2), y2, z2 (n1 / 4)
enum { NQ_Y, NQ_YN, NQ_Z1, NQ_TMP, NQ_Y2, NQ_Z2, NQ_PLANES };

void plane_offsets(const NqPlan &pl, size_t off[NQ_PLANES + 1])
{
    const size_t sz[NQ_PLANES] = {pl.n1, pl.n1, pl.n1, pl.n1 / 2, pl.n1 / 4, pl.n1 / 4};      // (n1 is a multiple of 96² = 9216)
    off[0] = 0;
    for (int i = 0; i < NQ_PLANES; ++i) off[i + 1] = off[i] + ((sz[i] + 31) & ~(size_t)31);
}

int check_resize_shape(int N, int H, int W, int Ho, int Wo, int Ph, int Pw)
{
    FEMASR_REQUIRE(N >= 1 && H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1, "imresize: empty shape N=%d %dx%d -> %dx%d", N, H, W, Ho, Wo);
    FEMASR_REQUIRE(N <= NQ_MAX_IMAGES, "imresize: N = %d planes per call exceeds %d (split the batch)", N, NQ_MAX_IMAGES);
    FEMASR_REQUIRE(Ph >= 1 && Pw >= 1, "imresize: tap counts %d, %d", Ph, Pw);
    FEMASR_REQUIRE((long long)H * W < (1ll << 31) && (long long)Ho * W < (1ll << 31) && (long long)Ho * Wo < (1ll << 31) &&
                       (long long)Ho * Ph < (1ll << 31) && (long long)Wo * Pw < (1ll << 31),
                   "imresize: a plane of %dx%d -> %dx%d reaches 2^31 elements", H, W, Ho, Wo);
    return FEMASR_OK;
}

template <typename Tin, typename Tout>
int launch_resize(hipStream_t s, const Tin *in, int N, int H, int W, int Ho, int Wo, const double *w_h, const int32_t *idx_h, int Ph,
                  const double *w_w, const int32_t *idx_w, int Pw, double out_mul, Tout *out, double *tmp)
{
    const dim3 gh((unsigned)(((long long)Ho * W + NQ_THREADS - 1) / NQ_THREADS), (unsigned)N);
    hipLaunchKernelGGL(imresize_h_kernel<Tin>, gh, dim3(NQ_THREADS), 0, s, in, H, W, Ho, w_h, idx_h, Ph, tmp);
    FEMASR_CHECK_HIP(hipGetLastError());
    const dim3 gw((unsigned)(((long long)Ho * Wo + NQ_THREADS - 1) / NQ_THREADS), (unsigned)N);
    hipLaunchKernelGGL(imresize_w_kernel<Tout>, gw, dim3(NQ_THREADS), 0, s, (const double *)tmp, Ho, W, Wo, w_w, idx_w, Pw, out_mul, out);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

}  // namespace

extern "C" {

int femasr_imresize_workspace_bytes(int N, int H, int W, int Ho, int Wo, size_t *bytes)
{
    FEMASR_REQUIRE(bytes, "imresize_workspace_bytes: null argument");
    const int rc = check_resize_shape(N, H, W, Ho, Wo, 1, 1);
    if (rc) return rc;
    *bytes = ((size_t)N * Ho * W * sizeof(double) + 255) & ~(size_t)255;
    return FEMASR_OK;
}

int femasr_imresize(void *stream, const void *in, int is_f64, int N, int H, int W, int Ho, int Wo, const double *w_h, const int32_t *idx_h,
                    int taps_h, const double *w_w, const int32_t *idx_w, int taps_w, void *out, void *ws, size_t ws_bytes)
{
    FEMASR_REQUIRE(in && out && ws && w_h && idx_h && w_w && idx_w, "imresize: null argument");
    FEMASR_REQUIRE(is_f64 == 0 || is_f64 == 1, "imresize: is_f64 must be 0 (float32 planes) or 1 (float64), got %d", is_f64);
    FEMASR_REQUIRE(((uintptr_t)ws & 255) == 0, "imresize: workspace must be 256-byte aligned");
    const int rc = check_resize_shape(N, H, W, Ho, Wo, taps_h, taps_w);
    if (rc) return rc;
    const size_t need = ((size_t)N * Ho * W * sizeof(double) + 255) & ~(size_t)255;
    if (ws_bytes < need) return femasr_set_error(FEMASR_ERR_WORKSPACE, "imresize: workspace %zu bytes < %zu needed", ws_bytes, need);
    const hipStream_t s = (hipStream_t)stream;
    if (is_f64)
        return launch_resize(s, (const double *)in, N, H, W, Ho, Wo, w_h, idx_h, taps_h, w_w, idx_w, taps_w, 1.0, (double *)out, (double *)ws);
    return launch_resize(s, (const float *)in, N, H, W, Ho, Wo, w_h, idx_h, taps_h, w_w, idx_w, taps_w, 1.0, (float *)out, (double *)ws);
}

int femasr_niqe_workspace_bytes(int B, int H, int W, int crop_border, size_t *bytes)
{
    FEMASR_REQUIRE(bytes, "niqe_workspace_bytes: null argument");
    NqPlan pl;
    const int rc = make_plan(B, H, W, crop_border, &pl);
    if (rc) return rc;
    size_t off[NQ_PLANES + 1];
    plane_offsets(pl, off);
    *bytes = off[NQ_PLANES] * sizeof(double);
    return FEMASR_OK;
}

int femasr_niqe_plane_offsets(int B, int H, int W, int crop_border, size_t offsets[4])
{
    FEMASR_REQUIRE(offsets, "niqe_plane_offsets: null argument");
    NqPlan pl;
    const int rc = make_plan(B, H, W, crop_border, &pl);
    if (rc) return rc;
    size_t off[NQ_PLANES + 1];
    plane_offsets(pl, off);
    offsets[0] = off[NQ_Y] * sizeof(double);
    offsets[1] = off[NQ_Z1] * sizeof(double);
    offsets[2] = off[NQ_Y2] * sizeof(double);
    offsets[3] = off[NQ_Z2] * sizeof(double);
    return FEMASR_OK;
}

int femasr_niqe_features(void *stream, const uint8_t *img, int B, int H, int W, int crop_border, const double *window, const double *tables,
                         const double *w_h, const int32_t *idx_h, int taps_h, const double *w_w, const int32_t *idx_w, int taps_w,
                         double *features, int32_t *positions, void *ws, size_t ws_bytes)
{
    FEMASR_REQUIRE(img && window && tables && w_h && idx_h && w_w && idx_w && features && positions && ws, "niqe: null argument");
    FEMASR_REQUIRE(((uintptr_t)ws & 255) == 0, "niqe: workspace must be 256-byte aligned");
    FEMASR_REQUIRE(taps_h >= 1 && taps_w >= 1, "niqe: tap counts %d, %d", taps_h, taps_w);
    NqPlan pl;
    const int rc = make_plan(B, H, W, crop_border, &pl);
    if (rc) return rc;
    size_t off[NQ_PLANES + 1];
    plane_offsets(pl, off);
    const size_t need = off[NQ_PLANES] * sizeof(double);
    if (ws_bytes < need) return femasr_set_error(FEMASR_ERR_WORKSPACE, "niqe: workspace %zu bytes < %zu needed", ws_bytes, need);
    const hipStream_t s = (hipStream_t)stream;
    double *base = (double *)ws;
    double *y = base + off[NQ_Y], *yn = base + off[NQ_YN], *z1 = base + off[NQ_Z1], *tmp = base + off[NQ_TMP], *y2 = base + off[NQ_Y2],
           *z2 = base + off[NQ_Z2];
    const int Hb = pl.Hb, Wb = pl.Wb, H2 = Hb / 2, W2 = Wb / 2;
    hipLaunchKernelGGL(niqe_y_kernel, dim3((unsigned)(((long long)Hb * Wb + NQ_THREADS - 1) / NQ_THREADS), (unsigned)B), dim3(NQ_THREADS), 0, s,
                       img, H, W, crop_border, Hb, Wb, y, yn);
    FEMASR_CHECK_HIP(hipGetLastError());
    const int tx1 = (Wb + MS_TW - 1) / MS_TW, ty1 = (Hb + MS_TH - 1) / MS_TH;
    hipLaunchKernelGGL(niqe_mscn_kernel, dim3((unsigned)(tx1 * ty1), (unsigned)B), dim3(NQ_THREADS), 0, s, (const double *)y, Hb, Wb, tx1, window,
                       z1);
    FEMASR_CHECK_HIP(hipGetLastError());
    const int rr = launch_resize(s, (const double *)yn, B, Hb, Wb, H2, W2, w_h, idx_h, taps_h, w_w, idx_w, taps_w, 255.0, y2, tmp);
    if (rr) return rr;
    const int tx2 = (W2 + MS_TW - 1) / MS_TW, ty2 = (H2 + MS_TH - 1) / MS_TH;
    hipLaunchKernelGGL(niqe_mscn_kernel, dim3((unsigned)(tx2 * ty2), (unsigned)B), dim3(NQ_THREADS), 0, s, (const double *)y2, H2, W2, tx2, window,
                       z2);
    FEMASR_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(niqe_block_kernel, dim3((unsigned)(pl.nh * pl.nw), 2, (unsigned)B), dim3(NQ_THREADS), 0, s, (const double *)z1,
                       (const double *)z2, Hb, Wb, pl.nh, tables, features, positions);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

}  // extern "C"

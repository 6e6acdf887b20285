// dists.hip — DISTS (Ding et al., "Image Quality Assessment: Unifying Structure and Texture Similarity"; pyiqa 'dists') on gfx950:
// the full-reference metric SR papers report beside LPIPS.  The backbone is the VGG16 of lpips.hip with other glue: ImageNet input
// normalisation, an L2 "Hann" pool instead of the max-pool, and a head of per-channel means, variances and covariances.
//
// Schedule of one femasr_dists_forward (x, y: (B,3,H,W) fp32 NCHW in [0,1]):
//   dists_input_kernel          both images -> ONE NHWC batch of 2B images (x in samples 0..B-1, y in B..2B-1), (v - mean) / std in fp32
//   dists_moments_input_kernel  map 0, the raw NCHW input (C = 3): the five fp64 sums of a run of pixels of one channel per block
//   backbone convs              femasr_conv2d_launch with act = FEMASR_ACT_RELU on the direct fp32 forms, as lpips.hip calls it:
//                               every feature map is bit-identical to oracle.conv2d + ReLU
//   dists_moments_kernel        after the last conv of each stage: per (pair, channel) the sums Sx, Sy, Sxx, Syy, Sxy of a run of pixels
//   dists_reduce_kernel         the runs' partials summed in index order -> sums[map][pair][5][C]
//   dists_l2pool_kernel         in front of stages 2..5: sqrt(conv2d(f^2, hann 3x3 / 16, stride 2, pad 1, groups C) + 1e-12)
//   dists_finalize_kernel       per pair in fp64: means, v = Sxx / N - m^2, S1, S2, the alpha / beta weighted sums, 1 - total / w
// Summation order (no atomics, no cross-lane step on the feature maps): a lane owns one channel and adds the pixels of its block's run
// in ascending order; the run length depends on the map's H x W only; the partials of a (pair, channel) are added in block order; the
// weighted terms in channel order per map, the maps in order.  Map 0 has one cross-lane step: thread t of 256 takes pixels t, t + 256, ..
// of the run, a 64-lane xor butterfly, the four waves in order.  Nothing depends on B, the stream or the pair's place in the batch.
#include "common.h"
#include <string>
#include <vector>

namespace {

constexpr int DS_NMAPS = 6, DS_NSTAGES = 5, DS_NCONV = 13;
constexpr int DS_CTOTAL = 1475;                      // 3 + 64 + 128 + 256 + 512 + 512
constexpr int DS_MAX_PAIRS = 65535;                  // gridDim.y / .z limit: pairs per launch
constexpr int DS_MAX_RUNS = 512;                     // runs (blocks) per map and pair: the partials stay a few percent of a feature map
constexpr int DS_MIN_RUN = 64, DS_MIN_RUN_INPUT = 1024;      // pixels per run at least (feature maps: one lane per channel; input: 256 threads)
constexpr int DS_MIN_SIDE = 8;
const int kMapC[DS_NMAPS] = {3, 64, 128, 256, 512, 512};

struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

__global__ __launch_bounds__(256) void dists_input_kernel(const float *__restrict__ x, const float *__restrict__ y, int B, int H, int W,
                                                          float *__restrict__ out)
{
    const size_t HW = (size_t)H * W, total = 2 * (size_t)B * HW;
    const float mean[3] = {(float)0.485, (float)0.456, (float)0.406};
    const float stdv[3] = {(float)0.229, (float)0.224, (float)0.225};
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t s = i / HW, p = i - s * HW;
        const float *src = s < (size_t)B ? x + s * 3 * HW : y + (s - B) * 3 * HW;
#pragma unroll
        for (int c = 0; c < 3; ++c) out[i * 3 + c] = (src[c * HW + p] - mean[c]) / stdv[c];
    }
}

// f: (B2,H,W,C) NHWC -> out (B2,Hp,Wp,C), Hp = ceil(H / 2).  One wave per (output pixel, 64-channel group): every access is a row of 64
// channels.  g = (1 2 1)(1 2 1)^T / 16: powers of two, so each fmaf rounds once, for the addition.
__global__ __launch_bounds__(256) void dists_l2pool_kernel(const float *__restrict__ f, long long B2, int H, int W, int C, int Hp, int Wp,
                                                           float *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int nj = C >> 6;
    const long long items = B2 * Hp * Wp * nj;
    const long long wave0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * 4;
    for (long long it = wave0; it < items; it += nwaves) {      // (uniform per wave)
        const int j = (int)(it % nj);
        const long long q = it / nj;                             // output pixel over (B2, Hp, Wp)
        const int ox = (int)(q % Wp);
        const long long r = q / Wp;
        const int oy = (int)(r % Hp);
        const long long s = r / Hp;
        const int c = lane + 64 * j;
        const float *src = f + (size_t)s * H * W * C + c;
        float acc = 0.f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = 2 * oy - 1 + ky;
            if (iy < 0 || iy >= H) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = 2 * ox - 1 + kx;
                if (ix < 0 || ix >= W) continue;
                const float v = src[((size_t)iy * W + ix) * C];
                const float g = (ky == 1 ? 0.5f : 0.25f) * (kx == 1 ? 0.5f : 0.25f);
                acc = __builtin_fmaf(g, v * v, acc);
            }
        }
        out[(size_t)q * C + c] = __builtin_sqrtf(acc + 1e-12f);
    }
}

// f: (2B,HW,C) NHWC.  Block (run, 64-channel group, pair) of ONE wave: lane = channel, pixels [run * P, min(HW, (run + 1) * P)) ascending.
// part[pair][run][5][C].  The products of two float32 values are exact in fp64; only the additions round.
__global__ __launch_bounds__(64) void dists_moments_kernel(const float *__restrict__ f, int B, long long HW, int C, int P,
                                                           double *__restrict__ part)
{
    const int run = blockIdx.x, nruns = gridDim.x, b = blockIdx.z;
    const int c = blockIdx.y * 64 + threadIdx.x;
    const float *fx = f + (size_t)b * HW * C + c, *fy = f + (size_t)(b + B) * HW * C + c;
    const long long p0 = (long long)run * P, p1 = p0 + P < HW ? p0 + P : HW;
    double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
    long long p = p0;
    for (; p + 8 <= p1; p += 8) {
        float a[8], d[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {        // sixteen rows in flight
            a[i] = fx[(size_t)(p + i) * C];
            d[i] = fy[(size_t)(p + i) * C];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const double u = (double)a[i], v = (double)d[i];
            sx = sx + u;
            sy = sy + v;
            sxx = sxx + u * u;
            syy = syy + v * v;
            sxy = sxy + u * v;
        }
    }
    for (; p < p1; ++p) {
        const double u = (double)fx[(size_t)p * C], v = (double)fy[(size_t)p * C];
        sx = sx + u;
        sy = sy + v;
        sxx = sxx + u * u;
        syy = syy + v * v;
        sxy = sxy + u * v;
    }
    double *dst = part + ((size_t)b * nruns + run) * 5 * C + c;
    dst[0] = sx;
    dst[(size_t)C] = sy;
    dst[(size_t)2 * C] = sxx;
    dst[(size_t)3 * C] = syy;
    dst[(size_t)4 * C] = sxy;
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

// Map 0: x, y (B,3,HW) NCHW.  Block (run, channel, pair) of 256 threads; part[pair][run][5][3].
__global__ __launch_bounds__(256) void dists_moments_input_kernel(const float *__restrict__ x, const float *__restrict__ y, long long HW, int P,
                                                                  double *__restrict__ part)
{
    __shared__ double red[4][5];
    const int run = blockIdx.x, nruns = gridDim.x, c = blockIdx.y, b = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float *px = x + ((size_t)b * 3 + c) * HW, *py = y + ((size_t)b * 3 + c) * HW;
    const long long p0 = (long long)run * P, p1 = p0 + P < HW ? p0 + P : HW;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long p = p0 + threadIdx.x; p < p1; p += 256) {
        const double u = (double)px[p], v = (double)py[p];
        s[0] = s[0] + u;
        s[1] = s[1] + v;
        s[2] = s[2] + u * u;
        s[3] = s[3] + v * v;
        s[4] = s[4] + u * v;
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        s[q] = wave_sum(s[q]);
        if (lane == 0) red[wave][q] = s[q];
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        const int q = threadIdx.x;
        part[(((size_t)b * nruns + run) * 5 + q) * 3 + c] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
    }
}

// part[pair][nruns][n5] -> sums[pair][n5] (n5 = 5 C), the runs added in index order
__global__ __launch_bounds__(256) void dists_reduce_kernel(const double *__restrict__ part, int nruns, int n5, double *__restrict__ sums)
{
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= n5) return;
    const double *p = part + (size_t)b * nruns * n5 + i;
    double s = p[0];
    for (int k = 1; k < nruns; ++k) s = s + p[(size_t)k * n5];
    sums[(size_t)b * n5 + i] = s;
}

struct FinalizeArgs {
    long long off[DS_NMAPS];      // first sum of map k (doubles): maps back to back, each [B][5][C_k]
    double n[DS_NMAPS];           // pixels of map k
    double w;                     // sum(alpha) + sum(beta)
};

// channels of map k, as selects: a table indexed by a register would live in scratch memory
__device__ __forceinline__ int map_channels(int k) { return k == 0 ? 3 : (k == 1 ? 64 : (k == 2 ? 128 : (k == 3 ? 256 : 512))); }

__global__ __launch_bounds__(256) void dists_finalize_kernel(const double *__restrict__ sums, FinalizeArgs a, const float *__restrict__ alpha,
                                                             const float *__restrict__ beta, double *__restrict__ scores,
                                                             double *__restrict__ terms)
{
    __shared__ double t1[DS_CTOTAL], t2[DS_CTOTAL];      // alpha S1 and beta S2 of every channel, then summed in channel order
    __shared__ double mt[DS_NMAPS][2];
    const int b = blockIdx.x, t = threadIdx.x;
    const double c1 = 1e-6, c2 = 1e-6;
    int coff = 0;
    for (int k = 0; k < DS_NMAPS; ++k) {
        const int C = map_channels(k);
        const double *s = sums + a.off[k] + (size_t)b * 5 * C;
        const double n = a.n[k];
        for (int c = t; c < C; c += 256) {
            const double mx = s[c] / n, my = s[C + c] / n;
            const double vx = s[2 * C + c] / n - mx * mx, vy = s[3 * C + c] / n - my * my;
            const double cov = s[4 * C + c] / n - mx * my;
            const double S1 = (2.0 * mx * my + c1) / (mx * mx + my * my + c1);
            const double S2 = (2.0 * cov + c2) / (vx + vy + c2);
            t1[coff + c] = (double)alpha[coff + c] * S1;
            t2[coff + c] = (double)beta[coff + c] * S2;
        }
        coff += C;
    }
    __syncthreads();
    if (t < 2 * DS_NMAPS) {
        const int k = t >> 1;
        const int c0 = k == 0 ? 0 : (k == 1 ? 3 : (k == 2 ? 67 : (k == 3 ? 195 : (k == 4 ? 451 : 963)))), C = map_channels(k);
        const double *src = (t & 1) ? t2 : t1;
        double acc = 0.0;
        for (int c = 0; c < C; ++c) acc = acc + src[c0 + c];
        mt[k][t & 1] = acc;
    }
    __syncthreads();
    if (t == 0) {
        double total = 0.0;
        for (int k = 0; k < DS_NMAPS; ++k) {
            total = total + (mt[k][0] + mt[k][1]);
            if (terms) {
                terms[((size_t)b * DS_NMAPS + k) * 2] = mt[k][0];
                terms[((size_t)b * DS_NMAPS + k) * 2 + 1] = mt[k][1];
            }
        }
        scores[b] = 1.0 - total / a.w;
    }
}

unsigned grid_1d(size_t n)
{
    size_t g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

// torchvision `features` indices under the DISTS module's stage names
struct DsConv {
    const char *key;
    int cin, cout;
    int stage;      // 1..5
    int last;       // the stage's last conv: its ReLU output is feature map `stage`
};
const DsConv kConvs[DS_NCONV] = {
    {"stage1.0", 3, 64, 1, 0},     {"stage1.2", 64, 64, 1, 1},
    {"stage2.5", 64, 128, 2, 0},   {"stage2.7", 128, 128, 2, 1},
    {"stage3.10", 128, 256, 3, 0}, {"stage3.12", 256, 256, 3, 0}, {"stage3.14", 256, 256, 3, 1},
    {"stage4.17", 256, 512, 4, 0}, {"stage4.19", 512, 512, 4, 0}, {"stage4.21", 512, 512, 4, 1},
    {"stage5.24", 512, 512, 5, 0}, {"stage5.26", 512, 512, 5, 0}, {"stage5.28", 512, 512, 5, 1},
};

int pool_out(int n) { return (n + 1) / 2; }
size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// pixels per run of a map of hw pixels: a function of hw alone
int run_pixels(long long hw, int min_run)
{
    const long long p = (hw + DS_MAX_RUNS - 1) / DS_MAX_RUNS;
    return (int)(p < min_run ? min_run : p);
}
int run_count(long long hw, int min_run) { const int p = run_pixels(hw, min_run); return (int)((hw + p - 1) / p); }

size_t moments_ws_bytes(int B, long long hw, int C)
{
    return align256((size_t)B * run_count(hw, C == 3 ? DS_MIN_RUN_INPUT : DS_MIN_RUN) * 5 * C * sizeof(double));
}

int l2pool_launch(hipStream_t s, const float *f, int B2, int H, int W, int C, float *out)
{
    FEMASR_REQUIRE(f && out, "dists_l2pool: null pointer");
    FEMASR_REQUIRE(B2 >= 1 && H >= 1 && W >= 1, "dists_l2pool: empty shape B2=%d H=%d W=%d", B2, H, W);
    FEMASR_REQUIRE(C >= 64 && C <= 512 && (C % 64) == 0, "dists_l2pool: C = %d must be a multiple of 64 in 64..512", C);
    FEMASR_REQUIRE((long long)B2 * H * W * C < (1ll << 31), "dists_l2pool: tensor reaches 2^31 elements");
    const int Hp = pool_out(H), Wp = pool_out(W);
    const long long items = (long long)B2 * Hp * Wp * (C / 64);
    const long long blocks = (items + 3) / 4;
    hipLaunchKernelGGL(dists_l2pool_kernel, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(256), 0, s, f, (long long)B2, H, W, C, Hp,
                       Wp, out);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

int reduce_launch(hipStream_t s, const double *part, int B, int nruns, int C, double *sums)
{
    hipLaunchKernelGGL(dists_reduce_kernel, dim3((unsigned)((5 * C + 255) / 256), (unsigned)B), dim3(256), 0, s, part, nruns, 5 * C, sums);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

int moments_check(const void *f, int B, int H, int W, const void *ws, size_t ws_bytes, const void *sums, int C, const char *what)
{
    FEMASR_REQUIRE(f && ws && sums, "%s: null pointer", what);
    FEMASR_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: empty shape B=%d H=%d W=%d", what, B, H, W);
    FEMASR_REQUIRE(B <= DS_MAX_PAIRS, "%s: B = %d pairs per call exceeds %d (split the batch)", what, B, DS_MAX_PAIRS);
    FEMASR_REQUIRE(2ll * B * H * W * C < (1ll << 31), "%s: tensor reaches 2^31 elements", what);
    FEMASR_REQUIRE(((uintptr_t)ws & 255) == 0, "%s: workspace must be 256-byte aligned", what);
    FEMASR_REQUIRE(ws_bytes >= moments_ws_bytes(B, (long long)H * W, C), "%s: workspace %zu bytes < %zu needed", what, ws_bytes,
                   moments_ws_bytes(B, (long long)H * W, C));
    return FEMASR_OK;
}

// f (2B,H,W,C) NHWC -> sums [B][5][C]; `part` holds moments_ws_bytes
int moments_launch(hipStream_t s, const float *f, int B, int H, int W, int C, double *part, double *sums)
{
    const long long hw = (long long)H * W;
    const int P = run_pixels(hw, DS_MIN_RUN), nruns = run_count(hw, DS_MIN_RUN);
    hipLaunchKernelGGL(dists_moments_kernel, dim3((unsigned)nruns, (unsigned)(C / 64), (unsigned)B), dim3(64), 0, s, f, B, hw, C, P, part);
    FEMASR_CHECK_HIP(hipGetLastError());
    return reduce_launch(s, part, B, nruns, C, sums);
}

int moments_input_launch(hipStream_t s, const float *x, const float *y, int B, int H, int W, double *part, double *sums)
{
    const long long hw = (long long)H * W;
    const int P = run_pixels(hw, DS_MIN_RUN_INPUT), nruns = run_count(hw, DS_MIN_RUN_INPUT);
    hipLaunchKernelGGL(dists_moments_input_kernel, dim3((unsigned)nruns, 3u, (unsigned)B), dim3(256), 0, s, x, y, hw, P, part);
    FEMASR_CHECK_HIP(hipGetLastError());
    return reduce_launch(s, part, B, nruns, 3, sums);
}

}  // namespace

struct femasr_dists_handle {
    int device = 0;
    float *w[DS_NCONV] = {}, *bias[DS_NCONV] = {};
    bool wset[DS_NCONV] = {}, bset[DS_NCONV] = {};
    float *ab[2] = {};                     // alpha, beta on the device
    std::vector<float> ab_host[2];         // and on the host, for w = sum(alpha) + sum(beta)
    bool abset[2] = {};
    double wsum = 0.0;
    bool finalized = false;
};

namespace {

struct DsPlan {
    int h[DS_NMAPS], w[DS_NMAPS];          // map sizes (map 0: the input)
    size_t max_elems_per_image;            // largest NHWC tensor of one image (floats)
};

void make_plan(int H, int W, DsPlan *pl)
{
    pl->h[0] = pl->h[1] = H;
    pl->w[0] = pl->w[1] = W;
    for (int k = 2; k < DS_NMAPS; ++k) {
        pl->h[k] = pool_out(pl->h[k - 1]);
        pl->w[k] = pool_out(pl->w[k - 1]);
    }
    pl->max_elems_per_image = 0;
    for (int k = 1; k < DS_NMAPS; ++k) {
        const size_t e = (size_t)pl->h[k] * pl->w[k] * kMapC[k];
        if (e > pl->max_elems_per_image) pl->max_elems_per_image = e;
    }
}

int check_shape(int B, int H, int W, DsPlan *pl)
{
    FEMASR_REQUIRE(B >= 1 && H >= 1 && W >= 1, "dists: empty shape B=%d H=%d W=%d", B, H, W);
    FEMASR_REQUIRE(H >= DS_MIN_SIDE && W >= DS_MIN_SIDE, "dists: needs H, W >= %d, got %dx%d", DS_MIN_SIDE, H, W);
    FEMASR_REQUIRE(B <= DS_MAX_PAIRS, "dists: B = %d pairs per call exceeds %d (split the batch)", B, DS_MAX_PAIRS);
    make_plan(H, W, pl);
    FEMASR_REQUIRE(2 * (long long)B * (long long)pl->max_elems_per_image < (1ll << 31),
                   "dists: a feature tensor of 2B=%d images at %dx%d reaches 2^31 elements (split the batch)", 2 * B, H, W);
    return FEMASR_OK;
}

// workspace: [input 2B x H x W x 3][feature buffer A][feature buffer B][partials of one map][sums of the 6 maps]
struct WsLayout {
    size_t in_off, a_off, b_off, part_off, sums_off, total;
    long long sums_off_map[DS_NMAPS];
};

WsLayout layout(const DsPlan &pl, int B, int H, int W)
{
    WsLayout L{};
    L.in_off = 0;
    L.a_off = align256(L.in_off + 2 * (size_t)B * H * W * 3 * sizeof(float));
    L.b_off = align256(L.a_off + 2 * (size_t)B * pl.max_elems_per_image * sizeof(float));
    L.part_off = align256(L.b_off + 2 * (size_t)B * pl.max_elems_per_image * sizeof(float));
    size_t pmax = 0;
    long long n = 0;
    for (int k = 0; k < DS_NMAPS; ++k) {
        const size_t pb = moments_ws_bytes(B, (long long)pl.h[k] * pl.w[k], kMapC[k]);
        if (pb > pmax) pmax = pb;
        L.sums_off_map[k] = n;
        n += (long long)B * 5 * kMapC[k];
    }
    L.sums_off = L.part_off + pmax;
    L.total = align256(L.sums_off + (size_t)n * sizeof(double));
    return L;
}

int forward_check(const femasr_dists_handle *h, const void *x, const void *y, int B, int H, int W, const void *ws, size_t ws_bytes,
                  const void *out, DsPlan *pl, WsLayout *L, const char *what)
{
    FEMASR_REQUIRE(h && x && y && ws && out, "%s: null argument", what);
    FEMASR_CHECK(check_shape(B, H, W, pl));
    FEMASR_REQUIRE(((uintptr_t)ws & 255) == 0, "%s: workspace must be 256-byte aligned", what);
    *L = layout(*pl, B, H, W);
    FEMASR_REQUIRE(ws_bytes >= L->total, "%s: workspace %zu bytes < %zu needed", what, ws_bytes, L->total);
    FEMASR_REQUIRE(h->finalized, "%s: weights not finalized (femasr_dists_finalize_weights)", what);
    return FEMASR_OK;
}

// the backbone and, with scores, the head; with feats, a copy of the five stage maps (NHWC, 2B images each, back to back)
int run(femasr_dists_handle *h, hipStream_t s, const float *x, const float *y, int B, int H, int W, const DsPlan &pl, const WsLayout &L, void *ws,
        double *scores, double *terms, float *feats)
{
    DeviceGuard guard(h->device);
    FEMASR_REQUIRE(guard.ok, "dists: hipSetDevice(%d) failed", h->device);
    char *base = (char *)ws;
    float *X = (float *)(base + L.in_off), *bufA = (float *)(base + L.a_off), *bufB = (float *)(base + L.b_off);
    double *part = (double *)(base + L.part_off), *sums = (double *)(base + L.sums_off);
    const int B2 = 2 * B;
    hipLaunchKernelGGL(dists_input_kernel, dim3(grid_1d((size_t)B2 * H * W)), dim3(256), 0, s, x, y, B, H, W, X);
    FEMASR_CHECK_HIP(hipGetLastError());
    if (scores) FEMASR_CHECK(moments_input_launch(s, x, y, B, H, W, part, sums + L.sums_off_map[0]));
    const float *cur = X;
    for (int i = 0; i < DS_NCONV; ++i) {
        const DsConv &c = kConvs[i];
        const int ch = pl.h[c.stage], cw = pl.w[c.stage];
        float *dst = cur == bufA ? bufB : bufA;
        femasr_conv_args a{};
        a.in = cur; a.B = B2; a.H = ch; a.W = cw; a.Cin = c.cin;
        a.w = h->w[i]; a.bias = h->bias[i];
        a.Cout = c.cout; a.ksz = 3; a.stride = 1; a.pad = 1; a.up2 = 0;
        a.prologue = FEMASR_PRO_NONE; a.act = FEMASR_ACT_RELU;
        a.out = dst; a.Ho = ch; a.Wo = cw;
        FEMASR_CHECK(femasr_conv2d_launch(s, &a, nullptr, nullptr, nullptr));
        cur = dst;
        if (!c.last) continue;
        if (feats) {
            const size_t n = (size_t)B2 * ch * cw * c.cout;
            FEMASR_CHECK_HIP(hipMemcpyAsync(feats, cur, n * sizeof(float), hipMemcpyDeviceToDevice, s));
            feats += n;
        }
        if (scores) FEMASR_CHECK(moments_launch(s, cur, B, ch, cw, c.cout, part, sums + L.sums_off_map[c.stage]));
        if (c.stage < DS_NSTAGES) {
            float *pooled = cur == bufA ? bufB : bufA;
            FEMASR_CHECK(l2pool_launch(s, cur, B2, ch, cw, c.cout, pooled));
            cur = pooled;
        }
    }
    if (!scores) return FEMASR_OK;
    FinalizeArgs fa{};
    for (int k = 0; k < DS_NMAPS; ++k) {
        fa.off[k] = L.sums_off_map[k];
        fa.n[k] = (double)pl.h[k] * (double)pl.w[k];
    }
    fa.w = h->wsum;
    hipLaunchKernelGGL(dists_finalize_kernel, dim3((unsigned)B), dim3(256), 0, s, sums, fa, h->ab[0], h->ab[1], scores, terms);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

}  // namespace

extern "C" {

int femasr_dists_create(int device, femasr_dists_handle **out)
{
    FEMASR_REQUIRE(out, "dists_create: null out");
    FEMASR_REQUIRE(device >= 0, "dists_create: device %d", device);      // the device is first touched by set_weight
    femasr_dists_handle *h = new femasr_dists_handle;
    h->device = device;
    *out = h;
    return FEMASR_OK;
}

void femasr_dists_destroy(femasr_dists_handle *h)
{
    if (!h) return;
    DeviceGuard guard(h->device);
    for (float *p : h->w) if (p) (void)hipFree(p);
    for (float *p : h->bias) if (p) (void)hipFree(p);
    for (float *p : h->ab) if (p) (void)hipFree(p);
    delete h;
}

int femasr_dists_set_weight(femasr_dists_handle *h, const char *key, const float *dev_ptr, const int64_t *shape, int ndim)
{
    FEMASR_REQUIRE(h && key && dev_ptr && shape, "dists_set_weight: null argument");
    const std::string k(key);
    DeviceGuard guard(h->device);
    FEMASR_REQUIRE(guard.ok, "dists_set_weight: hipSetDevice(%d) failed", h->device);
    for (int e = 0; e < 2; ++e) {
        if (k != (e ? "beta" : "alpha")) continue;
        if (!(ndim == 4 && shape[0] == 1 && shape[1] == DS_CTOTAL && shape[2] == 1 && shape[3] == 1))
            return femasr_set_error(FEMASR_ERR_WEIGHT, "dists_set_weight: '%s' must be (1, %d, 1, 1)", key, DS_CTOTAL);
        if (!h->ab[e]) FEMASR_CHECK_HIP(hipMalloc((void **)&h->ab[e], DS_CTOTAL * sizeof(float)));
        h->ab_host[e].assign(DS_CTOTAL, 0.f);
        FEMASR_CHECK_HIP(hipMemcpyAsync(h->ab[e], dev_ptr, DS_CTOTAL * sizeof(float), hipMemcpyDeviceToDevice, nullptr));
        FEMASR_CHECK_HIP(hipMemcpyAsync(h->ab_host[e].data(), dev_ptr, DS_CTOTAL * sizeof(float), hipMemcpyDeviceToHost, nullptr));
        FEMASR_CHECK_HIP(hipStreamSynchronize(nullptr));
        h->abset[e] = true;
        h->finalized = false;
        return FEMASR_OK;
    }
    for (int i = 0; i < DS_NCONV; ++i) {
        const DsConv &c = kConvs[i];
        const std::string pre(c.key);
        if (k == pre + ".weight") {
            if (!(ndim == 4 && shape[0] == c.cout && shape[1] == c.cin && shape[2] == 3 && shape[3] == 3))
                return femasr_set_error(FEMASR_ERR_WEIGHT, "dists_set_weight: '%s' must be (%d, %d, 3, 3)", key, c.cout, c.cin);
            if (!h->w[i]) FEMASR_CHECK_HIP(hipMalloc((void **)&h->w[i], femasr_packed_weight_floats(c.cout, c.cin, 3, 3) * sizeof(float)));
            const int rc = femasr_repack_oihw(nullptr, dev_ptr, c.cout, c.cin, 3, 3, h->w[i]);
            if (rc) return rc;
            FEMASR_CHECK_HIP(hipStreamSynchronize(nullptr));
            h->wset[i] = true;
            h->finalized = false;
            return FEMASR_OK;
        }
        if (k == pre + ".bias") {
            if (!(ndim == 1 && shape[0] == c.cout))
                return femasr_set_error(FEMASR_ERR_WEIGHT, "dists_set_weight: '%s' must be (%d,)", key, c.cout);
            if (!h->bias[i]) FEMASR_CHECK_HIP(hipMalloc((void **)&h->bias[i], (size_t)c.cout * sizeof(float)));
            FEMASR_CHECK_HIP(hipMemcpyAsync(h->bias[i], dev_ptr, (size_t)c.cout * sizeof(float), hipMemcpyDeviceToDevice, nullptr));
            FEMASR_CHECK_HIP(hipStreamSynchronize(nullptr));
            h->bset[i] = true;
            h->finalized = false;
            return FEMASR_OK;
        }
    }
    return femasr_set_error(FEMASR_ERR_WEIGHT, "dists_set_weight: unknown key '%s'", key);
}

int femasr_dists_finalize_weights(femasr_dists_handle *h)
{
    FEMASR_REQUIRE(h, "dists_finalize_weights: null handle");
    for (int i = 0; i < DS_NCONV; ++i) {
        if (!h->wset[i]) return femasr_set_error(FEMASR_ERR_WEIGHT, "dists_finalize_weights: '%s.weight' was never set", kConvs[i].key);
        if (!h->bset[i]) return femasr_set_error(FEMASR_ERR_WEIGHT, "dists_finalize_weights: '%s.bias' was never set", kConvs[i].key);
    }
    for (int e = 0; e < 2; ++e)
        if (!h->abset[e]) return femasr_set_error(FEMASR_ERR_WEIGHT, "dists_finalize_weights: '%s' was never set", e ? "beta" : "alpha");
    double w = 0.0;      // fp64, index order, alpha then beta
    for (int e = 0; e < 2; ++e)
        for (int c = 0; c < DS_CTOTAL; ++c) w = w + (double)h->ab_host[e][c];
    h->wsum = w;
    h->finalized = true;
    return FEMASR_OK;
}

int femasr_dists_workspace_bytes(const femasr_dists_handle *h, int B, int H, int W, size_t *bytes)
{
    FEMASR_REQUIRE(h && bytes, "dists_workspace_bytes: null argument");
    DsPlan pl;
    FEMASR_CHECK(check_shape(B, H, W, &pl));
    *bytes = layout(pl, B, H, W).total;
    return FEMASR_OK;
}

int femasr_dists_forward(femasr_dists_handle *h, void *stream, const float *x_nchw, const float *y_nchw, int B, int H, int W, void *ws,
                         size_t ws_bytes, double *scores, double *terms)
{
    DsPlan pl;
    WsLayout L;
    FEMASR_CHECK(forward_check(h, x_nchw, y_nchw, B, H, W, ws, ws_bytes, scores, &pl, &L, "dists_forward"));
    return run(h, (hipStream_t)stream, x_nchw, y_nchw, B, H, W, pl, L, ws, scores, terms, nullptr);
}

int femasr_dists_features(femasr_dists_handle *h, void *stream, const float *x_nchw, const float *y_nchw, int B, int H, int W, void *ws,
                          size_t ws_bytes, float *features)
{
    DsPlan pl;
    WsLayout L;
    FEMASR_CHECK(forward_check(h, x_nchw, y_nchw, B, H, W, ws, ws_bytes, features, &pl, &L, "dists_features"));
    return run(h, (hipStream_t)stream, x_nchw, y_nchw, B, H, W, pl, L, ws, nullptr, nullptr, features);
}

int femasr_dists_l2pool(void *stream, const float *f, int B2, int H, int W, int C, float *out)
{
    return l2pool_launch((hipStream_t)stream, f, B2, H, W, C, out);
}

int femasr_dists_moments_workspace_bytes(int B, int H, int W, int C, size_t *bytes)
{
    FEMASR_REQUIRE(bytes, "dists_moments_workspace_bytes: null argument");
    FEMASR_REQUIRE(B >= 1 && H >= 1 && W >= 1, "dists_moments_workspace_bytes: empty shape B=%d H=%d W=%d", B, H, W);
    FEMASR_REQUIRE(B <= DS_MAX_PAIRS, "dists_moments_workspace_bytes: B = %d pairs per call exceeds %d", B, DS_MAX_PAIRS);
    FEMASR_REQUIRE(C == 3 || (C >= 64 && C <= 512 && (C % 64) == 0), "dists_moments_workspace_bytes: C = %d must be 3 or a multiple of 64 in 64..512", C);
    *bytes = moments_ws_bytes(B, (long long)H * W, C);
    return FEMASR_OK;
}

int femasr_dists_moments(void *stream, const float *f, int B, int H, int W, int C, void *ws, size_t ws_bytes, double *sums)
{
    FEMASR_REQUIRE(C >= 64 && C <= 512 && (C % 64) == 0, "dists_moments: C = %d must be a multiple of 64 in 64..512", C);
    FEMASR_CHECK(moments_check(f, B, H, W, ws, ws_bytes, sums, C, "dists_moments"));
    return moments_launch((hipStream_t)stream, f, B, H, W, C, (double *)ws, sums);
}

int femasr_dists_moments_input(void *stream, const float *x_nchw, const float *y_nchw, int B, int H, int W, void *ws, size_t ws_bytes,
                               double *sums)
{
    FEMASR_REQUIRE(y_nchw, "dists_moments_input: null pointer");
    FEMASR_CHECK(moments_check(x_nchw, B, H, W, ws, ws_bytes, sums, 3, "dists_moments_input"));
    return moments_input_launch((hipStream_t)stream, x_nchw, y_nchw, B, H, W, (double *)ws, sums);
}

}  // extern "C"

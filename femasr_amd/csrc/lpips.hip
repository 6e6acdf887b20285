// lpips.hip — LPIPS v0.1 (inference) on gfx950: the perceptual metric the reference validates with (pyiqa 'lpips' = AlexNet
// backbone, 'lpips-vgg' = VGG16; options/train_FeMaSR_LQ_stage.yml key_metric, basicsr/models/femasr_model.py:27-34,262).
//
// Schedule of one femasr_lpips_forward (x0, x1: (B,3,H,W) fp32 NCHW in [0,1]):
//   lpips_input_kernel   both images -> ONE NHWC batch of 2B images (x0 in samples 0..B-1, x1 in B..2B-1) with the input
//                        scaling fused: t = 2x - 1, then (t - shift) / scale (fp32, IEEE division)
//   backbone convs       femasr_conv2d_launch with act = FEMASR_ACT_RELU on the direct fp32 forms (kernels_conv.hip): Cin = 3
//                        -> generic implicit GEMM, AlexNet's 5x5 -> vectorised implicit GEMM, every 3x3 with Cin % 32 == 0 ->
//                        halo kernel.  Each output is one fmaf chain in the oracle's K order (bit-identical to oracle.conv2d).
//   lpips_tap_kernel     after each tapped conv: per pixel of sample b the head value of the pair (f[b], f[b+B]) in fp32,
//                        one fp64 partial per (sample, 32-pixel block); where a max-pool follows the tap the SAME launch (other blocks' role)
//                        writes the pooled map (every pool of both nets follows a tap)
//   lpips_finalize_kernel  per sample: the partials of each tap summed in a fixed order, mean over the tap's H x W, the
//                        five terms summed in tap order in fp32
// Reduction order (no atomics): per pixel, per lane over its channels (c = lane + 64 j, j ascending), then a 64-lane xor
// butterfly (offsets 32, 16, .., 1; every lane ends with the same bits); per wave over its 8 pixels in ascending order (fp64);
// per block the four waves in order; per sample in finalize, thread t over partials t, t + 256, .. then an LDS tree.  Every
// sum depends only on the pair's own pixels and on (H, W, C): results are run-to-run deterministic and batch-invariant.
#include "common.h"
#include <string>
#include <vector>

namespace {

constexpr int LP_NTAPS = 5;
constexpr int TAP_THREADS = 256;
constexpr int TAP_PIX = 32;                  // head pixels per block (8 per wave): a 1-pair launch of a small tap still fills the CUs
constexpr int POOL_PIX = 16;                 // pooled pixels per block (4 per wave)
constexpr int TAP_MAX_PAIRS = 65535;         // gridDim.y limit: pairs per launch
constexpr int TAP_MAXJ = 8;                  // C <= 512, C % 64 == 0

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

__global__ __launch_bounds__(256) void lpips_input_kernel(const float *__restrict__ x0, const float *__restrict__ x1, int B, int H, int W,
                                                          float *__restrict__ out)
{
    const size_t HW = (size_t)H * W, total = 2 * (size_t)B * HW;
    const float shift[3] = {(float)-.030, (float)-.088, (float)-.188};
    const float scale[3] = {(float).458, (float).448, (float).450};
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t s = i / HW, p = i - s * HW;
        const float *src = s < (size_t)B ? x0 + s * 3 * HW : x1 + (s - B) * 3 * HW;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float t = 2.f * src[c * HW + p] - 1.f;
            out[i * 3 + c] = (t - shift[c]) / scale[c];
        }
    }
}

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

// max over the K x K window at src (row pitch W*C floats) of channel c; max_pool2d semantics: NaN propagates
template <int K>
__device__ __forceinline__ float window_max(const float *src, size_t rowp, int C, int c)
{
    float v[K * K];
#pragma unroll
    for (int ky = 0; ky < K; ++ky)
#pragma unroll
        for (int kx = 0; kx < K; ++kx) v[ky * K + kx] = src[ky * rowp + (size_t)kx * C + c];      // all loads in flight together
    float m = v[0];
#pragma unroll
    for (int i = 1; i < K * K; ++i) m = (v[i] > m || v[i] != v[i]) ? v[i] : m;
    return m;
}

// f: (2B,H,W,C) NHWC.  part[b][blockIdx.x] for blockIdx.x < nblk.  pool 1: 3x3 stride 2, pool 2: 2x2 stride 2 (no padding,
// floor) into pooled (2B,Hp,Wp,C).  One launch, two block roles: blocks < nblk evaluate the head of 32 pixels, blocks < npblk
// (the same blocks, over a different pixel range) pool 16 output pixels; the map is read once for the head and once more (through
// L2) for the pool windows.
__global__ __launch_bounds__(TAP_THREADS) void lpips_tap_kernel(const float *__restrict__ f, int B, int H, int W, int C,
                                                                 const float *__restrict__ wl, int pool, float *__restrict__ pooled,
                                                                 int Hp, int Wp, double *__restrict__ part, int nblk, int npblk)
{
    __shared__ double red[TAP_THREADS / 64];
    const int b = blockIdx.y, blk = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nj = C >> 6;
    const long long HW = (long long)H * W;
    if (blk < nblk) {      // (uniform) head
        float wr[TAP_MAXJ];
#pragma unroll
        for (int j = 0; j < TAP_MAXJ; ++j) wr[j] = j < nj ? wl[lane + 64 * j] : 0.f;
        const float *f0 = f + (size_t)b * HW * C, *f1 = f + (size_t)(b + B) * HW * C;
        double acc = 0.0;
        const long long p0 = (long long)blk * TAP_PIX + wave * (TAP_PIX / 4);
        for (int i = 0; i < TAP_PIX / 4; ++i) {
            const long long p = p0 + i;
            if (p >= HW) break;     // (uniform)
            float a[TAP_MAXJ], c[TAP_MAXJ];
#pragma unroll
            for (int j = 0; j < TAP_MAXJ; ++j) {
                a[j] = j < nj ? f0[p * C + lane + 64 * j] : 0.f;
                c[j] = j < nj ? f1[p * C + lane + 64 * j] : 0.f;
            }
            float s0 = 0.f, s1 = 0.f;
#pragma unroll
            for (int j = 0; j < TAP_MAXJ; ++j) {
                if (j < nj) {
                    s0 = __builtin_fmaf(a[j], a[j], s0);
                    s1 = __builtin_fmaf(c[j], c[j], s1);
                }
            }
            s0 = wave_sum(s0);
            s1 = wave_sum(s1);
            const float r0 = __builtin_sqrtf(s0) + 1e-10f, r1 = __builtin_sqrtf(s1) + 1e-10f;     // normalize_tensor: f / (|f| + eps)
            float d = 0.f;
#pragma unroll
            for (int j = 0; j < TAP_MAXJ; ++j) {
                if (j < nj) {
                    const float t = a[j] / r0 - c[j] / r1;
                    d = __builtin_fmaf(wr[j], t * t, d);
                }
            }
            acc = acc + (double)wave_sum(d);
        }
        if (lane == 0) red[wave] = acc;
        __syncthreads();
        if (threadIdx.x == 0) part[(size_t)b * nblk + blk] = ((red[0] + red[1]) + red[2]) + red[3];
    }
    if (pool && blk < npblk) {      // (uniform) pooled map of both samples of the pair
        const long long HWp = (long long)Hp * Wp;
        for (int i = 0; i < POOL_PIX / 4; ++i) {
            const long long q = (long long)blk * POOL_PIX + wave * (POOL_PIX / 4) + i;
            if (q >= HWp) break;
            const int oy = (int)(q / Wp), ox = (int)(q - (long long)oy * Wp);
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int s = b + e * B;
                const float *src = f + (((size_t)s * H + 2 * oy) * W + 2 * ox) * C;
                float *dst = pooled + ((size_t)s * HWp + q) * C;
                const size_t rowp = (size_t)W * C;
                for (int j = 0; j < nj; ++j) {
                    const int c = lane + 64 * j;
                    dst[c] = pool == 1 ? window_max<3>(src, rowp, C, c) : window_max<2>(src, rowp, C, c);
                }
            }
        }
    }
}

struct FinalizeArgs {
    long long off[LP_NTAPS];     // first partial of tap k (doubles): taps back to back, each [B][nblk_k]
    int nblk[LP_NTAPS];
    double hw[LP_NTAPS];
    int ntaps, B;
};

__global__ __launch_bounds__(256) void lpips_finalize_kernel(const double *__restrict__ part, FinalizeArgs a, float *__restrict__ out,
                                                             float *__restrict__ per_layer)
{
    __shared__ double red[256];
    const int b = blockIdx.x, t = threadIdx.x;
    float total = 0.f;
    for (int k = 0; k < a.ntaps; ++k) {
        const double *pk = part + a.off[k] + (size_t)b * a.nblk[k];
        double s = 0.0;
        for (int i = t; i < a.nblk[k]; i += 256) s = s + pk[i];
        red[t] = s;
        __syncthreads();
        for (int w = 128; w >= 1; w >>= 1) {
            if (t < w) red[t] = red[t] + red[t + w];
            __syncthreads();
        }
        const float term = (float)(red[0] / a.hw[k]);
        total = k == 0 ? term : total + term;
        if (t == 0 && per_layer) per_layer[(size_t)b * a.ntaps + k] = term;
        __syncthreads();
    }
    if (t == 0) out[b] = total;
}

unsigned grid_1d(size_t n)
{
    size_t g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

// ---- the two backbones (torchvision `features` indices; lpips / pyiqa slice names)
struct LpConv {
    const char *key;     // canonical weight prefix
    int cin, cout, ksz, stride, pad;
    int tap;             // 0: none, else the tap (1..5) this conv's ReLU output is
    int pool;            // after the tap: 0 none, 1 maxpool 3/2, 2 maxpool 2/2
};
const LpConv kAlex[] = {
    {"net.slice1.0", 3, 64, 11, 4, 2, 1, 1},
    {"net.slice2.3", 64, 192, 5, 1, 2, 2, 1},
    {"net.slice3.6", 192, 384, 3, 1, 1, 3, 0},
    {"net.slice4.8", 384, 256, 3, 1, 1, 4, 0},
    {"net.slice5.10", 256, 256, 3, 1, 1, 5, 0},
};
const LpConv kVgg[] = {
    {"net.slice1.0", 3, 64, 3, 1, 1, 0, 0},      {"net.slice1.2", 64, 64, 3, 1, 1, 1, 2},
    {"net.slice2.5", 64, 128, 3, 1, 1, 0, 0},    {"net.slice2.7", 128, 128, 3, 1, 1, 2, 2},
    {"net.slice3.10", 128, 256, 3, 1, 1, 0, 0},  {"net.slice3.12", 256, 256, 3, 1, 1, 0, 0},  {"net.slice3.14", 256, 256, 3, 1, 1, 3, 2},
    {"net.slice4.17", 256, 512, 3, 1, 1, 0, 0},  {"net.slice4.19", 512, 512, 3, 1, 1, 0, 0},  {"net.slice4.21", 512, 512, 3, 1, 1, 4, 2},
    {"net.slice5.24", 512, 512, 3, 1, 1, 0, 0},  {"net.slice5.26", 512, 512, 3, 1, 1, 0, 0},  {"net.slice5.28", 512, 512, 3, 1, 1, 5, 0},
};

const int kAlexLin[LP_NTAPS] = {64, 192, 384, 256, 256}, kVggLin[LP_NTAPS] = {64, 128, 256, 512, 512};      // channels of the taps

// output size of max_pool2d without padding (floor; 0 when the window does not fit - C++ division truncates toward 0, so test first)
int pool_out(int n, int pool) { return pool == 1 ? (n < 3 ? 0 : (n - 3) / 2 + 1) : n / 2; }

// Shapes of one forward at (H, W): per conv its output size, per tap its size; false if a pool would have no output.
struct LpPlan {
    int n = 0;
    int ho[13], wo[13];
    int tap_h[LP_NTAPS], tap_w[LP_NTAPS], tap_c[LP_NTAPS];
    size_t max_elems_per_image = 0;      // largest NHWC tensor of one image (floats)
};

}  // namespace

struct femasr_lpips_handle {
    int net = 0, device = 0;
    const LpConv *convs = nullptr;
    int nconv = 0;
    std::vector<float *> w, bias;
    std::vector<bool> wset, bset;
    float *lin[LP_NTAPS] = {};
    bool linset[LP_NTAPS] = {};
    bool finalized = false;
};

namespace {

bool make_plan(const femasr_lpips_handle *h, int H, int W, LpPlan *pl)
{
    pl->n = h->nconv;
    int y = H, x = W;
    pl->max_elems_per_image = (size_t)H * W * 3;
    for (int i = 0; i < h->nconv; ++i) {
        const LpConv &c = h->convs[i];
        y = (y + 2 * c.pad - c.ksz) / c.stride + 1;
        x = (x + 2 * c.pad - c.ksz) / c.stride + 1;
        if (y < 1 || x < 1) return false;
        pl->ho[i] = y;
        pl->wo[i] = x;
        const size_t e = (size_t)y * x * c.cout;
        if (e > pl->max_elems_per_image) pl->max_elems_per_image = e;
        if (c.tap) {
            pl->tap_h[c.tap - 1] = y;
            pl->tap_w[c.tap - 1] = x;
            pl->tap_c[c.tap - 1] = c.cout;
        }
        if (c.pool) {
            y = pool_out(y, c.pool);
            x = pool_out(x, c.pool);
            if (y < 1 || x < 1) return false;
        }
    }
    return true;
}

int min_side(int net) { return net == 0 ? 31 : 16; }

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// workspace: [input 2B x H x W x 3][feature buffer A][feature buffer B][partials of the 5 taps]
struct WsLayout {
    size_t in_off, a_off, b_off, part_off, total;
    long long part_off_tap[LP_NTAPS];
    int nblk[LP_NTAPS];
};

int check_shape(const femasr_lpips_handle *h, int B, int H, int W, LpPlan *pl)
{
    FEMASR_REQUIRE(B >= 1 && H >= 1 && W >= 1, "lpips: empty shape B=%d H=%d W=%d", B, H, W);
    FEMASR_REQUIRE(B <= TAP_MAX_PAIRS, "lpips: B = %d pairs per call exceeds %d (split the batch)", B, TAP_MAX_PAIRS);
    FEMASR_REQUIRE(H >= min_side(h->net) && W >= min_side(h->net),
                   "lpips: %s needs H, W >= %d (a max-pool of the backbone would have no output), got %dx%d",
                   h->net == 0 ? "alex" : "vgg16", min_side(h->net), H, W);
    FEMASR_REQUIRE(make_plan(h, H, W, pl), "lpips: %dx%d is too small for the backbone", H, W);
    FEMASR_REQUIRE(2 * (long long)B * (long long)pl->max_elems_per_image < (1ll << 31),
                   "lpips: a feature tensor of 2B=%d images at %dx%d reaches 2^31 elements (split the batch)", 2 * B, H, W);
    return FEMASR_OK;
}

WsLayout layout(const LpPlan &pl, int B, int H, int W)
{
    WsLayout L{};
    L.in_off = 0;
    L.a_off = align256(L.in_off + 2 * (size_t)B * H * W * 3 * sizeof(float));
    L.b_off = align256(L.a_off + 2 * (size_t)B * pl.max_elems_per_image * sizeof(float));
    L.part_off = align256(L.b_off + 2 * (size_t)B * pl.max_elems_per_image * sizeof(float));
    long long n = 0;
    for (int k = 0; k < LP_NTAPS; ++k) {
        L.nblk[k] = (int)(((long long)pl.tap_h[k] * pl.tap_w[k] + TAP_PIX - 1) / TAP_PIX);
        L.part_off_tap[k] = n;
        n += (long long)B * L.nblk[k];
    }
    L.total = align256(L.part_off + (size_t)n * sizeof(double));
    return L;
}

int tap_launch(hipStream_t s, const float *f, int B2, int H, int W, int C, const float *w_lin, int pool, float *pooled, double *partials)
{
    FEMASR_REQUIRE(f && w_lin && partials && B2 >= 2 && (B2 % 2) == 0 && H >= 1 && W >= 1,
                   "lpips_tap: null pointer or bad shape (B2 = %d must be an even pair count x 2)", B2);
    FEMASR_REQUIRE(B2 / 2 <= TAP_MAX_PAIRS, "lpips_tap: %d pairs per launch exceed %d", B2 / 2, TAP_MAX_PAIRS);
    FEMASR_REQUIRE(C >= 64 && C <= 64 * TAP_MAXJ && (C % 64) == 0, "lpips_tap: C = %d must be a multiple of 64 in 64..512", C);
    FEMASR_REQUIRE(pool >= 0 && pool <= 2 && (!pool || pooled), "lpips_tap: pool must be 0, 1 (3/2) or 2 (2/2), with pooled_out");
    FEMASR_REQUIRE((long long)B2 * H * W * C < (1ll << 31), "lpips_tap: tensor reaches 2^31 elements");
    const int Hp = pool ? pool_out(H, pool) : 0, Wp = pool ? pool_out(W, pool) : 0;
    FEMASR_REQUIRE(!pool || (Hp >= 1 && Wp >= 1), "lpips_tap: %dx%d is too small for the max-pool", H, W);
    const int B = B2 / 2;
    const long long HW = (long long)H * W;
    const int nblk = (int)((HW + TAP_PIX - 1) / TAP_PIX);
    const int npblk = pool ? (int)(((long long)Hp * Wp + POOL_PIX - 1) / POOL_PIX) : 0;
    const int gx = nblk > npblk ? nblk : npblk;
    hipLaunchKernelGGL(lpips_tap_kernel, dim3((unsigned)gx, (unsigned)B), dim3(TAP_THREADS), 0, s, f, B, H, W, C, w_lin, pool, pooled, Hp, Wp,
                       partials, nblk, npblk);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

int finalize_launch(hipStream_t s, const double *partials, int B, int ntaps, const int32_t *tap_hw, float *out, float *per_layer)
{
    FEMASR_REQUIRE(partials && tap_hw && out && B >= 1 && ntaps >= 1 && ntaps <= LP_NTAPS, "lpips_finalize: bad arguments");
    FinalizeArgs a{};
    a.ntaps = ntaps;
    a.B = B;
    long long off = 0;
    for (int k = 0; k < ntaps; ++k) {
        FEMASR_REQUIRE(tap_hw[2 * k] >= 1 && tap_hw[2 * k + 1] >= 1, "lpips_finalize: empty tap %d", k);
        const long long hw = (long long)tap_hw[2 * k] * tap_hw[2 * k + 1];
        a.nblk[k] = (int)((hw + TAP_PIX - 1) / TAP_PIX);
        a.hw[k] = (double)hw;
        a.off[k] = off;
        off += (long long)B * a.nblk[k];
    }
    hipLaunchKernelGGL(lpips_finalize_kernel, dim3((unsigned)B), dim3(256), 0, s, partials, a, out, per_layer);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

}  // namespace

extern "C" {

int femasr_lpips_create(int net, int device, femasr_lpips_handle **out)
{
    FEMASR_REQUIRE(out, "lpips_create: null out");
    FEMASR_REQUIRE(net == 0 || net == 1, "lpips_create: net must be 0 (alex) or 1 (vgg16), got %d", net);
    DeviceGuard guard(device);
    FEMASR_REQUIRE(guard.ok, "lpips_create: hipSetDevice(%d) failed", device);
    femasr_lpips_handle *h = new femasr_lpips_handle;
    h->net = net;
    h->device = device;
    h->convs = net == 0 ? kAlex : kVgg;
    h->nconv = net == 0 ? (int)(sizeof(kAlex) / sizeof(kAlex[0])) : (int)(sizeof(kVgg) / sizeof(kVgg[0]));
    h->w.assign(h->nconv, nullptr);
    h->bias.assign(h->nconv, nullptr);
    h->wset.assign(h->nconv, false);
    h->bset.assign(h->nconv, false);
    *out = h;
    return FEMASR_OK;
}

void femasr_lpips_destroy(femasr_lpips_handle *h)
{
    if (!h) return;
    DeviceGuard guard(h->device);
    for (float *p : h->w) if (p) (void)hipFree(p);
    for (float *p : h->bias) if (p) (void)hipFree(p);
    for (float *p : h->lin) if (p) (void)hipFree(p);
    delete h;
}

int femasr_lpips_set_weight(femasr_lpips_handle *h, const char *key, const float *dev_ptr, const int64_t *shape, int ndim)
{
    FEMASR_REQUIRE(h && key && dev_ptr && shape, "lpips_set_weight: null argument");
    const std::string k(key);
    DeviceGuard guard(h->device);
    FEMASR_REQUIRE(guard.ok, "lpips_set_weight: hipSetDevice(%d) failed", h->device);
    for (int t = 0; t < LP_NTAPS; ++t) {
        if (k != "lin" + std::to_string(t) + ".model.1.weight") continue;
        const int C = (h->net == 0 ? kAlexLin : kVggLin)[t];
        if (!(ndim == 4 && shape[0] == 1 && shape[1] == C && shape[2] == 1 && shape[3] == 1))
            return femasr_set_error(FEMASR_ERR_WEIGHT, "lpips_set_weight: '%s' must be (1, %d, 1, 1)", key, C);
        if (!h->lin[t]) FEMASR_CHECK_HIP(hipMalloc((void **)&h->lin[t], (size_t)C * sizeof(float)));
        FEMASR_CHECK_HIP(hipMemcpyAsync(h->lin[t], dev_ptr, (size_t)C * sizeof(float), hipMemcpyDeviceToDevice, nullptr));
        FEMASR_CHECK_HIP(hipStreamSynchronize(nullptr));
        h->linset[t] = true;
        h->finalized = false;
        return FEMASR_OK;
    }
    for (int i = 0; i < h->nconv; ++i) {
        const LpConv &c = h->convs[i];
        const std::string pre(c.key);
        if (k == pre + ".weight") {
            if (!(ndim == 4 && shape[0] == c.cout && shape[1] == c.cin && shape[2] == c.ksz && shape[3] == c.ksz))
                return femasr_set_error(FEMASR_ERR_WEIGHT, "lpips_set_weight: '%s' must be (%d, %d, %d, %d)", key, c.cout, c.cin, c.ksz, c.ksz);
            if (!h->w[i]) FEMASR_CHECK_HIP(hipMalloc((void **)&h->w[i], femasr_packed_weight_floats(c.cout, c.cin, c.ksz, c.ksz) * sizeof(float)));
            const int rc = femasr_repack_oihw(nullptr, dev_ptr, c.cout, c.cin, c.ksz, c.ksz, h->w[i]);
            if (rc) return rc;
            FEMASR_CHECK_HIP(hipStreamSynchronize(nullptr));
            h->wset[i] = true;
            h->finalized = false;
            return FEMASR_OK;
        }
        if (k == pre + ".bias") {
            if (!(ndim == 1 && shape[0] == c.cout))
                return femasr_set_error(FEMASR_ERR_WEIGHT, "lpips_set_weight: '%s' must be (%d,)", key, c.cout);
            if (!h->bias[i]) FEMASR_CHECK_HIP(hipMalloc((void **)&h->bias[i], (size_t)c.cout * sizeof(float)));
            FEMASR_CHECK_HIP(hipMemcpyAsync(h->bias[i], dev_ptr, (size_t)c.cout * sizeof(float), hipMemcpyDeviceToDevice, nullptr));
            FEMASR_CHECK_HIP(hipStreamSynchronize(nullptr));
            h->bset[i] = true;
            h->finalized = false;
            return FEMASR_OK;
        }
    }
    return femasr_set_error(FEMASR_ERR_WEIGHT, "lpips_set_weight: unknown key '%s' for the %s net", key, h->net == 0 ? "alex" : "vgg16");
}

int femasr_lpips_finalize_weights(femasr_lpips_handle *h)
{
    FEMASR_REQUIRE(h, "lpips_finalize_weights: null handle");
    for (int i = 0; i < h->nconv; ++i) {
        if (!h->wset[i]) return femasr_set_error(FEMASR_ERR_WEIGHT, "lpips_finalize_weights: '%s.weight' was never set", h->convs[i].key);
        if (!h->bset[i]) return femasr_set_error(FEMASR_ERR_WEIGHT, "lpips_finalize_weights: '%s.bias' was never set", h->convs[i].key);
    }
    for (int t = 0; t < LP_NTAPS; ++t)
        if (!h->linset[t]) return femasr_set_error(FEMASR_ERR_WEIGHT, "lpips_finalize_weights: 'lin%d.model.1.weight' was never set", t);
    h->finalized = true;
    return FEMASR_OK;
}

int femasr_lpips_workspace_bytes(const femasr_lpips_handle *h, int B, int H, int W, size_t *bytes)
{
    FEMASR_REQUIRE(h && bytes, "lpips_workspace_bytes: null argument");
    LpPlan pl;
    const int rc = check_shape(h, B, H, W, &pl);
    if (rc) return rc;
    *bytes = layout(pl, B, H, W).total;
    return FEMASR_OK;
}

int femasr_lpips_forward(femasr_lpips_handle *h, void *stream, const float *x0_nchw, const float *x1_nchw, int B, int H, int W,
                         float *out, float *per_layer, void *ws, size_t ws_bytes)
{
    FEMASR_REQUIRE(h && x0_nchw && x1_nchw && out && ws, "lpips_forward: null argument");
    FEMASR_REQUIRE(h->finalized, "lpips_forward: weights not finalized (femasr_lpips_finalize_weights)");
    FEMASR_REQUIRE(((uintptr_t)ws & 255) == 0, "lpips_forward: workspace must be 256-byte aligned");
    LpPlan pl;
    int rc = check_shape(h, B, H, W, &pl);
    if (rc) return rc;
    const WsLayout L = layout(pl, B, H, W);
    if (ws_bytes < L.total)
        return femasr_set_error(FEMASR_ERR_WORKSPACE, "lpips_forward: workspace %zu bytes < %zu needed", ws_bytes, L.total);
    DeviceGuard guard(h->device);
    FEMASR_REQUIRE(guard.ok, "lpips_forward: hipSetDevice(%d) failed", h->device);
    const hipStream_t s = (hipStream_t)stream;
    char *base = (char *)ws;
    float *X = (float *)(base + L.in_off), *bufA = (float *)(base + L.a_off), *bufB = (float *)(base + L.b_off);
    double *part = (double *)(base + L.part_off);
    const int B2 = 2 * B;
    hipLaunchKernelGGL(lpips_input_kernel, dim3(grid_1d((size_t)B2 * H * W)), dim3(256), 0, s, x0_nchw, x1_nchw, B, H, W, X);
    FEMASR_CHECK_HIP(hipGetLastError());
    const float *cur = X;
    int ch = H, cw = W;
    for (int i = 0; i < h->nconv; ++i) {
        const LpConv &c = h->convs[i];
        float *dst = cur == bufA ? bufB : bufA;
        femasr_conv_args a{};
        a.in = cur; a.B = B2; a.H = ch; a.W = cw; a.Cin = c.cin;
        a.w = h->w[i]; a.bias = h->bias[i];
        a.Cout = c.cout; a.ksz = c.ksz; a.stride = c.stride; a.pad = c.pad; a.up2 = 0;
        a.prologue = FEMASR_PRO_NONE; a.act = FEMASR_ACT_RELU;
        a.out = dst; a.Ho = pl.ho[i]; a.Wo = pl.wo[i];
        rc = femasr_conv2d_launch(s, &a, nullptr, nullptr, nullptr);
        if (rc) return rc;
        cur = dst;
        ch = pl.ho[i];
        cw = pl.wo[i];
        if (c.tap) {
            float *pooled = c.pool ? (cur == bufA ? bufB : bufA) : nullptr;
            rc = tap_launch(s, cur, B2, ch, cw, c.cout, h->lin[c.tap - 1], c.pool, pooled, part + L.part_off_tap[c.tap - 1]);
            if (rc) return rc;
            if (c.pool) {
                cur = pooled;
                ch = pool_out(ch, c.pool);
                cw = pool_out(cw, c.pool);
            }
        }
    }
    int32_t hw[2 * LP_NTAPS];
    for (int k = 0; k < LP_NTAPS; ++k) {
        hw[2 * k] = pl.tap_h[k];
        hw[2 * k + 1] = pl.tap_w[k];
    }
    return finalize_launch(s, part, B, LP_NTAPS, hw, out, per_layer);
}

int femasr_lpips_scale_input(void *stream, const float *x0_nchw, const float *x1_nchw, int B, int H, int W, float *out_nhwc)
{
    FEMASR_REQUIRE(x0_nchw && x1_nchw && out_nhwc && B >= 1 && H >= 1 && W >= 1, "lpips_scale_input: bad arguments");
    FEMASR_REQUIRE(2 * (long long)B * H * W * 3 < (1ll << 31), "lpips_scale_input: tensor reaches 2^31 elements");
    hipLaunchKernelGGL(lpips_input_kernel, dim3(grid_1d((size_t)2 * B * H * W)), dim3(256), 0, (hipStream_t)stream, x0_nchw, x1_nchw, B, H, W,
                       out_nhwc);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

int femasr_lpips_tap_partials(int H, int W)
{
    if (H < 1 || W < 1) return 0;
    return (int)(((long long)H * W + TAP_PIX - 1) / TAP_PIX);
}

int femasr_lpips_tap(void *stream, const float *f, int B2, int H, int W, int C, const float *w_lin, int pool, float *pooled_out,
                     double *partials)
{
    return tap_launch((hipStream_t)stream, f, B2, H, W, C, w_lin, pool, pooled_out, partials);
}

int femasr_lpips_finalize(void *stream, const double *partials, int B, int ntaps, const int32_t *tap_hw, float *out, float *per_layer)
{
    return finalize_launch((hipStream_t)stream, partials, B, ntaps, tap_hw, out, per_layer);
}

}  // extern "C"

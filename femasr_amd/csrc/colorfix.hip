// colorfix.hip — the opt-in wavelet colour fix (femasr_amd/colorfix.py) on gfx950: the coarse bands of a super-resolved
// canvas are replaced by those of its bicubically upsampled input,
//   up = imresize(lq, s);  d = up - sr;  L a-trous levels of the (1/4, 1/2, 1/4) blur on d, radius 2^i, replicate border;  out = sr + d.
//
// Schedule of one group of planes (a group is as many planes as the caller's workspace holds; a uint8 image is three planes, channel
// c of image b being plane 3 b + c, so the peak of the uint8 path is a plane's workspace, never the canvas in fp32):
//   cf_hpass_kernel   the H pass of imresize into the fp64 intermediate (sH x W); uint8: the deinterleave and (float)byte / 255.0f fused in
//   cf_diff_kernel    the W pass, rounded once to fp32 (= femasr_imresize's float32 result), minus sr -> d
//   cf_level_kernel   one level, both passes in one launch: every thread recomputes the three horizontal rows its vertical taps need
//                     (nine loads of d, served by L2: the plane is read once from HBM per level), ping-pong between the two buffers
//   cf_store_kernel   out = sr + d: fp32 store (may alias sr), or rint(clamp(out, 0, 1) * 255) into HWC bytes (may alias sr)
//
// Arithmetic.  The resize accumulates in fp64 in tap order as niqe.hip does.  Everything after it is ONE IEEE fp32 operation per written
// step (the library is built with -ffp-contract=off), in the order of the definition:
//   t[y,x]  = (0.25 d[y,cl(x-r)] + 0.5 d[y,x]) + 0.25 d[y,cl(x+r)]
//   d'[y,x] = (0.25 t[cl(y-r),x] + 0.5 t[y,x]) + 0.25 t[cl(y+r),x]
// so tests/colorfix_ref.py (float32 numpy) reproduces every bit.  No atomics, no LDS, no scratch; every output element is written by one
// thread and depends on its own plane only: run-to-run deterministic, independent of batch, grouping and stream.
#include "common.h"
#include "pixel.h"
#include <math.h>

namespace {

constexpr int CF_THREADS = 256;
constexpr int CF_MAX_GROUP = 65535;       // planes per launch: grid.y
constexpr int CF_MAX_LEVELS = 12;

// Element p of plane `unit` of an image batch: fp32 planes back to back, or channel unit % 3 of the uint8 HWC image unit / 3 as
// (float)byte / 255.0f (IEEE division) - the deinterleave of the uint8 form
template <bool U8>
__device__ __forceinline__ size_t cf_index(size_t unit, size_t plane, size_t p)
{
    if constexpr (U8)
        return ((unit / 3) * plane + p) * 3 + unit % 3;
    else
        return unit * plane + p;
}

template <bool U8>
__device__ __forceinline__ float cf_load(const void *base, size_t unit, size_t plane, size_t p)
{
    if constexpr (U8)
        return pixel_byte_to_unit(((const uint8_t *)base)[cf_index<U8>(unit, plane, p)]);
    else
        return ((const float *)base)[cf_index<U8>(unit, plane, p)];
}

// planes u0 + blockIdx.y of lq -> tmp: (grid.y, sH, W) fp64
template <bool U8>
__global__ __launch_bounds__(CF_THREADS) void cf_hpass_kernel(const void *__restrict__ lq, size_t u0, int H, int W, int sH,
                                                              const double *__restrict__ w, const int32_t *__restrict__ idx, int P,
                                                              double *__restrict__ tmp)
{
    const size_t unit = u0 + blockIdx.y;
    const int p = blockIdx.x * CF_THREADS + threadIdx.x;
    if (p >= sH * W) return;
    const int i = p / W, x = p - i * W;
    double acc = 0.0;
    for (int k = 0; k < P; ++k) {
        const int j = clampi(idx[i * P + k], 0, H - 1);      // (tables from imresize_tables are in range; the clamp keeps a bad table in bounds)
        acc = acc + w[i * P + k] * (double)cf_load<U8>(lq, unit, (size_t)H * W, (size_t)j * W + x);
    }
    tmp[blockIdx.y * ((size_t)sH * W) + p] = acc;
}

// d = (float)(W pass of tmp) - sr;   d: (grid.y, sH, sW) fp32, sr: planes u0 + blockIdx.y
template <bool U8>
__global__ __launch_bounds__(CF_THREADS) void cf_diff_kernel(const double *__restrict__ tmp, const void *__restrict__ sr, size_t u0, int W, int sH,
                                                             int sW, const double *__restrict__ w, const int32_t *__restrict__ idx, int P,
                                                             float *__restrict__ d)
{
    const size_t unit = u0 + blockIdx.y;
    const int p = blockIdx.x * CF_THREADS + threadIdx.x;
    if (p >= sH * sW) return;
    const int y = p / sW, j = p - y * sW;
    const size_t plane = (size_t)sH * sW;
    const double *src = tmp + blockIdx.y * ((size_t)sH * W) + (size_t)y * W;
    double acc = 0.0;
    for (int k = 0; k < P; ++k) {
        const int x = clampi(idx[j * P + k], 0, W - 1);
        acc = acc + w[j * P + k] * src[x];
    }
    d[blockIdx.y * plane + p] = (float)acc - cf_load<U8>(sr, unit, plane, (size_t)p);
}

__device__ __forceinline__ float cf_row(const float *__restrict__ row, int xm, int x, int xp)
{
    return (0.25f * row[xm] + 0.5f * row[x]) + 0.25f * row[xp];
}

// one a-trous level of radius r on the planes (grid.y, sH, sW): in -> out (different buffers)
__global__ __launch_bounds__(CF_THREADS) void cf_level_kernel(const float *__restrict__ in, int sH, int sW, int r, float *__restrict__ out)
{
    const size_t plane = (size_t)sH * sW;
    const int p = blockIdx.x * CF_THREADS + threadIdx.x;
    if (p >= sH * sW) return;
    const int y = p / sW, x = p - y * sW;
    const float *src = in + blockIdx.y * plane;
    // (r <= 2^11 and sH sW < 2^31: the sums below stay inside int)
    const int xm = x - r < 0 ? 0 : x - r, xp = x + r > sW - 1 ? sW - 1 : x + r;
    const int ym = y - r < 0 ? 0 : y - r, yp = y + r > sH - 1 ? sH - 1 : y + r;
    const float tm = cf_row(src + (size_t)ym * sW, xm, x, xp);
    const float t0 = cf_row(src + (size_t)y * sW, xm, x, xp);
    const float tp = cf_row(src + (size_t)yp * sW, xm, x, xp);
    out[blockIdx.y * plane + p] = (0.25f * tm + 0.5f * t0) + 0.25f * tp;
}

// out = sr + d on the planes u0 + blockIdx.y; fp32: NCHW planes, uint8: rint(clamp(out, 0, 1) * 255), half to even, into the plane's bytes
// of the HWC image.  out may be sr: a thread reads only the element it writes, and byte stores leave the other channels alone.
template <bool U8>
__global__ __launch_bounds__(CF_THREADS) void cf_store_kernel(const void *sr, size_t u0, const float *__restrict__ d, int sH, int sW, void *out)
{
    const size_t unit = u0 + blockIdx.y;
    const int p = blockIdx.x * CF_THREADS + threadIdx.x;
    if (p >= sH * sW) return;
    const size_t plane = (size_t)sH * sW;
    const float v = cf_load<U8>(sr, unit, plane, (size_t)p) + d[blockIdx.y * plane + p];
    if constexpr (U8)
        ((uint8_t *)out)[cf_index<U8>(unit, plane, p)] = pixel_unit_to_byte(v);
    else
        ((float *)out)[cf_index<U8>(unit, plane, p)] = v;
}

size_t cf_align(size_t v) { return (v + 255) & ~(size_t)255; }

// bytes of the workspace for a group of g planes: two fp32 buffers (g, sH, sW) and the fp64 intermediate of the resize (g, sH, W)
size_t cf_bytes(size_t g, int W, int sH, int sW)
{
    return 2 * cf_align(g * sH * sW * sizeof(float)) + cf_align(g * sH * W * sizeof(double));
}

int cf_check_shape(long long planes, int H, int W, int sH, int sW, int s)
{
    FEMASR_REQUIRE(planes >= 1 && H >= 1 && W >= 1 && sH >= 1 && sW >= 1 && s >= 1, "color_fix: empty shape: %lld planes, %dx%d -> %dx%d, scale %d",
                   planes, H, W, sH, sW, s);
    FEMASR_REQUIRE((long long)s * H == sH && (long long)s * W == sW, "color_fix: %dx%d is not %d times %dx%d", sH, sW, s, H, W);
    FEMASR_REQUIRE((long long)sH * sW < (1ll << 31), "color_fix: a plane of %dx%d reaches 2^31 elements", sH, sW);
    return FEMASR_OK;
}

template <bool U8>
int cf_run(hipStream_t st, const void *sr, const void *lq, long long planes, int H, int W, int sH, int sW, int s, int levels, const double *w_h,
           const int32_t *idx_h, int taps_h, const double *w_w, const int32_t *idx_w, int taps_w, void *out, void *ws, size_t ws_bytes)
{
    FEMASR_REQUIRE(sr && lq && out && ws && w_h && idx_h && w_w && idx_w, "color_fix: null argument");
    FEMASR_CHECK(cf_check_shape(planes, H, W, sH, sW, s));
    FEMASR_REQUIRE(levels >= 1 && levels <= CF_MAX_LEVELS, "color_fix: levels must be 1..%d, got %d", CF_MAX_LEVELS, levels);
    FEMASR_REQUIRE(taps_h >= 1 && taps_w >= 1 && (long long)sH * taps_h < (1ll << 31) && (long long)sW * taps_w < (1ll << 31),
                   "color_fix: tap counts %d, %d", taps_h, taps_w);
    FEMASR_REQUIRE(((uintptr_t)ws & 255) == 0, "color_fix: workspace must be 256-byte aligned");
    // the group: as many planes as the workspace holds
    size_t g = ws_bytes / ((size_t)sH * ((size_t)sW * 2 * sizeof(float) + (size_t)W * sizeof(double)));
    if (g > (size_t)planes) g = (size_t)planes;
    if (g > (size_t)CF_MAX_GROUP) g = CF_MAX_GROUP;
    while (g > 0 && cf_bytes(g, W, sH, sW) > ws_bytes) --g;
    FEMASR_REQUIRE(g >= 1, "color_fix: workspace %zu bytes < %zu needed for one plane", ws_bytes, cf_bytes(1, W, sH, sW));
    const size_t plane = (size_t)sH * sW;
    float *buf_a = (float *)ws;
    float *buf_b = (float *)((char *)ws + cf_align(g * plane * sizeof(float)));
    double *tmp = (double *)((char *)ws + 2 * cf_align(g * plane * sizeof(float)));
    const unsigned bx_h = (unsigned)(((long long)sH * W + CF_THREADS - 1) / CF_THREADS), bx = (unsigned)((plane + CF_THREADS - 1) / CF_THREADS);
    for (size_t u0 = 0; u0 < (size_t)planes; u0 += g) {
        const unsigned nu = (unsigned)((size_t)planes - u0 < g ? (size_t)planes - u0 : g);
        hipLaunchKernelGGL(cf_hpass_kernel<U8>, dim3(bx_h, nu), dim3(CF_THREADS), 0, st, lq, u0, H, W, sH, w_h, idx_h, taps_h, tmp);
        FEMASR_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(cf_diff_kernel<U8>, dim3(bx, nu), dim3(CF_THREADS), 0, st, (const double *)tmp, sr, u0, W, sH, sW, w_w, idx_w, taps_w,
                           buf_a);
        FEMASR_CHECK_HIP(hipGetLastError());
        float *cur = buf_a, *nxt = buf_b;
        for (int i = 0; i < levels; ++i) {
            hipLaunchKernelGGL(cf_level_kernel, dim3(bx, nu), dim3(CF_THREADS), 0, st, (const float *)cur, sH, sW, 1 << i, nxt);
            FEMASR_CHECK_HIP(hipGetLastError());
            float *t = cur;
            cur = nxt;
            nxt = t;
        }
        hipLaunchKernelGGL(cf_store_kernel<U8>, dim3(bx, nu), dim3(CF_THREADS), 0, st, sr, u0, (const float *)cur, sH, sW, out);
        FEMASR_CHECK_HIP(hipGetLastError());
    }
    return FEMASR_OK;
}

}  // namespace

extern "C" {

int femasr_color_fix_workspace_bytes(int planes, int H, int W, int sH, int sW, int s, size_t *bytes)
{
    FEMASR_REQUIRE(bytes, "color_fix_workspace_bytes: null argument");
    FEMASR_CHECK(cf_check_shape(planes, H, W, sH, sW, s));
    *bytes = cf_bytes((size_t)planes, W, sH, sW);
    return FEMASR_OK;
}

int femasr_color_fix(void *stream, const float *sr, const float *lq, int planes, int H, int W, int sH, int sW, int s, int levels,
                     const double *w_h, const int32_t *idx_h, int taps_h, const double *w_w, const int32_t *idx_w, int taps_w, float *out,
                     void *ws, size_t ws_bytes)
{
    return cf_run<false>((hipStream_t)stream, sr, lq, planes, H, W, sH, sW, s, levels, w_h, idx_h, taps_h, w_w, idx_w, taps_w, out, ws, ws_bytes);
}

int femasr_color_fix_u8(void *stream, const uint8_t *sr, const uint8_t *lq, int B, int H, int W, int sH, int sW, int s, int levels,
                        const double *w_h, const int32_t *idx_h, int taps_h, const double *w_w, const int32_t *idx_w, int taps_w, uint8_t *out,
                        void *ws, size_t ws_bytes)
{
    return cf_run<true>((hipStream_t)stream, sr, lq, 3ll * B, H, W, sH, sW, s, levels, w_h, idx_h, taps_h, w_w, idx_w, taps_w, out, ws, ws_bytes);
}

}  // extern "C"

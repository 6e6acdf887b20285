// kernels_layout.hip — the kernels that only move elements: the relayouts either side of the network (mirror pad, crop, uint8 image <->
// fp32 tensor), the tile steps of test_tile (extract, paste, overlap-blend paste) and concat+resize.  No arithmetic beyond the pixel
// rules of pixel.h and the blend's weighted mean.
#include "common.h"
#include "pixel.h"
#include <type_traits>

namespace {

// ------------------------------------------------------------------------------------------
// relayout: pad / crop (femasr_arch.py:454-465) and image pre / post-processing (img2tensor, tensor2img) as ONE kernel over a source and a
// destination format.  A format holds the dimensions of one image of its tensor and gives an element's offset from (n, c, y, x), the
// decode of a linear offset into (n, c, y, x), and the conversion between its element type and the unit-range float.
// ------------------------------------------------------------------------------------------
struct F32_NCHW {
    typedef float T;
    int C, H, W;
    __device__ __forceinline__ size_t at(int n, int c, int y, int x) const { return (((size_t)n * C + c) * H + y) * W + x; }
    __device__ __forceinline__ void decode(size_t i, int &n, int &c, int &y, int &x) const
    {
        x = (int)(i % W);
        size_t r = i / W;
        y = (int)(r % H);
        r /= H;
        c = (int)(r % C);
        n = (int)(r / C);
    }
    static __device__ __forceinline__ float load(T v) { return v; }
    static __device__ __forceinline__ T store(float v) { return v; }
};

struct F32_NHWC {
    typedef float T;
    int C, H, W;
    __device__ __forceinline__ size_t at(int n, int c, int y, int x) const { return (((size_t)n * H + y) * W + x) * C + c; }
    __device__ __forceinline__ void decode(size_t i, int &n, int &c, int &y, int &x) const
    {
        c = (int)(i % C);
        size_t r = i / C;
        x = (int)(r % W);
        r /= W;
        y = (int)(r % H);
        n = (int)(r / H);
    }
    static __device__ __forceinline__ float load(T v) { return v; }
    static __device__ __forceinline__ T store(float v) { return v; }
};

// uint8 HWC image, 3 channels; swap_rb = the bytes are in cv2's BGR order (channel c of the tensor is byte 2 - c); elements pass through
// the pixel rules: (float)u8 / 255.0f on the way in, clamp [0,1], x255, round half to even on the way out
struct U8_HWC {
    typedef unsigned char T;
    int H, W, swap_rb;
    __device__ __forceinline__ size_t at(int n, int c, int y, int x) const { return (((size_t)n * H + y) * W + x) * 3 + (swap_rb ? 2 - c : c); }
    __device__ __forceinline__ void decode(size_t i, int &n, int &c, int &y, int &x) const
    {
        c = (int)(i % 3);
        c = swap_rb ? 2 - c : c;
        size_t r = i / 3;
        x = (int)(r % W);
        r /= W;
        y = (int)(r % H);
        n = (int)(r / H);
    }
    static __device__ __forceinline__ float load(T v) { return pixel_byte_to_unit(v); }
    static __device__ __forceinline__ T store(float v) { return pixel_unit_to_byte(v); }
};

// one thread per OUTPUT element in the destination's order (coalesced stores); the source coordinate goes through the mirror rule -
// padded row H+i <- row H-1-i - which a crop (destination no larger than the source) never takes
template <class Src, class Dst>
__global__ void relayout_kernel(const typename Src::T *__restrict__ in, const Src src, typename Dst::T *__restrict__ out, const Dst dst, size_t total)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        int n, c, y, x;
        dst.decode(i, n, c, y, x);
        const int sy = y < src.H ? y : 2 * src.H - 1 - y, sx = x < src.W ? x : 2 * src.W - 1 - x;
        out[i] = Dst::store(Src::load(in[src.at(n, c, sy, sx)]));
    }
}

template <class Src, class Dst>
int relayout_launch(void *stream, const typename Src::T *in, const Src src, typename Dst::T *out, const Dst dst, size_t total)
{
    hipLaunchKernelGGL((relayout_kernel<Src, Dst>), dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, in, src, out, dst, total);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

// ------------------------------------------------------------------------------------------
// test_tile (femasr_arch.py:387-447): crops of one shape class -> one batch; upscaled tile bodies -> the canvas.  One kernel each over
// the element format: fp32 NCHW planes, E = 1 element per pixel; uint8 HWC (round 6: the tiled / multi-GPU path moves one byte per
// value), C = 1 plane of E = 3 interleaved bytes per pixel.
// ------------------------------------------------------------------------------------------
template <bool U8>
using tile_elem = typename std::conditional<U8, unsigned char, float>::type;

// out[(k*B + b), c, y, x] = in[b, c, yx[2k] + y, yx[2k+1] + x]   (the reference's input[:, :, y0p:y1p, x0p:x1p]); thread = one element
// of a tile row of E * tw contiguous elements
template <bool U8>
__global__ void extract_tiles_kernel(const tile_elem<U8> *__restrict__ in, int B, int C, int H, int W, const int *__restrict__ yx, int n,
                                     int th, int tw, tile_elem<U8> *__restrict__ out, size_t total)
{
    const int E = U8 ? 3 : 1, rowe = E * tw;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int xe = (int)(i % rowe);
        size_t r = i / rowe;
        const int y = (int)(r % th);
        r /= th;
        const int c = U8 ? 0 : (int)(r % C);
        r = U8 ? r : r / C;
        const int b = (int)(r % B), k = (int)(r / B);
        out[i] = in[((((size_t)b * (U8 ? 1 : C) + c) * H + yx[2 * k] + y) * W + yx[2 * k + 1]) * E + xe];
    }
}

// canvas[b, c, dy + y, dx + x] = tiles[(k*B + b), c, sy + y, sx + x] for y < h, x < w; rect k = (sy, sx, dy, dx, h, w)
// (`output[:, :, dst] = output_tile[:, :, src]`, femasr_arch.py:443-446).  One block per (tile, image, channel, row).
template <bool U8>
__global__ void paste_tiles_kernel(const tile_elem<U8> *__restrict__ tiles, int B, int C, int th, int tw, const int *__restrict__ rects,
                                   int n, int Ho, int Wo, tile_elem<U8> *__restrict__ out, int hmax)
{
    const int E = U8 ? 3 : 1;
    size_t r = blockIdx.x;
    const int y = (int)(r % hmax);
    r /= hmax;
    const int c = U8 ? 0 : (int)(r % C);
    r = U8 ? r : r / C;
    const int b = (int)(r % B), k = (int)(r / B);
    const int *rc = rects + 6 * k;
    if (y >= rc[4]) return;
    const tile_elem<U8> *src = tiles + (((((size_t)k * B + b) * (U8 ? 1 : C) + c) * th + rc[0] + y) * tw + rc[1]) * E;
    tile_elem<U8> *dst = out + ((((size_t)b * (U8 ? 1 : C) + c) * Ho + rc[2] + y) * Wo + rc[3]) * E;
    for (int x = threadIdx.x; x < E * rc[5]; x += blockDim.x) dst[x] = src[x];
}

// ------------------------------------------------------------------------------------------
// Overlap-blend paste (NOT the reference's arithmetic; opt-in): every canvas pixel is the weighted mean of the
// upscaled WINDOWS (halo included) that contain it, tiles visited in row-major order.  Gather form: one thread per canvas element,
// no atomics, no weight canvas, the canvas is written once and never read.
// geom[8k..] = (window origin y, x on the canvas, th, tw, leading / trailing margin in y, leading / trailing margin in x) in upscaled
// pixels (tiling.blend_table); a margin of 0 is an image border.  ptrs[k] = tile k, image 0; image b follows th*tw*channels later.
// ------------------------------------------------------------------------------------------
// 1-D weight of window coordinate i in [0, len): a linear ramp over the 2*margin wide overlap, centred on the body edge, sampled at
// pixel centres; > 0 everywhere, 1 outside the ramps.  One IEEE divide per side (the integers are exact in fp32: below 2^24).
__device__ __forceinline__ float blend_weight(int i, int len, int lead, int trail)
{
    const float wl = lead == 0 ? 1.0f : fminf(1.0f, (float)(2 * i + 1) / (float)(4 * lead));
    const float wr = trail == 0 ? 1.0f : fminf(1.0f, (float)(2 * (len - 1 - i) + 1) / (float)(4 * trail));
    return fminf(wl, wr);
}

// One block = one canvas row (b, c, Y) inside one body-cell column cx: the candidate tiles - the pixel's own cell and its +-1
// neighbours (2 tile_pad <= tile_size) - depend on the block alone, so the table reads are scalar loads and every tile row is
// read as one contiguous run along x.  The last cell row / column takes what the canvas has beyond it (hand-made tables only).
template <bool U8>
__global__ __launch_bounds__(256) void blend_tiles_kernel(const unsigned long long *__restrict__ ptrs, const int *__restrict__ geom,
                                                         int tiles_y, int tiles_x, int pitch, int C, int Ho, int Wo, void *__restrict__ out_)
{
    using T = typename std::conditional<U8, unsigned char, float>::type;
    // fp32: rows are (b, c, Y), E = 1 element per pixel; uint8 HWC: rows are (b, Y), E = 3 interleaved elements per pixel
    const int E = U8 ? 3 : 1;
    size_t r = blockIdx.x;
    const int Y = (int)(r % Ho);
    r /= Ho;
    const int c = U8 ? 0 : (int)(r % C);
    const size_t b = U8 ? r : r / C;
    const int cx = blockIdx.y, cy = min(Y / pitch, tiles_y - 1);
    const int x0 = cx * pitch, x1 = cx == tiles_x - 1 ? Wo : min(x0 + pitch, Wo);
    T *dst = (T *)out_ + (size_t)blockIdx.x * Wo * E;
    for (int j = x0 * E + threadIdx.x; j < x1 * E; j += blockDim.x) {
        const int X = U8 ? j / 3 : j, ch = U8 ? j - 3 * X : 0;
        float acc = 0.0f, den = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int ty = cy + dy;
            if (ty < 0 || ty >= tiles_y) continue;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int tx = cx + dx;
                if (tx < 0 || tx >= tiles_x) continue;
                const int k = ty * tiles_x + tx;
                const int *g = geom + 8 * k;
                const int ly = Y - g[0], th = g[2], tw = g[3];
                if (ly < 0 || ly >= th) continue;                          // (block-uniform)
                const int lx = X - g[1];
                if (lx < 0 || lx >= tw) continue;                          // every read stays inside the th x tw tile the table names
                const float w = blend_weight(ly, th, g[4], g[5]) * blend_weight(lx, tw, g[6], g[7]);
                const T *t = (const T *)ptrs[k] + b * ((size_t)th * tw * (U8 ? 3 : C));
                const float v = (float)(U8 ? t[((size_t)ly * tw + lx) * 3 + ch] : t[((size_t)c * th + ly) * tw + lx]);
                acc = acc + w * v;
                den = den + w;
            }
        }
        float q = den > 0.0f ? acc / den : 0.0f;                            // (no tile: a hand-made table; 0 like the paste's zero canvas)
        if (U8) {
            // (not pixel_unit_to_byte: the mean of bytes is already on the 0..255 scale - no x255, no NaN step: other arithmetic)
            q = q < 0.f ? 0.f : (q > 255.f ? 255.f : q);                   // tensor2img's rounding: half to even
            dst[j] = (T)rintf(q);
        } else {
            dst[j] = (T)q;
        }
    }
}

// out[n,y,x,:] = cat(a[n,y,x,:Ca], b[n, y*Hb/H, x*Wb/W, :Cb]); one thread per float4 of the output (Ca, Cb % 4 == 0)
__global__ void concat_resize_kernel(const float *__restrict__ a, int Ca, const float *__restrict__ b, int Hb, int Wb, int Cb,
                                     int H, int W, float *__restrict__ out, size_t total4)
{
    const int C4 = (Ca + Cb) >> 2, Ca4 = Ca >> 2;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4);
        size_t r = i / C4;
        const int x = (int)(r % W);
        r /= W;
        const int y = (int)(r % H);
        const size_t n = r / H;
        float4 v;
        if (c4 < Ca4) {
            v = ld4(a + ((n * H + y) * W + x) * Ca + 4 * c4);
        } else {
            const int sy = (int)(((long long)y * Hb) / H), sx = (int)(((long long)x * Wb) / W);
            v = ld4(b + ((n * Hb + sy) * Wb + sx) * Cb + 4 * (c4 - Ca4));
        }
        *reinterpret_cast<float4 *>(out + i * 4) = v;
    }
}

template <bool U8>
int extract_launch(void *stream, const tile_elem<U8> *in, int B, int C, int H, int W, const int32_t *yx_dev, int n, int th, int tw, tile_elem<U8> *out)
{
    const size_t total = (size_t)n * B * C * th * tw * (U8 ? 3 : 1);
    hipLaunchKernelGGL(extract_tiles_kernel<U8>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, in, B, C, H, W, yx_dev, n, th, tw, out, total);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

template <bool U8>
int paste_launch(void *stream, const tile_elem<U8> *tiles, int B, int C, int n, int th, int tw, const int32_t *rects_dev, int hmax, int Ho, int Wo,
                 tile_elem<U8> *out)
{
    const size_t rows = (size_t)n * B * C * hmax;
    FEMASR_REQUIRE(rows < ((size_t)1 << 31), "%s: too many rows", U8 ? "paste_tiles_u8" : "paste_tiles");
    hipLaunchKernelGGL(paste_tiles_kernel<U8>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, tiles, B, C, th, tw, rects_dev, n, Ho, Wo, out, hmax);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------
// C ABI (include/femasr_hip.h)
// ------------------------------------------------------------------------------------------
extern "C" {

int femasr_pad_nchw_to_nhwc(void *stream, const float *in, int B, int C, int H, int W, int Hp, int Wp, float *out)
{
    FEMASR_REQUIRE(in && out && B > 0 && C > 0 && H > 0 && W > 0, "pad: bad args");
    FEMASR_REQUIRE(Hp >= H && Wp >= W && Hp - H <= H && Wp - W <= W, "pad: mirror pad larger than the image (%d,%d)->(%d,%d)", H, W, Hp, Wp);
    return relayout_launch(stream, in, F32_NCHW{C, H, W}, out, F32_NHWC{C, Hp, Wp}, (size_t)B * Hp * Wp * C);
}

// femasr_forward_u8: the image decode (img2tensor + `/255.`) fused into the pad, swap_rb = the cv2 BGR order ...
int femasr_pad_u8hwc_to_nhwc(void *stream, const uint8_t *in, int B, int H, int W, int swap_rb, int Hp, int Wp, float *out)
{
    FEMASR_REQUIRE(in && out && B > 0 && H > 0 && W > 0 && Hp >= H && Wp >= W && Hp <= 2 * H && Wp <= 2 * W, "pad_u8: bad args");
    return relayout_launch(stream, in, U8_HWC{H, W, swap_rb}, out, F32_NHWC{3, Hp, Wp}, (size_t)B * Hp * Wp * 3);
}

// ... and tensor2img fused into the crop
int femasr_crop_nhwc_to_u8hwc(void *stream, const float *in, int B, int Hs, int Ws, int Hc, int Wc, int swap_rb, uint8_t *out)
{
    FEMASR_REQUIRE(in && out && B > 0 && Hc > 0 && Wc > 0 && Hc <= Hs && Wc <= Ws, "crop_u8: bad args");
    return relayout_launch(stream, in, F32_NHWC{3, Hs, Ws}, out, U8_HWC{Hc, Wc, swap_rb}, (size_t)B * Hc * Wc * 3);
}

int femasr_crop_nhwc_to_nchw(void *stream, const float *in, int B, int Hs, int Ws, int C, int Hc, int Wc, float *out)
{
    FEMASR_REQUIRE(in && out && B > 0 && C > 0 && Hc > 0 && Wc > 0 && Hc <= Hs && Wc <= Ws, "crop: bad args");
    return relayout_launch(stream, in, F32_NHWC{C, Hs, Ws}, out, F32_NCHW{C, Hc, Wc}, (size_t)B * C * Hc * Wc);
}

// the steps either side of the path on one image: uint8 HWC (BGR or RGB) <-> fp32 CHW RGB
int femasr_image_u8_to_f32(void *stream, const uint8_t *in_hwc, int H, int W, int swap_rb, float *out_chw)
{
    FEMASR_REQUIRE(in_hwc && out_chw && H > 0 && W > 0, "image_u8_to_f32: bad args");
    return relayout_launch(stream, in_hwc, U8_HWC{H, W, swap_rb}, out_chw, F32_NCHW{3, H, W}, (size_t)3 * H * W);
}

int femasr_image_f32_to_u8(void *stream, const float *in_chw, int H, int W, int swap_rb, uint8_t *out_hwc)
{
    FEMASR_REQUIRE(in_chw && out_hwc && H > 0 && W > 0, "image_f32_to_u8: bad args");
    return relayout_launch(stream, in_chw, F32_NCHW{3, H, W}, out_hwc, U8_HWC{H, W, swap_rb}, (size_t)3 * H * W);
}

int femasr_extract_tiles(void *stream, const float *in, int B, int C, int H, int W, const int32_t *yx_dev, int n, int th, int tw, float *out)
{
    FEMASR_REQUIRE(in && yx_dev && out && B > 0 && C > 0 && n > 0 && th > 0 && tw > 0 && th <= H && tw <= W, "extract_tiles: bad args");
    return extract_launch<false>(stream, in, B, C, H, W, yx_dev, n, th, tw, out);
}

int femasr_paste_tiles(void *stream, const float *tiles, int B, int C, int n, int th, int tw, const int32_t *rects_dev, int hmax,
                       int Ho, int Wo, float *out)
{
    FEMASR_REQUIRE(tiles && rects_dev && out && B > 0 && C > 0 && n > 0 && th > 0 && tw > 0 && hmax > 0 && hmax <= th, "paste_tiles: bad args");
    return paste_launch<false>(stream, tiles, B, C, n, th, tw, rects_dev, hmax, Ho, Wo, out);
}

int femasr_extract_tiles_u8(void *stream, const uint8_t *in, int B, int H, int W, const int32_t *yx_dev, int n, int th, int tw, uint8_t *out)
{
    FEMASR_REQUIRE(in && yx_dev && out && B > 0 && n > 0 && th > 0 && tw > 0 && th <= H && tw <= W, "extract_tiles_u8: bad args");
    return extract_launch<true>(stream, in, B, 1, H, W, yx_dev, n, th, tw, out);
}

int femasr_paste_tiles_u8(void *stream, const uint8_t *tiles, int B, int n, int th, int tw, const int32_t *rects_dev, int hmax, int Ho, int Wo, uint8_t *out)
{
    FEMASR_REQUIRE(tiles && rects_dev && out && B > 0 && n > 0 && th > 0 && tw > 0 && hmax > 0 && hmax <= th, "paste_tiles_u8: bad args");
    return paste_launch<true>(stream, tiles, B, 1, n, th, tw, rects_dev, hmax, Ho, Wo, out);
}

static int blend_launch(bool u8, void *stream, const uint64_t *tile_ptrs_dev, const int32_t *geom_dev, int n, int tiles_y, int tiles_x,
                        int pitch, int B, int C, int Ho, int Wo, void *out)
{
    const char *who = u8 ? "blend_tiles_u8" : "blend_tiles";
    FEMASR_REQUIRE(tile_ptrs_dev && geom_dev && out, "%s: null pointer", who);
    FEMASR_REQUIRE(n > 0 && B > 0 && C > 0 && tiles_y > 0 && tiles_x > 0 && pitch > 0 && Ho > 0 && Wo > 0, "%s: bad sizes", who);
    FEMASR_REQUIRE((long long)tiles_y * tiles_x == n, "%s: %d tiles given for a %d x %d grid", who, n, tiles_y, tiles_x);
    FEMASR_REQUIRE(tiles_x <= 65535, "%s: more than 65535 tile columns", who);
    const size_t rows = (size_t)B * C * Ho;
    FEMASR_REQUIRE(rows < ((size_t)1 << 31), "%s: too many rows", who);
    const dim3 grid((unsigned)rows, (unsigned)tiles_x);
    if (u8)
        hipLaunchKernelGGL(blend_tiles_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned long long *)tile_ptrs_dev,
                           geom_dev, tiles_y, tiles_x, pitch, 1, Ho, Wo, out);
    else
        hipLaunchKernelGGL(blend_tiles_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned long long *)tile_ptrs_dev,
                           geom_dev, tiles_y, tiles_x, pitch, C, Ho, Wo, out);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

int femasr_blend_tiles(void *stream, const uint64_t *tile_ptrs_dev, const int32_t *geom_dev, int n, int tiles_y, int tiles_x, int pitch,
                       int B, int C, int Ho, int Wo, float *out)
{
    return blend_launch(false, stream, tile_ptrs_dev, geom_dev, n, tiles_y, tiles_x, pitch, B, C, Ho, Wo, out);
}

int femasr_blend_tiles_u8(void *stream, const uint64_t *tile_ptrs_dev, const int32_t *geom_dev, int n, int tiles_y, int tiles_x, int pitch,
                          int B, int Ho, int Wo, uint8_t *out)
{
    return blend_launch(true, stream, tile_ptrs_dev, geom_dev, n, tiles_y, tiles_x, pitch, B, 1, Ho, Wo, out);
}

int femasr_concat_resize(void *stream, const float *a, int Ca, const float *b, int Hb, int Wb, int Cb, int B, int H, int W, float *out)
{
    FEMASR_REQUIRE(a && b && out && B > 0 && H > 0 && W > 0 && Hb > 0 && Wb > 0, "concat_resize: bad args");
    FEMASR_REQUIRE(Ca > 0 && Cb > 0 && Ca % 4 == 0 && Cb % 4 == 0, "concat_resize: channel counts must be multiples of 4 (%d, %d)", Ca, Cb);
    const size_t total4 = (size_t)B * H * W * ((Ca + Cb) / 4);
    hipLaunchKernelGGL(concat_resize_kernel, dim3(grid_for(total4)), dim3(256), 0, (hipStream_t)stream, a, Ca, b, Hb, Wb, Cb, H, W, out,
                       total4);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

}  // extern "C"

// ensemble.hip — the two data-movement kernels of the opt-in x8 geometric self-ensemble (femasr_amd/ensemble.py) on gfx950.
//
// Variant k = 0..7: v = k & 1 flips rows, h = (k >> 1) & 1 flips columns, t = (k >> 2) & 1 transposes:  x_k = T^t(H^h(V^v(x))).
//   expand   x (H,W) -> k = 0..3 `straight` (H,W):   x_k[i,j] = x[v ? H-1-i : i, h ? W-1-j : j]
//                       k = 4..7 `transposed` (W,H): x_k[i,j] = x[v ? H-1-j : j, h ? W-1-i : i]
//   merge    y_k -> out (H,W):  z_k[i,j] = y_k[v ? H-1-i : i, h ? W-1-j : j]   (k = 0..3, y_k of (H,W))
//                               z_k[i,j] = y_k[h ? W-1-j : j, v ? H-1-i : i]   (k = 4..7, y_k of (W,H))
//            fp32:  out = 0.125f * (((((((z_0 + z_1) + z_2) + z_3) + z_4) + z_5) + z_6) + z_7), one IEEE add per step in this order (the
//                   library is built with -ffp-contract=off), so a sequential restatement gives the same bits
//            uint8: S = sum_k z_k (0..2040), out = (S + 3 + ((S >> 3) & 1)) >> 3 = S / 8 rounded half to even, per byte
// Buffers are variant-major ([k][image]); an element is one float of a (B,C,H,W) batch or one 3-byte pixel of a (B,H,W,3) batch.
//
// One launch each; a block owns one DE_T x DE_T tile of one plane.  Expand reads its tile once (row-wise, coalesced), stores the four
// straight variants from registers (a flipped row is still one contiguous run per wave), parks the tile in LDS and stores the four transposed
// variants from its columns - so those stores run along the transposed row as well.  Merge sums z_0..z_3 row-wise, parks the partial sum in
// LDS, picks it up column-wise - where the loads of the transposed results are the contiguous ones -, adds z_4..z_7, puts the finished value
// back and stores it row-wise.  The LDS pitch is DE_T + 1 words, so the column accesses (lane stride = pitch) fall on distinct banks.
// Every output element is written by exactly one thread from its own inputs: no atomics, no scratch, no allocation, no synchronisation;
// deterministic, capture-safe, on the caller's stream.  Offsets are 64-bit; a plane of 2^31 elements or more is refused.
#include "common.h"

namespace {

constexpr int DE_T = 64;                        // tile edge: one wave covers one tile row
constexpr int DE_ROWS = 4;                      // waves per block
constexpr int DE_THREADS = DE_T * DE_ROWS;
constexpr int DE_PITCH = DE_T + 1;

// An fp32 element: the sum is the running fp32 sum itself
struct de_f32 {
    using elem = float;
    using word = float;
    using sum = float;
    static __device__ __forceinline__ word load(const elem *p, size_t i) { return p[i]; }
    static __device__ __forceinline__ void store(elem *p, size_t i, word w) { p[i] = w; }
    static __device__ __forceinline__ sum first(word w) { return w; }
    static __device__ __forceinline__ sum add(sum s, word w) { return s + w; }
    static __device__ __forceinline__ word park(sum s) { return s; }
    static __device__ __forceinline__ sum pick(word w) { return w; }
    static __device__ __forceinline__ word finish(sum s) { return 0.125f * s; }
};

// A 3-byte pixel, moved whole: bytes 0..2 in bits 0..7, 8..15, 16..23 of a word.  The sum is one integer per channel (order-free); the
// partial sum of four variants (<= 1020 per channel) is parked in 10-bit fields
struct de_px8 {
    using elem = uint8_t;
    using word = uint32_t;
    struct sum { uint32_t r, g, b; };
    static __device__ __forceinline__ word load(const elem *p, size_t i)
    {
        const elem *q = p + 3 * i;
        return (word)q[0] | ((word)q[1] << 8) | ((word)q[2] << 16);
    }
    static __device__ __forceinline__ void store(elem *p, size_t i, word w)
    {
        elem *q = p + 3 * i;
        q[0] = (elem)(w & 255u);
        q[1] = (elem)((w >> 8) & 255u);
        q[2] = (elem)((w >> 16) & 255u);
    }
    static __device__ __forceinline__ sum first(word w) { return sum{w & 255u, (w >> 8) & 255u, (w >> 16) & 255u}; }
    static __device__ __forceinline__ sum add(sum s, word w) { return sum{s.r + (w & 255u), s.g + ((w >> 8) & 255u), s.b + ((w >> 16) & 255u)}; }
    static __device__ __forceinline__ word park(sum s) { return s.r | (s.g << 10) | (s.b << 20); }
    static __device__ __forceinline__ sum pick(word w) { return sum{w & 1023u, (w >> 10) & 1023u, (w >> 20) & 1023u}; }
    static __device__ __forceinline__ uint32_t eighth(uint32_t s) { return (s + 3u + ((s >> 3) & 1u)) >> 3; }      // S / 8, half to even
    static __device__ __forceinline__ word finish(sum s) { return eighth(s.r) | (eighth(s.g) << 8) | (eighth(s.b) << 16); }
};

// The block's tile: (plane, first row, first column) from the linear block index (tiles_x fastest)
__device__ __forceinline__ void de_tile(unsigned tiles_x, unsigned tiles_y, size_t &p, int &y0, int &x0)
{
    const unsigned bx = blockIdx.x % tiles_x, rest = blockIdx.x / tiles_x;
    x0 = (int)(bx * DE_T);
    y0 = (int)((rest % tiles_y) * DE_T);
    p = rest / tiles_y;
}

// x: `planes` planes of (H,W); straight: (4, planes, H, W); transposed: (4, planes, W, H)
template <class E>
__global__ __launch_bounds__(DE_THREADS) void de_expand_kernel(const typename E::elem *__restrict__ x, size_t planes, int H, int W, unsigned tiles_x,
                                                               unsigned tiles_y, typename E::elem *straight, typename E::elem *transposed)
{
    __shared__ typename E::word tile[DE_T][DE_PITCH];
    size_t p;
    int y0, x0;
    de_tile(tiles_x, tiles_y, p, y0, x0);
    const size_t plane = (size_t)H * W;
    const int lx = threadIdx.x % DE_T, lr = threadIdx.x / DE_T;
    const int xx = x0 + lx;
    for (int ly = lr; ly < DE_T; ly += DE_ROWS) {
        const int y = y0 + ly;
        if (y < H && xx < W) {
            const typename E::word w = E::load(x, p * plane + (size_t)y * W + xx);
            tile[ly][lx] = w;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = (k & 1) ? H - 1 - y : y, j = (k & 2) ? W - 1 - xx : xx;
                E::store(straight, ((size_t)k * planes + p) * plane + (size_t)i * W + j, w);
            }
        }
    }
    __syncthreads();
    const int ys = y0 + lx;                     // the lanes now run down a column of x: along a row of the transposed variants
    for (int r = lr; r < DE_T; r += DE_ROWS) {
        const int xs = x0 + r;
        if (ys < H && xs < W) {
            const typename E::word w = tile[lx][r];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = (k & 2) ? W - 1 - xs : xs, j = (k & 1) ? H - 1 - ys : ys;
                E::store(transposed, ((size_t)k * planes + p) * plane + (size_t)i * H + j, w);
            }
        }
    }
}

// straight: (4, planes, H, W); transposed: (4, planes, W, H); out: `planes` planes of (H,W)
template <class E>
__global__ __launch_bounds__(DE_THREADS) void de_merge_kernel(const typename E::elem *straight, const typename E::elem *transposed, size_t planes, int H,
                                                              int W, unsigned tiles_x, unsigned tiles_y, typename E::elem *__restrict__ out)
{
    __shared__ typename E::word tile[DE_T][DE_PITCH];
    size_t p;
    int y0, x0;
    de_tile(tiles_x, tiles_y, p, y0, x0);
    const size_t plane = (size_t)H * W;
    const int lx = threadIdx.x % DE_T, lr = threadIdx.x / DE_T;
    const int xx = x0 + lx;
    for (int ly = lr; ly < DE_T; ly += DE_ROWS) {
        const int y = y0 + ly;
        if (y < H && xx < W) {
            typename E::sum s = E::first(E::load(straight, p * plane + (size_t)y * W + xx));
#pragma unroll
            for (int k = 1; k < 4; ++k) {
                const int i = (k & 1) ? H - 1 - y : y, j = (k & 2) ? W - 1 - xx : xx;
                s = E::add(s, E::load(straight, ((size_t)k * planes + p) * plane + (size_t)i * W + j));
            }
            tile[ly][lx] = E::park(s);
        }
    }
    __syncthreads();
    const int yi = y0 + lx;                     // the lanes run down a column of out: along a row of the transposed results
    for (int r = lr; r < DE_T; r += DE_ROWS) {
        const int xj = x0 + r;
        if (yi < H && xj < W) {
            typename E::sum s = E::pick(tile[lx][r]);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = (k & 2) ? W - 1 - xj : xj, j = (k & 1) ? H - 1 - yi : yi;
                s = E::add(s, E::load(transposed, ((size_t)k * planes + p) * plane + (size_t)i * H + j));
            }
            tile[lx][r] = E::finish(s);
        }
    }
    __syncthreads();
    for (int ly = lr; ly < DE_T; ly += DE_ROWS) {
        const int y = y0 + ly;
        if (y < H && xx < W) E::store(out, p * plane + (size_t)y * W + xx, tile[ly][lx]);
    }
}

// The launch geometry, or the refusal: one block per tile, linear in grid.x
int de_grid(const char *what, long long planes, int H, int W, unsigned *tiles_x, unsigned *tiles_y, unsigned *blocks)
{
    FEMASR_REQUIRE(planes >= 1 && H >= 1 && W >= 1, "%s: empty shape: %lld planes of %dx%d", what, planes, H, W);
    FEMASR_REQUIRE((long long)H * W < (1ll << 31), "%s: a plane of %dx%d reaches 2^31 elements", what, H, W);
    const long long tx = ((long long)W + DE_T - 1) / DE_T, ty = ((long long)H + DE_T - 1) / DE_T;
    FEMASR_REQUIRE(tx * ty <= ((1ll << 31) - 1) / planes, "%s: %lld planes of %dx%d are more than 2^31 - 1 tiles", what, planes, H, W);
    *tiles_x = (unsigned)tx;
    *tiles_y = (unsigned)ty;
    *blocks = (unsigned)(tx * ty * planes);
    return FEMASR_OK;
}

template <class E>
int de_expand(const char *what, hipStream_t st, const typename E::elem *x, long long planes, int H, int W, typename E::elem *straight,
              typename E::elem *transposed)
{
    FEMASR_REQUIRE(x && straight && transposed, "%s: null argument", what);
    unsigned tx, ty, blocks;
    FEMASR_CHECK(de_grid(what, planes, H, W, &tx, &ty, &blocks));
    hipLaunchKernelGGL(de_expand_kernel<E>, dim3(blocks), dim3(DE_THREADS), 0, st, x, (size_t)planes, H, W, tx, ty, straight, transposed);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

template <class E>
int de_merge(const char *what, hipStream_t st, const typename E::elem *straight, const typename E::elem *transposed, long long planes, int H, int W,
             typename E::elem *out)
{
    FEMASR_REQUIRE(straight && transposed && out, "%s: null argument", what);
    unsigned tx, ty, blocks;
    FEMASR_CHECK(de_grid(what, planes, H, W, &tx, &ty, &blocks));
    hipLaunchKernelGGL(de_merge_kernel<E>, dim3(blocks), dim3(DE_THREADS), 0, st, straight, transposed, (size_t)planes, H, W, tx, ty, out);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

long long de_planes(int B, int C) { return B >= 1 && C >= 1 ? (long long)B * C : 0; }

}  // namespace

extern "C" {

int femasr_dihedral_expand(void *stream, const float *x, int B, int C, int H, int W, float *straight, float *transposed)
{
    return de_expand<de_f32>("dihedral_expand", (hipStream_t)stream, x, de_planes(B, C), H, W, straight, transposed);
}

int femasr_dihedral_expand_u8(void *stream, const uint8_t *x, int B, int H, int W, uint8_t *straight, uint8_t *transposed)
{
    return de_expand<de_px8>("dihedral_expand_u8", (hipStream_t)stream, x, de_planes(B, 1), H, W, straight, transposed);
}

int femasr_dihedral_merge(void *stream, const float *straight, const float *transposed, int B, int C, int H, int W, float *out)
{
    return de_merge<de_f32>("dihedral_merge", (hipStream_t)stream, straight, transposed, de_planes(B, C), H, W, out);
}

int femasr_dihedral_merge_u8(void *stream, const uint8_t *straight, const uint8_t *transposed, int B, int H, int W, uint8_t *out)
{
    return de_merge<de_px8>("dihedral_merge_u8", (hipStream_t)stream, straight, transposed, de_planes(B, 1), H, W, out);
}

}  // extern "C"

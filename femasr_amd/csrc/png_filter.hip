// png_filter.hip — PNG's row filters for 8-bit samples on gfx950 (femasr_amd/pngio.py): uint8 (B,H,W,C) images, C = 1 (gray),
// 2 (gray + alpha), 3 (RGB: what the network returns), 4 (RGBA) -> the byte stream PNG deflates, (B,H,1 + CW): per row one filter-type byte
// and the CW residuals.  The kernel is a template on the pixel size C (the distance to the left neighbour); C = 3 is femasr_png_filter_rgb8.
//
// Definition (pngio.filter_image, for C = 3 pngio.filter_rows; integers only).  n = CW, raw[y] = the n bytes of row y.  Per byte i, x = raw[y][i]:
//   a = raw[y][i-C] (0 if i < C),  b = raw[y-1][i] (0 if y == 0),  c = raw[y-1][i-C] (0 if either is outside)
//   f0 = x, f1 = x - a, f2 = x - b, f3 = x - ((a + b) >> 1), f4 = x - paeth(a, b, c)   (mod 256)
//   paeth: p = a + b - c, pa = |p - a|, pb = |p - b|, pc = |p - c|: a if pa <= pb and pa <= pc, else b if pb <= pc, else c
//   cost_t = sum_i min(f_t[i], 256 - f_t[i]);  adaptive: t* = the smallest t of least cost;  out[y] = [t*, f_t*[0..n)]
//
// One launch; a TEAM owns a row: the block's 256 threads, or - rows of up to PF_WAVE_ROW bytes - one of its four waves, so that small
// images do not launch mostly idle blocks.  A team
//   1. stages its row and the row above in LDS with aligned 16-byte loads (the row above was some other team's row: L2),
//   2. adds up the five costs over the row, 16 bytes per lane and step, reduces them over the wave with shuffles and - block teams - over
//      the waves with one LDS step, and every lane picks t* from the same five sums,
//   3. reads the row from LDS again, applies t* and stores.
// Rows of up to PF_BLOCK_ROW bytes are RESIDENT: global memory is read once.  Longer rows go through the same three steps in segments of
// that size and are read twice (second time from L2 where it holds them).
//
// Alignment.  Neither the input row (y n) nor the output row (y (n + 1)) starts on a 16-byte boundary in general.  All wide accesses
// are on ALIGNED addresses: a lane's unit of work is one aligned 16-byte chunk of the OUTPUT; the input bytes it needs are fetched from the
// LDS copy - which holds the input's aligned 16-byte chunks as loaded - through aligned dword reads and a funnel shift by the (row-uniform)
// byte distance between the two alignments.  Chunks that a row shares with its neighbours (its first and last) are stored byte by byte;
// a chunk of the input that is not wholly inside the image array (its very first and last) is loaded byte by byte.  No access leaves the
// buffers.
//
// Four bytes per instruction: x - y, (a + b) >> 1 are SWAR on dwords, the cost of four residuals is one v_sad_u8 (|r - 128| of r = f ^ 128 is
// min(f, 256 - f)); Paeth's predictor is per byte.  No workspace, no atomics, no scratch, no allocation, no synchronisation: capture-safe, on
// the caller's stream.  Offsets between rows and images are 64-bit, inside a row 32-bit (n <= 3 2^22: n and the cost sums, <= 128 n, fit).
#include "common.h"

namespace {

constexpr int PF_THREADS = 256;
constexpr int PF_WAVE = 64;
constexpr int PF_WAVE_ROW = 3072;        // rows of up to this many bytes (RGB: W <= 1024): one wave per row
constexpr int PF_BLOCK_ROW = 24576;      // rows of up to this many bytes (RGB: W <= 8192) are resident in a block team's LDS
constexpr int PF_FRONT = 32;             // LDS bytes in front of the first staged chunk (zero where they stand for bytes left of the row)
constexpr int PF_MAX_ROW = 3 << 22;      // bytes in a row (RGB: W <= 2^22)
constexpr int PF_ADAPTIVE = 5;
constexpr uint32_t PF_H = 0x80808080u;

// (hi:lo) >> 8 * bytes, bytes 0..3: v_alignbit_b32
__host__ __device__ __forceinline__ uint32_t pf_shift(uint32_t lo, uint32_t hi, unsigned bytes)
{
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * bytes));
}
// per byte x - y mod 256
__host__ __device__ __forceinline__ uint32_t pf_sub(uint32_t x, uint32_t y) { return ((x | PF_H) - (y & ~PF_H)) ^ ((x ^ ~y) & PF_H); }
// per byte (a + b) >> 1
__host__ __device__ __forceinline__ uint32_t pf_avg(uint32_t a, uint32_t b) { return (a & b) + (((a ^ b) & 0xfefefefeu) >> 1); }
// per byte Paeth's predictor
__host__ __device__ __forceinline__ uint32_t pf_paeth(uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const int ai = (int)((a >> k) & 255u), bi = (int)((b >> k) & 255u), ci = (int)((c >> k) & 255u);
        const int pa = abs(bi - ci), pb = abs(ai - ci), pc = abs(ai + bi - 2 * ci);
        const int p = (pa <= pb && pa <= pc) ? ai : (pb <= pc ? bi : ci);
        r |= (uint32_t)p << k;
    }
    return r;
}
// sum over the four bytes of min(f, 256 - f), added to acc
__host__ __device__ __forceinline__ uint32_t pf_cost(uint32_t f, uint32_t acc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sad_u8(f ^ PF_H, PF_H, acc);
#else
    for (int k = 0; k < 32; k += 8) {
        const uint32_t v = (f >> k) & 255u;
        acc += v < 256u - v ? v : 256u - v;
    }
    return acc;
#endif
}
// residual of filter t (0..4) for four bytes
__host__ __device__ __forceinline__ uint32_t pf_residual(int t, uint32_t x, uint32_t a, uint32_t b, uint32_t c)
{
    switch (t) {
    case 0: return x;
    case 1: return pf_sub(x, a);
    case 2: return pf_sub(x, b);
    case 3: return pf_sub(x, pf_avg(a, b));
    default: return pf_sub(x, pf_paeth(a, b, c));
    }
}
// the bytes of a dword that holds row bytes i .. i + 3 which lie in [0, n)
__host__ __device__ __forceinline__ uint32_t pf_valid(int i, int n)
{
    const int lo = i < 0 ? -i : 0, hi = n - i < 4 ? n - i : 4;
    if (lo >= hi) return 0u;
    const uint32_t upto_hi = hi >= 4 ? 0xffffffffu : (1u << (8 * hi)) - 1u;
    return upto_hi & ~((1u << (8 * lo)) - 1u);
}

// What a team knows about its row
struct pf_row {
    const uint8_t *in;       // byte 0 of the row
    uint8_t *out;            // byte 0 of the output row (the filter-type byte)
    int n;                   // C W
    unsigned so;             // out & 15: chunk k of the row is the aligned 16 bytes at out - so + 16 k = output bytes j = 16 k - so ..
    int nk;                  // chunks that hold a byte of the output row
    bool above;              // y > 0
};

// A segment: chunks k0 .. k1 of the row, and where the row bytes they need lie in LDS (byte offset of row byte 0; may be negative)
struct pf_seg {
    int k0, k1;
    int cur0, up0;
};

// Stages row bytes lo .. hi of the row at `row` into lds: the aligned 16-byte chunks that hold them, first chunk at byte PF_FRONT.
// Returns the LDS byte offset of row byte 0.  lo == 0: whatever precedes the row in its first chunk, and the 16 bytes in front of it, read 0.
// [gb, ge): the image array; a chunk not wholly inside it is loaded byte by byte.
template <int T>
__device__ __forceinline__ int pf_stage(uint4 *lds, const uint8_t *row, int lo, int hi, uintptr_t gb, uintptr_t ge, int lane)
{
    const uintptr_t first = (uintptr_t)(row + lo);
    const unsigned s = (unsigned)(first & 15u);
    const uintptr_t base = first - s;
    const int nc = (int)((s + (unsigned)(hi - lo) + 15u) >> 4);
    for (int c = lane; c < nc; c += T) {
        const uintptr_t p = base + 16u * (uintptr_t)c;
        uint32_t v[4];
        if (p >= gb && p + 16u <= ge) {
            const uint4 q = *reinterpret_cast<const uint4 *>(p);
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        } else {
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                v[m] = 0u;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uintptr_t pe = p + (uintptr_t)(4 * m + e);
                    if (pe >= gb && pe < ge) v[m] |= (uint32_t)*reinterpret_cast<const uint8_t *>(pe) << (8 * e);
                }
            }
        }
        if (lo == 0 && c == 0) {
#pragma unroll
            for (int m = 0; m < 4; ++m) v[m] &= pf_valid(4 * m - (int)s, 16);      // bytes left of the row: 0
            lds[PF_FRONT / 16 - 1] = make_uint4(0u, 0u, 0u, 0u);
        }
        lds[PF_FRONT / 16 + c] = make_uint4(v[0], v[1], v[2], v[3]);
    }
    return PF_FRONT + (int)s - lo;
}

// Row bytes i0 - 4 .. i0 + 16 from LDS (row byte 0 at byte `at0`) as x[m] = bytes i0 + 4 m .. and l[m] = bytes i0 + 4 m - BPP ..
template <int BPP>
__device__ __forceinline__ void pf_window(const uint32_t *lds, int at0, int i0, uint32_t x[4], uint32_t l[4])
{
    const int q = at0 + i0 - 4;                 // >= 12
    const uint32_t *w = lds + (q >> 2);
    const unsigned sub = (unsigned)q & 3u;      // the same for every chunk of a row
    uint32_t g[5];
    uint32_t prev = w[0];
#pragma unroll
    for (int m = 0; m < 5; ++m) {
        const uint32_t next = w[m + 1];
        g[m] = pf_shift(prev, next, sub);
        prev = next;
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        x[m] = g[m + 1];
        l[m] = pf_shift(g[m], g[m + 1], 4 - BPP);
    }
}

// Chunk k of the row: x, a, b, c of output bytes j = 16 k - so .. + 16, i.e. row bytes i0 = j - 1 ..
template <int BPP>
__device__ __forceinline__ int pf_chunk(const pf_row &r, const pf_seg &sg, const uint32_t *cur, const uint32_t *up, int k, uint32_t x[4], uint32_t a[4],
                                        uint32_t b[4], uint32_t c[4])
{
    const int i0 = 16 * k - (int)r.so - 1;
    pf_window<BPP>(cur, sg.cur0, i0, x, a);
    pf_window<BPP>(up, sg.up0, i0, b, c);            // (row 0: whatever the buffer holds, at the current row's offsets)
    const uint32_t keep = r.above ? 0xffffffffu : 0u;
#pragma unroll
    for (int m = 0; m < 4; ++m) b[m] &= keep, c[m] &= keep;
    return i0;
}

template <int T>
struct pf_team {
    static constexpr int TEAMS = PF_THREADS / T;
    static constexpr int CAP = (T == PF_WAVE ? PF_WAVE_ROW : PF_BLOCK_ROW) + 16;      // a resident row's chunks: n + 1 + so <= CAP + 15
    static constexpr int SEGK = CAP / 16;                                             // chunks per segment
    static constexpr int LDS16 = (CAP + 128) / 16;                                    // uint4 per staged row: front, the chunks, read-ahead
};

// filter: 0..4 fixed, 5 adaptive.  rows = B H.  BPP: bytes per pixel, 1..4.
template <int T, int BPP>
__global__ __launch_bounds__(PF_THREADS) void png_filter_kernel(const uint8_t *__restrict__ img, long long rows, int H, int W, int filter,
                                                                 uint8_t *__restrict__ out)
{
    using P = pf_team<T>;
    __shared__ uint4 lds[P::TEAMS][2][P::LDS16];
    __shared__ uint32_t partial[PF_THREADS / PF_WAVE][5];
    const int team = (int)threadIdx.x / T, lane = (int)threadIdx.x % T;
    const long long row = (long long)blockIdx.x * P::TEAMS + team;
    const bool active = row < rows;                      // (an idle team still meets the block's barriers)
    const int n = BPP * W;
    pf_row r;
    r.n = n;
    r.in = img + (size_t)(active ? row : 0) * (size_t)n;
    r.out = out + (size_t)(active ? row : 0) * (size_t)(n + 1);
    r.so = (unsigned)((uintptr_t)r.out & 15u);
    r.nk = (int)((r.so + (unsigned)n + 1u + 15u) >> 4);
    r.above = (active ? row : 0) % H != 0;
    const uintptr_t gb = (uintptr_t)img, ge = gb + (size_t)rows * (size_t)n;
    uint4 *cur16 = lds[team][0], *up16 = lds[team][1];
    const uint32_t *cur = reinterpret_cast<const uint32_t *>(cur16), *up = reinterpret_cast<const uint32_t *>(up16);
    const int nseg = ((n + 31) / 16 + P::SEGK - 1) / P::SEGK;      // from the largest nk a row of n bytes can have: the same for every team
    const bool resident = nseg == 1;

    auto stage = [&](int s) {
        pf_seg sg;
        sg.k0 = s * P::SEGK;
        sg.k1 = min(sg.k0 + P::SEGK, r.nk);
        sg.cur0 = sg.up0 = 0;
        if (active && sg.k0 < sg.k1) {
            const int lo = max(0, 16 * sg.k0 - 32), hi = min(n, 16 * sg.k1);
            sg.cur0 = pf_stage<T>(cur16, r.in, lo, hi, gb, ge, lane);
            sg.up0 = r.above ? pf_stage<T>(up16, r.in - n, lo, hi, gb, ge, lane) : sg.cur0;
        }
        return sg;
    };

    int t = filter;
    pf_seg sg = stage(0);
    __syncthreads();
    if (filter == PF_ADAPTIVE) {
        uint32_t cost[5] = {0u, 0u, 0u, 0u, 0u};
        for (int s = 0;;) {
            if (active) {
                for (int k = sg.k0 + lane; k < sg.k1; k += T) {
                    uint32_t x[4], a[4], b[4], c[4];
                    const int i0 = pf_chunk<BPP>(r, sg, cur, up, k, x, a, b, c);
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        const uint32_t ok = pf_valid(i0 + 4 * m, n);
#pragma unroll
                        for (int f = 0; f < 5; ++f) cost[f] = pf_cost(pf_residual(f, x[m], a[m], b[m], c[m]) & ok, cost[f]);
                    }
                }
            }
            if (++s == nseg) break;
            __syncthreads();                             // every lane is done with the segment in LDS
            sg = stage(s);
            __syncthreads();
        }
#pragma unroll
        for (int f = 0; f < 5; ++f) {
#pragma unroll
            for (int d = PF_WAVE / 2; d >= 1; d >>= 1) cost[f] += __shfl_xor(cost[f], d, PF_WAVE);
        }
        if (T > PF_WAVE) {
            const int wave = (int)threadIdx.x / PF_WAVE;
            if ((int)threadIdx.x % PF_WAVE == 0) {
#pragma unroll
                for (int f = 0; f < 5; ++f) partial[wave][f] = cost[f];
            }
            __syncthreads();
#pragma unroll
            for (int f = 0; f < 5; ++f) {
                cost[f] = 0u;
#pragma unroll
                for (int w = 0; w < PF_THREADS / PF_WAVE; ++w) cost[f] += partial[w][f];
            }
        }
        t = 0;
        uint32_t least = cost[0];
#pragma unroll
        for (int f = 1; f < 5; ++f) {
            if (cost[f] < least) least = cost[f], t = f;      // strictly less: the smallest t keeps a tie
        }
        if (!resident) {
            __syncthreads();
            sg = stage(0);
            __syncthreads();
        }
    }
    for (int s = 0;;) {
        if (active) {
            for (int k = sg.k0 + lane; k < sg.k1; k += T) {
                uint32_t x[4], a[4], b[4], c[4], f[4];
                pf_chunk<BPP>(r, sg, cur, up, k, x, a, b, c);
#pragma unroll
                for (int m = 0; m < 4; ++m) f[m] = pf_residual(t, x[m], a[m], b[m], c[m]);
                const int j0 = 16 * k - (int)r.so;       // output byte of the chunk's byte 0
                if (k == 0) {                            // output byte 0, the filter type, is byte `so` of chunk 0
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        if (m == (int)(r.so >> 2)) f[m] = (f[m] & ~(255u << (8 * (r.so & 3u)))) | ((uint32_t)t << (8 * (r.so & 3u)));
                    }
                }
                uint8_t *p = r.out + j0;                 // 16-byte aligned
                if (j0 >= 0 && j0 + 16 <= n + 1) {
                    *reinterpret_cast<uint4 *>(p) = make_uint4(f[0], f[1], f[2], f[3]);
                } else {                                 // a chunk shared with the row before or behind (or the buffer's end): bytes
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        if (j0 + e >= 0 && j0 + e <= n) p[e] = (uint8_t)(f[e >> 2] >> (8 * (e & 3)));
                    }
                }
            }
        }
        if (++s == nseg) break;
        __syncthreads();
        sg = stage(s);
        __syncthreads();
    }
}

}  // namespace

// what the two entries share; `name`: the entry's, for the messages
template <int BPP>
static int pf_launch(const char *name, void *stream, const uint8_t *img, int B, int H, int W, int filter, uint8_t *out)
{
    FEMASR_REQUIRE(img && out, "%s: null argument", name);
    FEMASR_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: empty shape: %d images of %dx%d", name, B, H, W);
    FEMASR_REQUIRE(filter >= 0 && filter <= PF_ADAPTIVE, "%s: filter %d is not 0..4 (fixed) or 5 (adaptive)", name, filter);
    FEMASR_REQUIRE(W <= PF_MAX_ROW / BPP, "%s: a row of W = %d pixels of %d bytes is more than 3 * 2^22 bytes (32-bit offsets and cost sums inside a row)",
                   name, W, BPP);
    const long long rows = (long long)B * H;
    FEMASR_REQUIRE(rows <= (1ll << 31) - 1, "%s: %d images of %d rows are more than 2^31 - 1 rows", name, B, H);
    hipStream_t st = (hipStream_t)stream;
    if (BPP * W <= PF_WAVE_ROW) {
        const unsigned blocks = (unsigned)((rows + pf_team<PF_WAVE>::TEAMS - 1) / pf_team<PF_WAVE>::TEAMS);
        hipLaunchKernelGGL((png_filter_kernel<PF_WAVE, BPP>), dim3(blocks), dim3(PF_THREADS), 0, st, img, rows, H, W, filter, out);
    } else {
        hipLaunchKernelGGL((png_filter_kernel<PF_THREADS, BPP>), dim3((unsigned)rows), dim3(PF_THREADS), 0, st, img, rows, H, W, filter, out);
    }
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

extern "C" int femasr_png_filter_rgb8(void *stream, const uint8_t *img, int B, int H, int W, int filter, uint8_t *out)
{
    return pf_launch<3>("png_filter_rgb8", stream, img, B, H, W, filter, out);
}

extern "C" int femasr_png_filter_u8(void *stream, const uint8_t *img, int B, int H, int W, int C, int filter, uint8_t *out)
{
    switch (C) {
    case 1: return pf_launch<1>("png_filter_u8", stream, img, B, H, W, filter, out);
    case 2: return pf_launch<2>("png_filter_u8", stream, img, B, H, W, filter, out);
    case 3: return pf_launch<3>("png_filter_u8", stream, img, B, H, W, filter, out);
    case 4: return pf_launch<4>("png_filter_u8", stream, img, B, H, W, filter, out);
    default: return femasr_set_error(FEMASR_ERR_INVALID, "png_filter_u8: C = %d is not 1..4 bytes per pixel", C);
    }
}

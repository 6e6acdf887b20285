// jpeg_dct.hip — the fast JPEG output (femasr_amd/jpegio.py): colour conversion, chroma subsampling, 8x8 DCT, quantisation and
// zigzag of a uint8 image on gfx950 in ONE launch (femasr_jpeg_coefficients_u8), and - host code, no GPU - the baseline Huffman coder of the
// scan's restart intervals (femasr_jpeg_entropy_rows / _bound).
//
// Definition (jpegio.coefficients_ref; integers only, >> is the arithmetic shift).  img uint8 (H,W,C), C = 1 gray (its own Y) or 3 RGB:
//   Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
//   Cb = clip(((-11059 R - 21709 G + 32768 B + 32768) >> 16) + 128, 0, 255),  Cr likewise with (32768, -27439, -5329)
//   the last column and row replicated up to a whole MCU (8x8; 16x16 for 4:2:0);  4:2:0 chroma (a + b + c + d + 2) >> 2 per 2x2 cell
//   per 8x8 block, v = p - 128:  R[y][u] = (sum_x T[u][x] v[y][x] + 512) >> 10,  F[w][u] = (sum_y T[w][y] R[y][u] + 32768) >> 16,
//   T[u][x] = rint(8192 a(u) cos((2x + 1) u pi / 16));  k = sign(F) ((|F| + (Q >> 1)) / Q), stored at zigzag position of 8 w + u.
//
// The kernel.  A block of 256 threads takes one MCU row and a STRIP of 256 pixel columns (32 MCUs of 8x8, 16 of 16x16):
//   1. stages the strip's 8 or 16 image rows in LDS as bytes, with aligned 16-byte loads whatever the alignment of a row (the chunks of the
//      image array that hold the bytes; a chunk that is not wholly inside the array - its very first and last - byte by byte).  Rows below
//      the image stage row H - 1 again;
//   2. converts to level-unshifted int16 samples, subsamples 4:2:0 chroma from the four pixels of a cell in registers, and writes the samples
//      BLOCK-major: the 8x8 blocks of the strip's MCUs in scan order, 72 int16 (144 bytes) apart.  Columns right of the image read column W - 1;
//   3. row pass: eight lanes per block, a lane reads its row as one 16-byte LDS read (16 lanes: 256 consecutive bytes but for the 16-byte
//      gap between two blocks), transforms it in registers (even / odd halves: 32 multiplies) and writes it back in place;
//   4. column pass: a lane reads column c of its block - eight 2-byte reads; the 144-byte block pitch puts the four blocks of a 32-lane
//      half on banks 4 b + {0..3}: no conflict -, transforms, quantises by the reciprocal multipliers of the table (one 64-bit multiply per
//      coefficient; the GPU has no integer divide) and scatters the eight int16 to their zigzag places in a second LDS image, 128 bytes a block;
//   5. eight lanes write a block's 128 bytes to its place in its plane as one whole line, 16 bytes a lane.
// No workspace, no atomics, no scratch, no allocation, no synchronisation: capture-safe, on the caller's stream.  Offsets into the image and
// the planes are 64-bit (a gray plane of 46400^2 pixels has more than 2^31 coefficients).  26.8 KiB of LDS a block.
#include "common.h"
#include <string.h>

namespace {

constexpr int JQ_THREADS = 256;
constexpr int JQ_STRIP = 256;                        // pixel columns per block
constexpr int JQ_RAW_PITCH = 800;                    // bytes per staged row: 15 (misalignment) + 3 * 256 + 15, in whole 16-byte chunks: 50
constexpr int JQ_RAW_ROWS = 16;
constexpr int JQ_MAX_BLOCKS = 96;                    // 8x8 blocks per strip: 32 MCUs x 3 (4:4:4) = 16 MCUs x 6 (4:2:0); gray 32
constexpr int JQ_BLOCK_PITCH = 72;                   // int16 per staged block (64 + 8: see step 4)
constexpr int JQ_RAW_BYTES = JQ_RAW_ROWS * JQ_RAW_PITCH;
static_assert(JQ_RAW_BYTES >= JQ_MAX_BLOCKS * 128, "the zigzag image reuses the raw rows");

// T[u][x] for x < 4 (T[u][7 - x] = (-1)^u T[u][x])
__device__ constexpr int JQ_T[8][4] = {{2896, 2896, 2896, 2896}, {4017, 3406, 2276, 799}, {3784, 1567, -1567, -3784}, {3406, -799, -4017, -2276},
                                       {2896, -2896, -2896, 2896}, {2276, -4017, 799, 3406}, {1567, -3784, 3784, -1567}, {799, -2276, 3406, -4017}};
// zigzag position of natural index 8 w + u
__constant__ uint8_t JQ_ZZ_OF_NAT[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                         10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// out[u] = (sum_x T[u][x] v[x] + half) >> shift
__device__ __forceinline__ void jq_dct8(const int v[8], int out[8], int half, int shift)
{
    int s[4], d[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) s[x] = v[x] + v[7 - x], d[x] = v[x] - v[7 - x];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        int acc = half;
#pragma unroll
        for (int x = 0; x < 4; ++x) acc += JQ_T[u][x] * ((u & 1) ? d[x] : s[x]);
        out[u] = acc >> shift;
    }
}

struct jq_args {
    const uint8_t *img;
    int H, W;
    int mcus_x;              // MCUs per row of the image
    const uint32_t *qtab[2];
    int16_t *out[3];
};

// C: 1 / 3 channels.  SUB: 4:2:0 (C = 3 only).  An MCU is M x M pixels and BPM blocks; a strip holds MPS MCUs.
template <int C, bool SUB>
__global__ __launch_bounds__(JQ_THREADS) void jpeg_coefficients_kernel(jq_args a)
{
    constexpr int M = SUB ? 16 : 8, BPM = C == 1 ? 1 : (SUB ? 6 : 3), MPS = JQ_STRIP / M, ROWS = M;
    __shared__ uint4 raw16[JQ_RAW_BYTES / 16];
    __shared__ uint4 blk16[JQ_MAX_BLOCKS * JQ_BLOCK_PITCH * 2 / 16];
    __shared__ uint32_t qt[2][128];
    uint8_t *raw = reinterpret_cast<uint8_t *>(raw16);
    int16_t *blk = reinterpret_cast<int16_t *>(blk16);
    int16_t *zz = reinterpret_cast<int16_t *>(raw16);        // (step 4 on: the raw rows are dead)
    const int tid = (int)threadIdx.x;
    const int strip = (int)blockIdx.x, mrow = (int)blockIdx.y;
    const int H = a.H, W = a.W;
    const int x0 = strip * JQ_STRIP, y0 = mrow * M;
    const int nv = min(W - x0, JQ_STRIP);                    // image columns in the strip (>= 1)
    const int nm = min(a.mcus_x - strip * MPS, MPS);         // MCUs in the strip (>= 1)
    const int nblk = nm * BPM;
    const uintptr_t gb = (uintptr_t)a.img, ge = gb + (size_t)H * (size_t)W * C;

    if (tid < 128) qt[0][tid] = a.qtab[0][tid];
    else if (C == 3) qt[1][tid - 128] = a.qtab[1][tid - 128];

    // 1. the rows, as the aligned 16-byte chunks that hold them
    auto row_ptr = [&](int r) { return gb + ((size_t)min(y0 + r, H - 1) * (size_t)W + (size_t)x0) * C; };
    for (int i = tid; i < ROWS * (JQ_RAW_PITCH / 16); i += JQ_THREADS) {
        const int r = i / (JQ_RAW_PITCH / 16), c = i % (JQ_RAW_PITCH / 16);
        const uintptr_t first = row_ptr(r);
        const unsigned s = (unsigned)(first & 15u);
        const int nc = (int)((s + (unsigned)(nv * C) + 15u) >> 4);            // <= 50
        if (c >= nc) continue;
        const uintptr_t p = first - s + 16u * (uintptr_t)c;
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
        raw16[r * (JQ_RAW_PITCH / 16) + c] = make_uint4(v[0], v[1], v[2], v[3]);
    }
    __syncthreads();

    // 2. samples, block-major.  px(r, x): the bytes of pixel x of the strip (clamped to the image) in staged row r
    auto px = [&](int r, int x) { return raw + r * JQ_RAW_PITCH + (int)(row_ptr(r) & 15u) + min(x, nv - 1) * C; };
    if (!SUB) {
        const int x = tid;
        if (x < nm * 8) {
            int16_t *dst = blk + (x >> 3) * BPM * JQ_BLOCK_PITCH + (x & 7);
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const uint8_t *p = px(r, x);
                if (C == 1) {
                    dst[r * 8] = (int16_t)p[0];
                } else {
                    const int R = p[0], G = p[1], B = p[2];
                    dst[r * 8] = (int16_t)((19595 * R + 38470 * G + 7471 * B + 32768) >> 16);
                    dst[JQ_BLOCK_PITCH + r * 8] = (int16_t)clampi(((-11059 * R - 21709 * G + 32768 * B + 32768) >> 16) + 128, 0, 255);
                    dst[2 * JQ_BLOCK_PITCH + r * 8] = (int16_t)clampi(((32768 * R - 27439 * G - 5329 * B + 32768) >> 16) + 128, 0, 255);
                }
            }
        }
    } else {
        const int cx = tid & 127;                            // a 2x2 cell: pixels (2 cy + dy, 2 cx + dx)
        if (cx < nm * 8) {
            int16_t *mcu = blk + (cx >> 3) * BPM * JQ_BLOCK_PITCH;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int cy = (tid >> 7) + 2 * i;
                int cb = 2, cr = 2;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = 2 * cy + (e >> 1), x = 2 * cx + (e & 1);
                    const uint8_t *p = px(r, x);
                    const int R = p[0], G = p[C > 1 ? 1 : 0], B = p[C > 1 ? 2 : 0];
                    mcu[(((r >> 3) << 1) + ((x >> 3) & 1)) * JQ_BLOCK_PITCH + (r & 7) * 8 + (x & 7)] =
                        (int16_t)((19595 * R + 38470 * G + 7471 * B + 32768) >> 16);
                    cb += clampi(((-11059 * R - 21709 * G + 32768 * B + 32768) >> 16) + 128, 0, 255);
                    cr += clampi(((32768 * R - 27439 * G - 5329 * B + 32768) >> 16) + 128, 0, 255);
                }
                mcu[4 * JQ_BLOCK_PITCH + cy * 8 + (cx & 7)] = (int16_t)(cb >> 2);
                mcu[5 * JQ_BLOCK_PITCH + cy * 8 + (cx & 7)] = (int16_t)(cr >> 2);
            }
        }
    }
    __syncthreads();

    // 3. row pass, in place
    for (int w = tid; w < nblk * 8; w += JQ_THREADS) {
        uint4 *row = reinterpret_cast<uint4 *>(blk + (w >> 3) * JQ_BLOCK_PITCH + (w & 7) * 8);
        const uint4 q = *row;
        const uint32_t d[4] = {q.x, q.y, q.z, q.w};
        int v[8], o[8];
#pragma unroll
        for (int m = 0; m < 4; ++m) v[2 * m] = (int)(d[m] & 0xffffu) - 128, v[2 * m + 1] = (int)(d[m] >> 16) - 128;
        jq_dct8(v, o, 512, 10);
        uint32_t e[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) e[m] = ((uint32_t)o[2 * m] & 0xffffu) | ((uint32_t)o[2 * m + 1] << 16);
        *row = make_uint4(e[0], e[1], e[2], e[3]);
    }
    __syncthreads();

    // 4. column pass, quantisation, zigzag
    for (int w = tid; w < nblk * 8; w += JQ_THREADS) {
        const int b = w >> 3, c = w & 7;
        const int16_t *col = blk + b * JQ_BLOCK_PITCH + c;
        int v[8], o[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) v[y] = col[y * 8];
        jq_dct8(v, o, 32768, 16);
        const int k = b % BPM;
        const uint32_t *t = qt[(C == 3 && k >= (SUB ? 4 : 1)) ? 1 : 0];
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            const int z = JQ_ZZ_OF_NAT[8 * y + c];
            const uint32_t n = (uint32_t)abs(o[y]) + (t[z] >> 1);
            const int quo = (int)(((uint64_t)n * (uint64_t)t[64 + z]) >> 24);
            zz[b * 64 + z] = (int16_t)(o[y] < 0 ? -quo : quo);
        }
    }
    __syncthreads();

    // 5. whole 128-byte lines
    for (int w = tid; w < nblk * 8; w += JQ_THREADS) {
        const int b = w >> 3, part = w & 7;
        const int mcu = strip * MPS + b / BPM, k = b % BPM;
        int16_t *plane;
        size_t by, bx, wb;
        if (SUB && k < 4) {
            plane = a.out[0], by = 2 * (size_t)mrow + (size_t)(k >> 1), bx = 2 * (size_t)mcu + (size_t)(k & 1), wb = 2 * (size_t)a.mcus_x;
        } else {
            plane = a.out[SUB ? k - 3 : k], by = (size_t)mrow, bx = (size_t)mcu, wb = (size_t)a.mcus_x;
        }
        *reinterpret_cast<uint4 *>(plane + (by * wb + bx) * 64 + (size_t)part * 8) = reinterpret_cast<const uint4 *>(zz)[w];
    }
}

template <int C, bool SUB>
int jq_launch(hipStream_t st, const jq_args &a, int mcu_rows)
{
    constexpr int MPS = JQ_STRIP / (SUB ? 16 : 8);
    hipLaunchKernelGGL((jpeg_coefficients_kernel<C, SUB>), dim3((unsigned)((a.mcus_x + MPS - 1) / MPS), (unsigned)mcu_rows), dim3(JQ_THREADS), 0, st, a);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

}  // namespace

extern "C" int femasr_jpeg_coefficients_u8(const uint8_t *img, int H, int W, int C, int subsampling, const uint32_t *qtab_y, const uint32_t *qtab_c,
                                           int16_t *out_y, int16_t *out_cb, int16_t *out_cr, void *stream)
{
    FEMASR_REQUIRE(C == 1 || C == 3, "jpeg_coefficients_u8: C = %d is not 1 (gray) or 3 (RGB)", C);
    FEMASR_REQUIRE(C == 1 || subsampling == 444 || subsampling == 420, "jpeg_coefficients_u8: subsampling %d is not 444 or 420", subsampling);
    FEMASR_REQUIRE(H >= 1 && W >= 1 && H <= 65535 && W <= 65535, "jpeg_coefficients_u8: %dx%d is outside 1..65535 pixels a side", H, W);
    FEMASR_REQUIRE(img && qtab_y && out_y, "jpeg_coefficients_u8: null argument");
    FEMASR_REQUIRE(C == 3 ? (qtab_c && out_cb && out_cr) : (!out_cb && !out_cr),
                   "jpeg_coefficients_u8: C = %d takes %s", C, C == 3 ? "qtab_c, out_cb and out_cr" : "neither out_cb nor out_cr");
    FEMASR_REQUIRE((((uintptr_t)out_y | (uintptr_t)out_cb | (uintptr_t)out_cr) & 15u) == 0, "jpeg_coefficients_u8: the output planes must be 16-byte aligned");
    const bool sub = C == 3 && subsampling == 420;
    const int m = sub ? 16 : 8;
    jq_args a;
    a.img = img, a.H = H, a.W = W, a.mcus_x = (W + m - 1) / m;
    a.qtab[0] = qtab_y, a.qtab[1] = qtab_c;
    a.out[0] = out_y, a.out[1] = out_cb, a.out[2] = out_cr;
    const int mcu_rows = (H + m - 1) / m;                    // <= 8192: a grid's y extent
    hipStream_t st = (hipStream_t)stream;
    if (C == 1) return jq_launch<1, false>(st, a, mcu_rows);
    return sub ? jq_launch<3, true>(st, a, mcu_rows) : jq_launch<3, false>(st, a, mcu_rows);
}

// ---- the scan: host code ----
namespace {

const uint8_t JH_DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t JH_DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t JH_AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const uint8_t JH_AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
     0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
     0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
     0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
     0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
     0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
     0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
     0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// symbol -> code and length, as Annex C builds them from (BITS, HUFFVAL)
struct jh_table {
    uint16_t code[256];
    uint8_t len[256];
    void build(const uint8_t bits[16], const uint8_t *vals)
    {
        memset(code, 0, sizeof code);
        memset(len, 0, sizeof len);
        unsigned c = 0;
        int k = 0;
        for (int l = 1; l <= 16; ++l) {
            for (int i = 0; i < bits[l - 1]; ++i, ++k, ++c) code[vals[k]] = (uint16_t)c, len[vals[k]] = (uint8_t)l;
            c <<= 1;
        }
    }
};
struct jh_tables {
    jh_table dc[2], ac[2];
    jh_tables()
    {
        for (int t = 0; t < 2; ++t) dc[t].build(JH_DC_BITS[t], JH_DC_VALS), ac[t].build(JH_AC_BITS[t], JH_AC_VALS[t]);
    }
};
const jh_tables &jh_get()
{
    static const jh_tables t;        // (initialised once, thread-safe)
    return t;
}

// Bits into bytes, 0xFF stuffed; never writes at or behind `end` (`full` says that it would have)
struct jh_bits {
    uint8_t *p, *end;
    uint64_t acc = 0;
    int n = 0;
    bool full = false;
    void byte(unsigned b)
    {
        if (p < end) *p++ = (uint8_t)b;
        else full = true;
    }
    void put(unsigned code, int len)
    {
        acc = (acc << len) | code;
        n += len;
        while (n >= 8) {
            const unsigned b = (unsigned)(acc >> (n - 8)) & 0xffu;
            byte(b);
            if (b == 0xffu) byte(0u);
            n -= 8;
        }
    }
    void pad()
    {
        if (n) put((1u << (8 - n)) - 1u, 8 - n);
    }
};

inline int jh_category(int v)
{
    unsigned a = (unsigned)(v < 0 ? -v : v);
    int s = 0;
    while (a) ++s, a >>= 1;
    return s;
}

// one block; false: a coefficient outside baseline JPEG
inline bool jh_block(jh_bits &w, const int16_t *blk, int *pred, const jh_table &dc, const jh_table &ac)
{
    const int diff = (int)blk[0] - *pred;
    *pred = blk[0];
    int size = jh_category(diff);
    if (size > 11) return false;
    w.put(dc.code[size], dc.len[size]);
    if (size) w.put((unsigned)(diff > 0 ? diff : diff - 1) & ((1u << size) - 1u), size);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = blk[k];
        if (v == 0) {
            ++run;
            continue;
        }
        for (; run > 15; run -= 16) w.put(ac.code[0xf0], ac.len[0xf0]);
        size = jh_category(v);
        if (size > 10) return false;
        const int sym = (run << 4) | size;
        w.put(ac.code[sym], ac.len[sym]);
        w.put((unsigned)(v > 0 ? v : v - 1) & ((1u << size) - 1u), size);
        run = 0;
    }
    if (run) w.put(ac.code[0], ac.len[0]);
    return true;
}

// 0: the arguments are no image layout; else blocks per MCU
inline int jh_blocks_per_mcu(int components, int subsampling)
{
    if (components == 1) return 1;
    if (components != 3) return 0;
    return subsampling == 444 ? 3 : (subsampling == 420 ? 6 : 0);
}

constexpr size_t JH_BLOCK_BYTES = 420;      // DC <= 16 + 11 bits, 63 AC of <= 16 + 10: 1665 bits = 209 bytes, every one stuffed: 418

}  // namespace

extern "C" size_t femasr_jpeg_entropy_bound(int mcus_per_row, int components, int subsampling, int rows)
{
    const int bpm = jh_blocks_per_mcu(components, subsampling);
    if (!bpm || mcus_per_row < 1 || mcus_per_row > 8192 || rows < 1 || rows > 8192) return 0;
    return (size_t)rows * ((size_t)mcus_per_row * (size_t)bpm * JH_BLOCK_BYTES + 4);
}

extern "C" long long femasr_jpeg_entropy_rows(const int16_t *y, const int16_t *cb, const int16_t *cr, int components, int subsampling,
                                              int mcu_rows, int mcus_per_row, int row0, int row1, uint8_t *out, size_t capacity)
{
    const int bpm = jh_blocks_per_mcu(components, subsampling);
    FEMASR_REQUIRE(bpm, "jpeg_entropy_rows: %d components with subsampling %d is not gray, 444 or 420", components, subsampling);
    FEMASR_REQUIRE(mcu_rows >= 1 && mcu_rows <= 8192 && mcus_per_row >= 1 && mcus_per_row <= 8192,
                   "jpeg_entropy_rows: %d x %d MCUs is outside 1..8192 a side", mcu_rows, mcus_per_row);
    FEMASR_REQUIRE(0 <= row0 && row0 < row1 && row1 <= mcu_rows, "jpeg_entropy_rows: rows %d..%d of %d", row0, row1, mcu_rows);
    FEMASR_REQUIRE(y && out && (components == 3 ? (cb && cr) : (!cb && !cr)), "jpeg_entropy_rows: a missing or surplus pointer");
    const jh_tables &t = jh_get();
    const int f = bpm == 6 ? 2 : 1;
    const size_t wy = (size_t)f * (size_t)mcus_per_row;      // blocks per row of the Y plane
    jh_bits w;
    w.p = out, w.end = out + capacity;
    for (int row = row0; row < row1; ++row) {
        int pred[3] = {0, 0, 0};
        bool ok = true;
        for (int m = 0; m < mcus_per_row && ok; ++m) {
            for (int dy = 0; dy < f && ok; ++dy) {
                for (int dx = 0; dx < f && ok; ++dx)
                    ok = jh_block(w, y + (((size_t)f * row + dy) * wy + (size_t)f * m + dx) * 64, &pred[0], t.dc[0], t.ac[0]);
            }
            if (components == 3 && ok) {
                const size_t at = ((size_t)row * mcus_per_row + m) * 64;
                ok = jh_block(w, cb + at, &pred[1], t.dc[1], t.ac[1]) && jh_block(w, cr + at, &pred[2], t.dc[1], t.ac[1]);
            }
        }
        FEMASR_REQUIRE(ok, "jpeg_entropy_rows: MCU row %d holds a coefficient outside baseline JPEG (a DC difference beyond 11 bits or an AC value beyond 10)", row);
        w.pad();
        if (row != mcu_rows - 1) w.byte(0xffu), w.byte(0xd0u + (unsigned)(row & 7));
        FEMASR_REQUIRE(!w.full, "jpeg_entropy_rows: %zu bytes do not hold MCU rows %d..%d (femasr_jpeg_entropy_bound gives a size that does)", capacity, row0, row1);
    }
    return (long long)(w.p - out);
}

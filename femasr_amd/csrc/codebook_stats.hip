// codebook_stats.hip — code-usage histogram of codebook index maps (femasr_amd/codebook.py) on gfx950.
//
// Definition: counts[g][c] = #{ t : indices[g][t] == c }, c in [0, n_e); invalid[g] = #{ t : indices[g][t] outside [0, n_e) }, compared on
// the full 64 bits (2^32 + 5 is invalid, not code 5).  counts[g].sum() + invalid[g] == M.  Integers only: exact, whatever the order.
//
// Two launches on the caller's stream, no global atomics, no memset of an output, no allocation, no synchronisation (capture-safe):
//   1. partial: grid (nb, G), 256 threads.  Block (b, g) owns tokens [b tok, min(M, (b+1) tok)) of group g and walks the bins in chunks of
//      HIST_CHUNK: zero the LDS counters, read its tokens (16-byte loads of two indices where the slice starts on 16 bytes, after one
//      single index where it does not; consecutive lanes read consecutive pairs), add 1 to the LDS counter of every index inside the chunk
//      (integer LDS atomics), write the chunk's counters to its own row of the workspace.  The first chunk also counts what is out of
//      range, in one more counter.  A block reads its tokens once per chunk: n_e <= HIST_CHUNK (every codebook of the networks) is one pass.
//      Row layout: part[(g nb + b)(n_e + 1) + c], c == n_e: the invalid count; uint32 (a block owns at most 2^31 tokens).
//   2. reduce: grid (ceil((n_e + 1) / 64), G), 1024 threads = 64 columns x 16 row groups.  Thread (c, r) sums part[g][r, r + 16, ...][c] in
//      ascending order in 64 bits; the 16 sums of a column meet in LDS and are added in ascending r - one fixed order - and written to
//      counts / invalid.  Consecutive lanes read consecutive words.  Every element of counts and invalid is written by this launch.
// nb is chosen from the shapes alone (hist_plan): about 8192 tokens per block, at most HIST_MAX_BLOCKS blocks in all groups together and at
// most HIST_MAX_PART_WORDS partial words where the shape allows.
#include <algorithm>

#include "common.h"

namespace {

constexpr int HIST_THREADS = 256;
constexpr int HIST_RCOLS = 64, HIST_RROWS = 16;      // reduce: columns per block x row groups (1024 threads)
constexpr int HIST_CHUNK = 4096;                     // bins per walk: 16 KiB of LDS counters
constexpr int HIST_MAX_NE = 1 << 20;                 // 256 walks; beyond it FEMASR_ERR_INVALID
constexpr long long HIST_TOK = 8192;                 // tokens a block takes at least (but for the last block of a group)
constexpr long long HIST_MAX_BLOCKS = 1024;
constexpr long long HIST_MAX_PART_WORDS = 1ll << 24; // 64 MiB of partials, exceeded only when G (n_e + 1) alone exceeds it
constexpr long long HIST_MAX_TOK = 1ll << 31;        // a uint32 counter cannot overflow

struct HistPlan { long long tok; int nb; };

// shapes -> tokens per block and blocks per group; the workspace query and the launch share it
HistPlan hist_plan(int G, long long M, int n_e)
{
    long long nb = (M + HIST_TOK - 1) / HIST_TOK;
    nb = std::min(nb, std::max(1ll, HIST_MAX_BLOCKS / G));
    nb = std::min(nb, std::max(1ll, HIST_MAX_PART_WORDS / ((long long)G * (n_e + 1))));
    const long long tok = (M + nb - 1) / nb;
    return HistPlan{tok, (int)((M + tok - 1) / tok)};      // every block owns at least one token
}

__device__ __forceinline__ void hist_count(long long v, long long c0, int cn, int n_e, bool first, uint32_t *bins, uint32_t &inv)
{
    const unsigned long long u = (unsigned long long)v - (unsigned long long)c0;       // v < c0 wraps far above cn
    if (u < (unsigned long long)cn) atomicAdd(&bins[(int)u], 1u);
    else if (first && (unsigned long long)v >= (unsigned long long)n_e) ++inv;          // negative, or >= n_e, on 64 bits
}

__global__ __launch_bounds__(HIST_THREADS) void index_hist_partial_kernel(const long long *__restrict__ idx, long long M, int n_e, long long tok,
                                                                          int nb, uint32_t *__restrict__ part)
{
    __shared__ uint32_t bins[HIST_CHUNK + 1];        // [HIST_CHUNK]: out of range
    const int b = (int)blockIdx.x, g = (int)blockIdx.y, tid = (int)threadIdx.x;
    const long long t0 = (long long)b * tok;
    const long long n = (M - t0 < tok ? M - t0 : tok);       // >= 1 (hist_plan)
    const long long *p = idx + (size_t)g * (size_t)M + (size_t)t0;
    uint32_t *row = part + ((size_t)g * (size_t)nb + (size_t)b) * (size_t)(n_e + 1);
    const long long head = (((uintptr_t)p & 15) != 0 && n > 0) ? 1 : 0;      // one index in front of the 16-byte pairs
    const long long npair = n > head ? (n - head) >> 1 : 0;
    const bool tail = n > head && ((n - head) & 1);
    const longlong2 *p2 = reinterpret_cast<const longlong2 *>(p + head);
    for (long long c0 = 0; c0 < n_e; c0 += HIST_CHUNK) {
        const int cn = n_e - c0 < HIST_CHUNK ? (int)(n_e - c0) : HIST_CHUNK;
        const bool first = c0 == 0;
        for (int i = tid; i < cn; i += HIST_THREADS) bins[i] = 0u;
        if (tid == 0) bins[HIST_CHUNK] = 0u;
        __syncthreads();
        uint32_t inv = 0u;
        if (tid == 0 && head) hist_count(p[0], c0, cn, n_e, first, bins, inv);
        if (tid == 1 && tail) hist_count(p[n - 1], c0, cn, n_e, first, bins, inv);
        long long i = tid;
        for (; i + 3 * HIST_THREADS < npair; i += 4 * HIST_THREADS) {        // four loads in flight per lane before the first counter moves
            longlong2 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = p2[i + u * HIST_THREADS];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                hist_count(v[u].x, c0, cn, n_e, first, bins, inv);
                hist_count(v[u].y, c0, cn, n_e, first, bins, inv);
            }
        }
        for (; i < npair; i += HIST_THREADS) {
            const longlong2 v = p2[i];
            hist_count(v.x, c0, cn, n_e, first, bins, inv);
            hist_count(v.y, c0, cn, n_e, first, bins, inv);
        }
        if (inv) atomicAdd(&bins[HIST_CHUNK], inv);
        __syncthreads();
        for (int i = tid; i < cn; i += HIST_THREADS) row[(size_t)c0 + i] = bins[i];
        if (first && tid == 0) row[n_e] = bins[HIST_CHUNK];
        __syncthreads();
    }
}

// Block (x, g): HIST_RCOLS consecutive columns of group g.  Thread (col, r) sums rows r, r + HIST_RROWS, ... of its column in ascending
// order; the HIST_RROWS sums of a column are then added in ascending r: one fixed order for every shape.
__global__ __launch_bounds__(HIST_RCOLS * HIST_RROWS) void index_hist_reduce_kernel(const uint32_t *__restrict__ part, int n_e, int nb,
                                                                                    long long *__restrict__ counts, long long *__restrict__ invalid)
{
    __shared__ long long sums[HIST_RROWS][HIST_RCOLS];
    const int cols = n_e + 1, g = (int)blockIdx.y;
    const int lane = (int)threadIdx.x % HIST_RCOLS, r = (int)threadIdx.x / HIST_RCOLS;
    const int c = (int)blockIdx.x * HIST_RCOLS + lane;
    long long acc = 0;
    if (c < cols) {
        const uint32_t *col = part + (size_t)g * (size_t)nb * (size_t)cols + (size_t)c;
#pragma unroll 8
        for (int b = r; b < nb; b += HIST_RROWS) acc += (long long)col[(size_t)b * (size_t)cols];
    }
    sums[r][lane] = acc;
    __syncthreads();
    if (r != 0 || c >= cols) return;
    long long tot = 0;
#pragma unroll
    for (int k = 0; k < HIST_RROWS; ++k) tot += sums[k][lane];
    if (c == n_e) invalid[g] = tot;
    else counts[(size_t)g * (size_t)n_e + (size_t)c] = tot;
}

int hist_check(const char *who, int G, int64_t M, int n_e)
{
    FEMASR_REQUIRE(G >= 1 && M >= 1 && n_e >= 1, "%s: empty shape: %d groups of %lld tokens, %d codes", who, G, (long long)M, n_e);
    FEMASR_REQUIRE(n_e <= HIST_MAX_NE, "%s: n_e = %d is more than the %d codes the kernel walks", who, n_e, HIST_MAX_NE);
    FEMASR_REQUIRE(G <= 65535, "%s: %d groups are more than 65535 (grid.y)", who, G);
    const HistPlan pl = hist_plan(G, M, n_e);
    FEMASR_REQUIRE(pl.tok <= HIST_MAX_TOK, "%s: %lld tokens per group are more than a block's 32-bit counters hold", who, (long long)M);
    return FEMASR_OK;
}

}  // namespace

extern "C" int femasr_index_histogram_workspace_bytes(int G, int64_t M, int n_e, size_t *bytes)
{
    FEMASR_REQUIRE(bytes, "index_histogram_workspace_bytes: null argument");
    FEMASR_CHECK(hist_check("index_histogram_workspace_bytes", G, M, n_e));
    const HistPlan pl = hist_plan(G, M, n_e);
    *bytes = (size_t)G * (size_t)pl.nb * (size_t)(n_e + 1) * sizeof(uint32_t);
    return FEMASR_OK;
}

extern "C" int femasr_index_histogram(void *stream, const int64_t *indices, int G, int64_t M, int n_e, int64_t *counts, int64_t *invalid,
                                      void *ws, size_t ws_bytes)
{
    FEMASR_REQUIRE(indices && counts && invalid && ws, "index_histogram: null argument");
    FEMASR_CHECK(hist_check("index_histogram", G, M, n_e));
    FEMASR_REQUIRE(((uintptr_t)indices & 7) == 0 && ((uintptr_t)counts & 7) == 0 && ((uintptr_t)invalid & 7) == 0 && ((uintptr_t)ws & 3) == 0,
                   "index_histogram: int64 arrays must start on 8 bytes, the workspace on 4");
    const HistPlan pl = hist_plan(G, M, n_e);
    const size_t need = (size_t)G * (size_t)pl.nb * (size_t)(n_e + 1) * sizeof(uint32_t);
    FEMASR_REQUIRE(ws_bytes >= need, "index_histogram: workspace of %zu bytes, %zu needed (femasr_index_histogram_workspace_bytes)", ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(index_hist_partial_kernel, dim3((unsigned)pl.nb, (unsigned)G), dim3(HIST_THREADS), 0, st, (const long long *)indices,
                       (long long)M, n_e, pl.tok, pl.nb, (uint32_t *)ws);
    FEMASR_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(index_hist_reduce_kernel, dim3((unsigned)((n_e + 1 + HIST_RCOLS - 1) / HIST_RCOLS), (unsigned)G), dim3(HIST_RCOLS * HIST_RROWS), 0, st,
                       (const uint32_t *)ws, n_e, pl.nb, (long long *)counts, (long long *)invalid);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

// kernels_probe.hip — the sustained-clock probe (bench.py): every wave streams back-to-back v_mfma_f32_32x32x2_f32 (64 shader cycles each: the load the
// network's hot kernels put on the chip) and records the s_memtime ticks (= shader cycles) its loop took; ticks / wall time of
// the launch = the clock the chip sustains under that load right now.
//
// math_eval_kernel: the device's elementary functions on their own (detmath.h, fast_silu of halo_mma.h), one value or pair per thread,
// so that tests/test_gpu_math_range.py can hold them to the oracle over all of fp32 instead of through a kernel's data.
#include "common.h"
#include "detmath.h"
#include "halo_mma.h"

typedef float probe_f32x16 __attribute__((ext_vector_type(16)));
__global__ __launch_bounds__(256) void clock_probe_kernel(int groups, float a, float b, unsigned long long *ticks)
{
    probe_f32x16 c0 = {0}, c1 = {0}, c2 = {0}, c3 = {0};
    a += (float)(threadIdx.x & 31) * 0.03125f;        // operands differ from lane to lane (tools/power_probe.py reads the package power under this loop)
    b += (float)((threadIdx.x >> 5) & 1) * 0.25f;
    const unsigned long long t0 = __builtin_readcyclecounter();
    for (int i = 0; i < groups; ++i) {
        c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c1, 0, 0, 0);
        c2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c2, 0, 0, 0);
        c3 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c3, 0, 0, 0);
    }
    float s = 0.f;
    for (int r = 0; r < 16; ++r) s += c0[r] + c1[r] + c2[r] + c3[r];
    const unsigned long long t1 = __builtin_readcyclecounter();
    if ((threadIdx.x & 63) == 0) ticks[blockIdx.x * 4 + (threadIdx.x >> 6)] = (t1 - t0) + (s == 12345.678f ? 1ull : 0ull);
}

// fn 0-3: det_expf / det_erff / det_silu / det_gelu of x[i];  4-7: their packed forms on the pairs (x[2i], x[2i+1]);  8: fast_silu.
// `items` counts values (fn < 4, fn 8) or pairs (fn 4-7).
__global__ __launch_bounds__(256) void math_eval_kernel(int fn, const float *__restrict__ x, long long items, float *__restrict__ y)
{
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += stride) {
        if (fn >= 4 && fn < 8) {
            const float2 v = *reinterpret_cast<const float2 *>(x + 2 * i);
            const det_f32x2 p = {v.x, v.y};
            const det_f32x2 r = fn == 4 ? det_expf2(p) : fn == 5 ? det_erff2(p) : fn == 6 ? det_silu2(p) : det_gelu2(p);
            *reinterpret_cast<float2 *>(y + 2 * i) = make_float2(r[0], r[1]);
        } else {
            const float v = x[i];
            y[i] = fn == 0 ? det_expf(v) : fn == 1 ? det_erff(v) : fn == 2 ? det_silu(v) : fn == 3 ? det_gelu(v) : fast_silu(v);
        }
    }
}

extern "C" {

int femasr_clock_probe_entries(void) { return FEMASR_CLOCK_PROBE_BLOCKS * 4; }      // what femasr_clock_probe writes: one tick count per wave

int femasr_clock_probe(void *stream, int mfmas_per_wave, unsigned long long *ticks)
{
    FEMASR_REQUIRE(ticks && mfmas_per_wave >= 4, "clock_probe: bad args");
    hipLaunchKernelGGL(clock_probe_kernel, dim3(FEMASR_CLOCK_PROBE_BLOCKS), dim3(256), 0, (hipStream_t)stream, mfmas_per_wave / 4, 1.0001f, 0.5f, ticks);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

int femasr_debug_math_eval(void *stream, int fn, const float *x, long long n, float *y)
{
    FEMASR_REQUIRE(x && y && n > 0 && fn >= 0 && fn <= 8, "debug_math_eval: bad args");
    const bool pairs = fn >= 4 && fn < 8;
    FEMASR_REQUIRE(!pairs || n % 2 == 0, "debug_math_eval: the packed forms take an even n");
    const long long items = pairs ? n / 2 : n;
    hipLaunchKernelGGL(math_eval_kernel, dim3(grid_for((size_t)items)), dim3(256), 0, (hipStream_t)stream, fn, x, items, y);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

}  // extern "C"

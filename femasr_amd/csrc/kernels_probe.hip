// kernels_probe.hip — the sustained-clock probe (bench.py): every wave streams back-to-back v_mfma_f32_32x32x2_f32 (64 shader cycles each: the load the
// network's hot kernels put on the chip) and records the s_memtime ticks (= shader cycles) its loop took; ticks / wall time of
// the launch = the clock the chip sustains under that load right now.
#include "common.h"

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

extern "C" {

int femasr_clock_probe_entries(void) { return FEMASR_CLOCK_PROBE_BLOCKS * 4; }      // what femasr_clock_probe writes: one tick count per wave

int femasr_clock_probe(void *stream, int mfmas_per_wave, unsigned long long *ticks)
{
    FEMASR_REQUIRE(ticks && mfmas_per_wave >= 4, "clock_probe: bad args");
    hipLaunchKernelGGL(clock_probe_kernel, dim3(FEMASR_CLOCK_PROBE_BLOCKS), dim3(256), 0, (hipStream_t)stream, mfmas_per_wave / 4, 1.0001f, 0.5f, ticks);
    FEMASR_CHECK_HIP(hipGetLastError());
    return FEMASR_OK;
}

}  // extern "C"

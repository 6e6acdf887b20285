// kernels_wino_up2.hip — nn.Upsample(x2, nearest) + 3x3 stride-1 pad-1 conv (femasr_arch.py:172-173,202-203) in a
// Winograd-type minimal form on the fp32 matrix cores: 25 multiplies per 4x4 outputs.
//
// A 4x4 tile of the OUTPUT (upsampled grid) reads a 6x6 patch of the upsampled image, i.e. only a 4x4 patch of the
// low-resolution input: per dimension d = (l0, l1, l1, l2, l2, l3).  Put through the F(4,3) input transform B^T that gives
//     r0 = 4 l0 - 5 l1 + l2,   r1 = 2 (l2 - 4 l1),   r2 = 0,   r3 = 3 (l2 - l1),   r4 = -(l2 - l1),   r5 = 4 l1 - 5 l2 + l3
// - one component vanishes and two are proportional, so per dimension FIVE products are enough for four outputs:
//     v0 = fma(4, l0, fma(-5, l1, l2))   v1 = fma(-4, l1, l2)   v3 = l2 - l1   v5 = fma(4, l1, fma(-5, l2, l3))
//     e0 = g0/4   e1 = -((g0 + g1) + g2)/3   eP = fma(4, g2, fma(4, g1, g0))/12   eQ = fma(4, g2, g0 + g1)/6   e5 = g2
//     m0 = e0 v0,  m1 = e1 v1,  mP = eP v3,  mQ = eQ v3,  m5 = e5 v5          (each summed over the input channels)
//     y0 = (m0 + m1) + mP    y1 = fma(2, mQ, m1)    y2 = fma(4, mP, m1)    y3 = fma(8, mQ, m1) + m5
// (the constants 2, 3 and -1 of r1, r3, r4 are folded into the filters).  In 2-D: 25 products per 16 outputs and channel
// pair where the phase-filter form of kernels_conv.hip needs 64 and the definition 144.  Like the F(4x4,3x3) kernel this is
// only used behind the codebook lookup of single-codebook networks; all fp32, every value one fixed sequence of IEEE
// operations restated by oracle/femasr_oracle.c orc_conv_up2_winograd.
//
// Structure = kernels_wino.hip (read its header first): block = 8 waves, two 16x16-pixel OUTPUT sub-blocks (= 2 x 16 tiles =
// one 32-row MFMA tile) x 64 output channels, K in steps of 8 input channels, every wave M phase then T phase, one barrier
// per step; the block decode and the shared parts of the epilogue are WinoFrame (wino_common.h).  What differs:
//   staging   the 10x10 low-resolution patch of a sub-block (8x8 + halo), plain copy (these convs have no GN prologue)
//   T phase   thread = (tile, channel, half): 12 LDS reads -> 8 of the 16 DISTINCT transformed values V[4][4] (components P and
//             Q share v3): V[16][32 tiles][8 channels]
//   M phase   50 (component, 32-column tile) pairs: wave w owns column tile w&1 of components w/2 + 4q, q = 0..5 (waves 0, 1
//             also q = 6): 13 / 13 / 12 / 12 pairs per SIMD
//   epilogue  (wino_common.h) Mx[25][32][32] per column tile, the 5 -> 4 output transform (at5) twice
#define FEMASR_WTT_BUF g_wu_ttbuf
#include "wino_common.h"

namespace {

template <int NRES, bool ADD>
__global__ __launch_bounds__(WINO_NT, 2) void conv3x3_wino_up2_kernel(const WinoParams p)
{
    constexpr bool HAS1 = NRES >= 1, HAS2 = NRES >= 2;      // residual operands of the epilogue (compile time; the network's x2 convs have none)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *Ps = smem;                        // [2][WU_PSZ]
    float *Vs = smem + 2 * WU_PSZ;           // [2][WU_VSZ]

    WinoFrame f(p);                          // block decode: the two output sub-blocks (uniform)
    const int t = f.t, lane = f.lane, wave = f.wave, c31 = f.c31, hh = f.hh, nb = f.nb, n0 = f.n0;
    const auto &sn = f.sn, &sy0 = f.sy0, &sx0 = f.sx0;
    const auto &sval = f.sval;

    // ---- staging unit of this thread (threads 0..399): (sub-block z, pixel of its 10x10 low-resolution patch, channel quad)
    const __amdgpu_buffer_rsrc_t rsrc_in = __builtin_amdgcn_make_buffer_rsrc((void *)(p.in + (size_t)sn[0] * p.H * p.W * p.Cin), 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_u = __builtin_amdgcn_make_buffer_rsrc((void *)p.u, 0, 0x7fffffff, 0x00020000);
    unsigned goff = 0xffffffffu;             // beyond num_records: the load returns zeros (padding, invalid sub-block, idle threads)
    int sdst = 0;
    {
        const int z = t >= 2 * WU_PPIX ? 1 : 0, r = t - 2 * WU_PPIX * z;
        const int pix = r >> 1, quad = r & 1;
        const int py = pix / WU_PW, px = pix - py * WU_PW;
        const int y = ((z ? sy0[1] : sy0[0]) >> 1) - 1 + py, x = ((z ? sx0[1] : sx0[0]) >> 1) - 1 + px;
        const bool ok = t < WU_UNITS && (z ? sval[1] : sval[0]) && y >= 0 && y < p.H && x >= 0 && x < p.W;
        if (ok) goff = (unsigned)((((size_t)(z ? sn[1] - sn[0] : 0) * p.H + y) * p.W + x) * p.Cin + 4 * quad) * 4u;
        sdst = (z * WU_PPIX + pix) * WU_PS + 4 * quad;
    }
    // ADD: the conv reads in + in2 (the decoder's `x + enc_feats[i]`, femasr_arch.py:361-362): a second request with the same offsets, one
    // packed add pair per unit while staging (zero padding stays zero: both requests return 0 there)
    const __amdgpu_buffer_rsrc_t rsrc_in2 = __builtin_amdgcn_make_buffer_rsrc((void *)((ADD ? p.in2 : p.in) + (size_t)sn[0] * p.H * p.W * p.Cin), 0, 0x7fffffff, 0x00020000);
    struct Unit { f32x4_t a, b; };
    Unit rp, rq;      // two register sets: the patch requested in step s is staged in step s+1 (kernels_wino.hip)
    auto load_patch_to = [&](Unit &rr, int s) {       // unconditional (steps past the end re-read the last one): the wait counters stay static
        const int sc = s < p.nsteps ? s : p.nsteps - 1;
        rr.a = __builtin_bit_cast(f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(rsrc_in, goff, sc * 32, 0));
        if (ADD) rr.b = __builtin_bit_cast(f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(rsrc_in2, goff, sc * 32, 0));
    };
    auto load_patch = [&](int s) { load_patch_to(rp, s); };
    auto store_patch_from = [&](const Unit &rr, int buf) {
        if (t < WU_UNITS) *reinterpret_cast<f32x4_t *>(Ps + buf * WU_PSZ + sdst) = ADD ? rr.a + rr.b : rr.a;
    };
    auto store_patch = [&](int buf) { store_patch_from(rp, buf); };

    // ---- input transform item: (tile tm, channel tch); waves 0-3 produce the rows v0, v1 of the column pass, waves 4-7 v3, v5
    // (w and w+4 share a SIMD: each SIMD carries both halves)
    const int thalf = wave >> 2;
    const int titem = (wave & 3) * 64 + lane;
    const int tm = titem >> 3, tch = titem & 7;
    // patch rows 2 ety + thalf .. + 2, columns 2 etx .. 2 etx + 3 of sub-block tm >> 4
    const int tsrc = (tm >> 4) * WU_PPIX * WU_PS + ((2 * ((tm & 15) >> 2) + thalf) * WU_PW + 2 * (tm & 3)) * WU_PS + tch;
    const int tdst = thalf * 8 * 256 + tm * 8 + (tch & 1) * 4 + (tch >> 1);
    float td[3][4];
    auto transform_read = [&](int pbuf) {
        const float *src = Ps + pbuf * WU_PSZ + tsrc;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) td[a][b] = src[(a * WU_PW + b) * WU_PS];
    };
    auto transform_write = [&](int vbuf) {
        float *dst = Vs + vbuf * WU_VSZ + tdst;
        float r[2][4];
        if (thalf == 0) {            // rows l0, l1, l2 -> v0, v1
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                r[0][b] = __builtin_fmaf(4.0f, td[0][b], __builtin_fmaf(-5.0f, td[1][b], td[2][b]));
                r[1][b] = __builtin_fmaf(-4.0f, td[1][b], td[2][b]);
            }
        } else {                     // rows l1, l2, l3 -> v3, v5
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                r[0][b] = td[1][b] - td[0][b];
                r[1][b] = __builtin_fmaf(4.0f, td[0][b], __builtin_fmaf(-5.0f, td[1][b], td[2][b]));
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float *o = dst + i * 4 * 256;
            o[0 * 256] = __builtin_fmaf(4.0f, r[i][0], __builtin_fmaf(-5.0f, r[i][1], r[i][2]));
            o[1 * 256] = __builtin_fmaf(-4.0f, r[i][1], r[i][2]);
            o[2 * 256] = r[i][2] - r[i][1];
            o[3 * 256] = __builtin_fmaf(4.0f, r[i][1], __builtin_fmaf(-5.0f, r[i][2], r[i][3]));
        }
    };

    // ---- M phase: pair q of wave w = (component w/2 + 4 q, column tile w & 1); q = 6 only exists for waves 0 and 1
    f32x16 acc[7];
#pragma unroll
    for (int q = 0; q < 7; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
    const unsigned lw = (unsigned)lane * 16u;
    const int aoff = c31 * 8 + hh * 4;
    const int wcomp0 = wave >> 1, wnt = wave & 1;
    const bool has6 = wave < 2;
    auto pcomp = [&](int q) -> int { const int c = wcomp0 + 4 * q; return c < 25 ? c : 24; };             // (clamped: the surplus load of waves 2-7 is never used)
    auto vcomp = [&](int q) -> int {           // component (i, j) of [0, 1, P, Q, 5]^2 -> distinct transformed value (P and Q share v3)
        const int c = pcomp(q), i = c / 5, j = c - 5 * i;
        return ((i > 2 ? i - 1 : i) << 2) + (j > 2 ? j - 1 : j);
    };
    auto ldU = [&](int s, int q) -> f32x4_t {  // unconditional, like load_patch (the addressing of kernels_wino.hip with 25 components)
        const int sc = s < p.nsteps ? s : p.nsteps - 1;
        return __builtin_bit_cast(f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(rsrc_u, lw, (((sc * 25 + pcomp(q)) * p.NT32 + 2 * nb + wnt) << 10), 0));
    };
    // U fragments: ring = pairs 0-2 of the NEXT step (loaded behind this step's pairs 0-2), early = pairs 3-5 (issued at the end of
    // the T phase, in flight across the barrier), late = pair 6 (issued at the start of the M phase)
    f32x4_t ring[3], early[3], late;
    auto issue_early = [&](int s) {
#pragma unroll
        for (int q = 3; q < 6; ++q) early[q - 3] = ldU(s, q);
    };
    auto mphase = [&](int s, auto par_c) {      // par_c = s & 1 at compile time
        constexpr int PAR = decltype(par_c)::value;
        const float *Vb = Vs + PAR * WU_VSZ + aoff;
        late = ldU(s, 6);
        // A fragments: the one of pair q+1 is REQUESTED before the MFMAs of pair q (two register sets, pinned with sched_barrier:
        // left alone the scheduler reuses one set and sinks the read below the MFMAs - an LDS round trip exposed per pair)
        f32x4_t af[2];
        af[0] = *reinterpret_cast<const f32x4_t *>(Vb + vcomp(0) * 256);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < 7; ++q) {
            if (q + 1 < 7) af[(q + 1) & 1] = *reinterpret_cast<const f32x4_t *>(Vb + vcomp(q + 1) * 256);
            __builtin_amdgcn_sched_barrier(0);
            const f32x4_t a = af[q & 1];
            const f32x4_t b = q < 3 ? ring[q] : (q < 6 ? early[q - 3] : late);
            if (q < 6 || has6) {
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[e], acc[q], 0, 0, 0);
            }
            if (q < 3) ring[q] = ldU(s + 1, q);
            if (q == 4) {      // behind the step's U requests (loads return in order)
                if (PAR) load_patch(s + 3);                       // (set rp) staged in the NEXT step's T phase, from the other set
                else load_patch_to(rq, s + 3);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    // ---- prologue: the patches of steps 0 and 1 requested together (two register sets), then the one step 0 stages
    load_patch(0);
    load_patch_to(rq, 1);
#pragma unroll
    for (int q = 0; q < 3; ++q) ring[q] = ldU(0, q);
    store_patch(0);
    load_patch(2);
    store_patch_from(rq, 1);
    __syncthreads();
    transform_read(0);
    transform_write(0);
    issue_early(0);
    __syncthreads();
    WTT(0)

    // ---- main loop.  Per step: M(s); transform of step s+1 (its patch was staged during step s-1); stage step s+2.
    // (Measured and dropped: 32-channel blocks with half the accumulators, <= 128 VGPRs and a 16-column epilogue exchange, so that
    // TWO blocks are resident per CU and one's prologue / epilogue runs under the other's MFMAs - bit-exact, and exactly as fast
    // as this form: 1.68 / 1.91 ms on both layer shapes.  The block's ends are instruction issue, not idle latency.
    // Also measured and dropped: the two waves of a SIMD taking the phases in opposite order - waves 0-3 M then T, waves 4-7 T then
    // M - so that one wave's LDS round trips run under its partner's MFMAs: 2.10 vs 1.68 ms on 256 -> 128 channels; the merged
    // control flow also costs a spilled accumulator tile per step.)
    auto step = [&](int s, auto par_c) {
        constexpr int PAR = decltype(par_c)::value;
        mphase(s, par_c);
        transform_read(PAR ^ 1);              // (unconditional: after the last step it transforms a stale patch into a dead buffer)
        __builtin_amdgcn_sched_barrier(0);
        transform_write(PAR ^ 1);
        __builtin_amdgcn_sched_barrier(0);
        // step s+2 -> the buffer the transform of step s read a barrier ago (from the set of this parity, requested a step ago)
        if (PAR) store_patch_from(rq, PAR); else store_patch_from(rp, PAR);
        issue_early(s + 1);
        __syncthreads();
        if (s < 40) WTT(16 + s)
    };
    for (int s = 0; s < p.nsteps; s += 2) {       // (nsteps = Cin / 8 is a multiple of 4)
        step(s, std::integral_constant<int, 0>{});
        step(s + 1, std::integral_constant<int, 1>{});
    }
    WTT(1)

    // ---------------------------------------------------------------------------------------------------------------
    // epilogue (wino_common.h) with 25 components and the 5 -> 4 transform.  The border masks, `fetch` and `round` are the text of
    // kernels_wino.hip (its comments apply) with at5, two Mx bases and Ho, Wo: as shared functions they cost SGPR spills and VGPRs
    float *Mx = smem;
    double *red = reinterpret_cast<double *>(smem + wino_mx(5));
    const bool gnp = p.gn_part != nullptr;
    const int cg = p.Cout >> 5;                      // channels per GroupNorm group (>= 2: Cout % 64 == 0)
    const int gpt = 32 / (cg < 32 ? cg : 32);        // groups per 32-channel tile (<= 16)
    const int pi = t >> 5;                           // tile pair: rows 2 pi, 2 pi + 1 of the accumulator tiles
    const int ez = wave >> 2, ety = wave & 3, etx = 2 * hh;      // sub-block (uniform), tile row (uniform), left tile of the pair
    unsigned vmask[2] = {0xffffu, 0xffffu}, ooff;
    bool full = true;
#pragma unroll
    for (int z = 0; z < 2; ++z) full = full && (z ? sval[1] : sval[0]) && (z ? sy0[1] : sy0[0]) + 16 <= p.Ho && (z ? sx0[1] : sx0[0]) + 16 <= p.Wo;      // (uniform)
    {
        const int oy = (ez ? sy0[1] : sy0[0]) + 4 * ety, ox = (ez ? sx0[1] : sx0[0]) + 4 * etx;
        if (!full) {         // per-pixel validity of the thread's two tiles (bit 4a + b): only a block that touches the image border needs it
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                unsigned m = 0;
#pragma unroll
                for (int k = 0; k < 16; ++k) m |= ((ez ? sval[1] : sval[0]) && oy + (k >> 2) < p.Ho && ox + 4 * e + (k & 3) < p.Wo ? 1u : 0u) << k;
                vmask[e] = m;
            }
        }
        ooff = (unsigned)((((ez ? sn[1] - sn[0] : 0) * p.Ho + oy) * p.Wo + ox) * p.Cout + n0 + c31) * 4u;      // (< 2^30: two images of < 2^27 elements)
    }
    f.template out_descriptors<NRES>(p);
    const __amdgpu_buffer_rsrc_t rs_out = f.rs_out, rs_r1 = f.rs_r1, rs_r2 = f.rs_r2;
    // uniform byte offset of pixel k = 4a + b of tile e, round r; the two strides are made opaque once per round (kernels_wino.hip)
    int cs_u = 0, rs_u = 0;
    auto soff = [&](int k, int e, int r) -> int { return (k >> 2) * rs_u + (4 * e + (k & 3)) * cs_u + 128 * r; };
    auto oob = [&](int e, int k) -> unsigned { return ~(unsigned)((int)(vmask[e] << (31 - k)) >> 31); };      // all-ones: pixel k of tile e is outside
    auto voff = [&](auto fullc, int e, int k) -> unsigned {
        if (decltype(fullc)::value) return ooff;
        return ooff | oob(e, k);
    };
    auto fetch = [&](auto fullc, const __amdgpu_buffer_rsrc_t rs, int r, tf2 (&dst)[16], int k0, int k1) {       // pixels k0 .. k1-1, no waits between
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (k < k0 || k >= k1) continue;
            dst[k][0] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff(fullc, 0, k), soff(k, 0, r), 0));
            dst[k][1] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff(fullc, 1, k), soff(k, 1, r), 0));
        }
    };
    auto round = [&](auto fullc, int r) {
        constexpr bool FULL = decltype(fullc)::value;
        tf2 r1[16], r2[16];
        if (!FULL) asm volatile("" : "+v"(vmask[0]), "+v"(vmask[1]));      // (opaque: the per-pixel masks are not to be hoisted out of the round loop)
        cs_u = __builtin_amdgcn_readfirstlane(p.Cout * 4);
        rs_u = __builtin_amdgcn_readfirstlane(p.Wo * p.Cout * 4);
        asm volatile("" : "+s"(cs_u), "+s"(rs_u));
        if (FULL) {          // (a border block fetches row by row below: kernels_wino.hip)
            if (HAS1) fetch(fullc, rs_r1, r, r1, 0, HAS2 ? 8 : 16);      // (two operands: upper tile rows now, lower ones behind the first pass - kernels_wino.hip)
            if (HAS2) fetch(fullc, rs_r2, r, r2, 0, 8);
        }
        const float bv = p.bias[n0 + 32 * r + c31];
        __syncthreads();
        WTT(3 + 4 * r)
        {
            // component stride: 16 tile pairs x 32 channels = 4 KiB; two bases keep every read inside the 64-KiB offset field
            int so1 = (16 * 512 + pi * 32 + c31) * 8;
            asm volatile("" : "+v"(so1));
            const tf2 *src0 = reinterpret_cast<const tf2 *>(Mx) + pi * 32 + c31;
            const tf2 *src1 = reinterpret_cast<const tf2 *>(reinterpret_cast<const char *>(Mx) + so1);
            auto mx = [&](int c) -> tf2 { return c < 16 ? src0[c * 512] : src1[(c - 16) * 512]; };
            tf2 tt[4][5];
#pragma unroll
            for (int j = 0; j < 5; ++j)
                at5(mx(0 * 5 + j), mx(1 * 5 + j), mx(2 * 5 + j), mx(3 * 5 + j), mx(4 * 5 + j), tt[0][j], tt[1][j], tt[2][j], tt[3][j]);
            if (FULL && HAS2) { fetch(fullc, rs_r1, r, r1, 8, 16); fetch(fullc, rs_r2, r, r2, 8, 16); }
            const tf2 bv2 = {bv, bv};
            tf2 s2 = {0.f, 0.f}, ss2 = {0.f, 0.f};
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                tf2 y[4];
                if (!FULL) {
                    __builtin_amdgcn_sched_barrier(0);
                    if (HAS1) fetch(fullc, rs_r1, r, r1, 4 * a, 4 * a + 4);
                    if (HAS2) fetch(fullc, rs_r2, r, r2, 4 * a, 4 * a + 4);
                    __builtin_amdgcn_sched_barrier(0);
                }
                at5(tt[a][0], tt[a][1], tt[a][2], tt[a][3], tt[a][4], y[0], y[1], y[2], y[3]);
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int k = 4 * a + b;
                    tf2 v = y[b] + bv2;
                    if (HAS1) v = v + r1[k];
                    if (HAS2) v = v + r2[k];
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[0]), rs_out, voff(fullc, 0, k), soff(k, 0, r), 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[1]), rs_out, voff(fullc, 1, k), soff(k, 1, r), 0);
                    if (gnp) {
                        if (!FULL) {
                            v[0] = __uint_as_float(__float_as_uint(v[0]) & ~oob(0, k));
                            v[1] = __uint_as_float(__float_as_uint(v[1]) & ~oob(1, k));
                        }
                        s2 = s2 + v;
                        ss2 = __builtin_elementwise_fma(v, v, ss2);
                    }
                }
            }
            if (gnp) {      // fp64 from here: the two tiles of the pair, the channels of the group (xor butterfly), the two pairs of the tile row
                double gs = (double)s2[0] + (double)s2[1], gss = (double)ss2[0] + (double)ss2[1];
                for (int d = 1; d < cg && d < 32; d <<= 1) {
                    gs = gs + __shfl_xor(gs, d, 64);
                    gss = gss + __shfl_xor(gss, d, 64);
                }
                const double a2 = gs + __shfl_xor(gs, 32, 64), b2 = gss + __shfl_xor(gss, 32, 64);
                if (lane < 32 && (c31 & (cg - 1)) == 0) {
                    double *dst = red + ((size_t)wave * 16 + c31 / cg) * 2;
                    dst[0] = a2;
                    dst[1] = b2;
                }
            }
        }
        WTT(4 + 4 * r)
    };
    // (one per-lane base, pinned as an integer offset: a wave's pairs are the components wave / 2 + 4 q; everything else is an
    // immediate offset)
    int wo0 = wcomp0 * 4096 + hh * 512 + c31 * 8;
    asm volatile("" : "+v"(wo0));
    char *wb0 = reinterpret_cast<char *>(Mx) + wo0;
    auto write_acc = [&]() {
#pragma unroll
        for (int q = 0; q < 7; ++q) {
            if (q < 6 || has6) f.store_acc_tile(wb0 + q * 4 * 4096, acc[q]);
        }
    };
#pragma unroll 1
    for (int r = 0; r < 2; ++r) {
        if (wnt == r) write_acc();
        WTT(2 + 4 * r)
        if (full) round(std::true_type{}, r); else round(std::false_type{}, r);
        __syncthreads();
        WTT(5 + 4 * r)
        f.gn_reduce(p, red, cg, gpt, r);
    }
    WTT_END
}

typedef void (*wu_kern_t)(const WinoParams);
wu_kern_t g_wu_kern[6] = {conv3x3_wino_up2_kernel<0, false>, conv3x3_wino_up2_kernel<1, false>, conv3x3_wino_up2_kernel<2, false>,      // [2 * ... ]: by residual
                          conv3x3_wino_up2_kernel<0, true>, conv3x3_wino_up2_kernel<1, true>, conv3x3_wino_up2_kernel<2, true>};          // operands, then + second input
unsigned long long g_attr_devs[6] = {0, 0, 0, 0, 0, 0};

}  // namespace

bool femasr_conv_wino_up2_shape_ok_lim(const femasr_conv_args *a, int log2_total, int log2_image)
{
    return wino_shape_ok(a, 5, 2, log2_total, log2_image) && a->up2 && a->prologue == FEMASR_PRO_NONE;
}
bool femasr_conv_wino_up2_shape_ok(const femasr_conv_args *a) { return femasr_conv_wino_up2_shape_ok_lim(a, FEMASR_WINO_LOG2_TOTAL, FEMASR_WINO_LOG2_IMAGE); }
const char *femasr_conv_wino_up2_variant_name() { return "conv3x3_wino_up2<2x16x16px x64,waves=8>"; }

int femasr_conv_wino_up2_launch(hipStream_t s, const femasr_conv_args *a, double *flops_out)
{
    FEMASR_REQUIRE(a && a->in && a->w_wino && a->bias && a->out && femasr_conv_wino_up2_shape_ok(a), "conv_wino_up2: bad arguments / shape");
    FEMASR_REQUIRE(a->Ho == 2 * a->H && a->Wo == 2 * a->W, "conv_wino_up2: Ho/Wo mismatch");
    WinoParams p{};
    FEMASR_CHECK(wino_params(a, "conv_wino_up2", p));
    const int nres = (a->res1 ? (a->res2 ? 2 : 1) : 0) + (a->in_add ? 3 : 0);      // (index into the instantiation table)
    const size_t lds = wino_lds_bytes(5, WU_MAIN, 0);
    FEMASR_CHECK(femasr_allow_dynamic_lds((const void *)g_wu_kern[nres], &g_attr_devs[nres], lds));
    hipLaunchKernelGGL(g_wu_kern[nres], dim3((unsigned)(p.MB * p.NB)), dim3(WINO_NT), lds, s, p);
    FEMASR_CHECK_HIP(hipGetLastError());
    // ALGORITHMIC flops (the definition's 9 taps per output pixel, like every other conv launcher); the kernel issues 25/144 of them
    if (flops_out) *flops_out = 2.0 * (double)a->B * a->Ho * a->Wo * 9.0 * (double)a->Cin * (double)a->Cout;
    return FEMASR_OK;
}

extern "C" {

#ifdef FEMASR_WINO_TT
int femasr_debug_wino_up2_ttbuf(unsigned long long *dev_buf)
{
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_wu_ttbuf), &dev_buf, sizeof(dev_buf));
}
#endif

size_t femasr_wino_up2_weight_floats(int O, int I) { return wino_weight_floats(5, O, I); }

int femasr_repack_oihw_wino_up2(void *stream, const float *in, int O, int I, float *out)
{
    return wino_repack<5, e5>(stream, in, O, I, out, "repack_wino_up2");
}

}  // extern "C"

"""-m gpu: every kernel on integer, impulse and flat-image inputs (tests/structured_inputs.py).

Kernel level: small integers make every summation order exact, so each conv form, the GEMMs, window attention and the codebook
search must return the result of a ten-line int64 numpy reference that shares no code with oracle/ or csrc/ - exactly; a single
1.0 must return the weights themselves; flat maps put GroupNorm / LayerNorm at zero variance (and the variance clamp), the
Winograd transforms at exact cancellation, the lookup at hundreds of identical rows.  Network level: the ten image contents
through every mode, the byte path where the output leaves [0, 1], batch independence, the tiled byte path.

tests/test_structured_inputs_host.py pins, on the CPU, what these tests rely on: the oracle equals the int64 references on every
integer family (the Winograd forms too: the {-576, 0, 576} x {0, 1} family is exact), the attention case is exact for shift 0 and 4,
no token of any content is a near tie under the chosen weight seed (nor under fp16 operands), and the recorded GroupNorm clamp cases have negative unclamped variance."""
import time

import numpy as np
import pytest
import torch

import structured_inputs as S
from femasr_amd import _lib, synth
from helpers import CONFIGS, oracle_net, synth_weights
from oracle import oracle as orc
from test_gpu_kernels import CONV_SMALL, GEMM_CFGS, conv_small, gemm_cfg            # noqa: F401  (the hooks' fixtures)
from test_gpu_network import TOL                                                    # 1e-3: the north-star bound, bf16x3's bound

pytestmark = pytest.mark.gpu
T0 = time.time()

# bounds the existing network tests state as literals (named here, not changed):
DEFAULT_MODE_TOL = 1e-4         # decoder_math 'fp32' against the oracle / fp32_strict: test_gpu_network.test_default_mode_vs_oracle_and_reference
LINEAR_SWITCH_TOL = 1e-4        # linear_math 'fp32' against 'bf16_split': test_gpu_r5.test_linear_math_switch_replans_and_differs
WINO_VS_DIRECT = 1e-4           # Winograd forms against the direct form, x max(1, |y|): test_gpu_kernels.test_conv_winograd_bit_exact
FAST_ACT_TOL = 1e-5             # fast-activation Winograd against the exact kernel, x max(1, |y|): test_conv_winograd_fast_act_close
BF16X3_KERNEL_TOL = 1e-4        # bf16x3 conv against the oracle, x |y|max: test_conv_bf16x3_within_tolerance


def f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bf16_rne(a):
    """fp32 -> the nearest bfloat16 (ties to even), as fp32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def assert_exact(got, want, what, coords='(n, y, x, c)'):
    bad = S.first_mismatch(got, want)
    assert not bad, f'{what} {coords}: {bad}'


def assert_bits(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = np.argwhere(bits(got) != bits(want))
    if len(diff):
        at = tuple(int(i) for i in diff[0])
        only_zero_signs = bool(np.all((got == 0) & (want == 0) | (bits(got) == bits(want))))
        raise AssertionError(f'{what}: {len(diff)} of {got.size} differ in their bits, first at {at}: got {got[at]!r} want {want[at]!r}, '
                             f'max-abs {np.abs(got.astype(np.float64) - want).max():.3e}, only signs of zeros: {only_zero_signs}')


def run_form(form, x, w, bias, k, s, p, up2, **kw):
    import gpu_utils as G
    flags = {'direct': {}, 'wino': dict(wino=True), 'split': dict(bf16s=True), 'bf16x3': dict(bf16x3=True), 'f16': dict(f16=True)}[form]
    return G.conv2d(f32(x), f32(w), f32(bias), k, s, p, up2, **flags, **kw)


# ------------------------------------------------------------------ integer exactness
@CONV_SMALL
@pytest.mark.parametrize('case', S.INT_CONV_CASES, ids=[c[0] for c in S.INT_CONV_CASES])
def test_integer_conv_equals_int64(cuda_device, case, conv_small):
    """Sparse inputs in {-2..2}, weights in {-3..3} (Winograd forms: {0, 1} and {-576, 0, 576}), integer bias and residuals, no
    prologue, no activation: every form returns the int64 convolution exactly, without residuals and with both."""
    name, shape, cout, k, s, p, up2, form = case
    x, w, b, r1, r2 = S.int_conv_operands(case)
    for nres in (0, 2):
        res = (r1, r2) if nres else (None, None)
        want = S.conv2d_ref(x, w, b, s, p, up2, *res)
        got = run_form(form, x, w, b, k, s, p, up2, res1=f32(res[0]), res2=f32(res[1]))
        assert_exact(got, want, f'{name} [{form}] nres {nres}')


@GEMM_CFGS
@pytest.mark.parametrize('n,k', S.INT_LINEAR_CASES)
def test_integer_linear_equals_int64(cuda_device, n, k, gemm_cfg):
    x, w, b, r1, r2 = S.int_linear_operands(n, k)
    rows = S.INT_LINEAR_ROWS
    want = S.linear_ref(x, w, b, r1, r2)
    got = run_form('direct', x.reshape(1, rows, 1, k), w.reshape(1, 1, k, n), b, 1, 1, 0, False,
                   res1=f32(r1).reshape(1, rows, 1, n), res2=f32(r2).reshape(1, rows, 1, n))
    assert_exact(got.reshape(rows, n), want, f'fp32 GEMM N {n} K {k}', '(row, column)')


@pytest.mark.parametrize('n,k', S.INT_LINEAR_CASES)
def test_integer_linear_split_gemm_equals_int64(cuda_device, n, k):
    x, w, b, r1, r2 = S.int_linear_operands(n, k)
    rows = S.INT_LINEAR_ROWS
    want = S.linear_ref(x, w, b, r1, r2)
    got = run_form('split', x.reshape(1, rows, 1, k), w.reshape(1, 1, k, n), b, 1, 1, 0, False,
                   res1=f32(r1).reshape(1, rows, 1, n), res2=f32(r2).reshape(1, rows, 1, n))
    assert_exact(got.reshape(rows, n), want, f'split GEMM N {n} K {k}', '(row, column)')


# ------------------------------------------------------------------ impulse response
IMPULSE_CASES = S.INT_CONV_CASES + [('f16_3x3', (2, 17, 23, 64), 128, 3, 1, 1, False, 'f16'), ('f16_up2', (1, 7, 9, 128), 64, 3, 1, 1, True, 'f16'),
                                    ('f16_k1', (1, 9, 11, 64), 96, 1, 1, 0, False, 'f16')]


@pytest.mark.parametrize('where', ['centre', 'corner'])
@pytest.mark.parametrize('case', IMPULSE_CASES, ids=[c[0] for c in IMPULSE_CASES])
def test_impulse_response_is_the_weights(cuda_device, case, where):
    """One 1.0 in one input channel, bias 0, noise weights.  Every output sum has one non-zero term, so the float64 reference IS the
    weight element (the fp16 forms: the weight rounded to fp16), and everything else is +0: compared bit for bit for the fp32 direct /
    halo / im2col forms, for the split-bf16 GEMM forms (w = w1 + w2 + w3 exactly) and for the bf16x3 halo form (which keeps two bf16
    terms per operand: the response is hi(w) + lo(w), 16 significant bits).  A nearest-x2 conv sees the 1.0 four times: its
    response is a sum of up to four taps, held bit for bit to the oracle's phase form and to the float64 sum within the three
    roundings of the pre-summed weights.  Winograd forms: bit for bit against the oracle, within the suite's Winograd-to-direct
    tolerance of the weights."""
    name, shape, cout, k, s, p, up2, form = case
    b, h, w_, cin = shape
    x = np.zeros(shape, np.float32)
    c0 = min(cin - 1, cin // 2 + 1)
    y0, x0 = (h // 2, w_ // 2) if where == 'centre' else (0, 0)
    x[:, y0, x0, c0] = 1.0
    wt = synth.uniform(41, name + 'iw', (k, k, cin, cout), -0.1, 0.1)
    bias = np.zeros(cout, np.float32)
    got = run_form(form, x, wt, bias, k, s, p, up2)
    if form == 'f16':
        weff = wt.astype(np.float16).astype(np.float64)
    elif form == 'bf16x3':          # hi = bf16(w), lo = bf16(w - hi); 1.0 has no lo part, so the two products hi_x hi_w + hi_x lo_w are all there is
        hi = bf16_rne(wt)
        weff = hi.astype(np.float64) + bf16_rne(wt - hi)
    else:
        weff = wt.astype(np.float64)
    want = S.conv2d_ref(x.astype(np.float64), weff, None, s, p, up2)
    assert np.count_nonzero(want) >= cout // 2
    if form == 'wino':
        assert_bits(got, orc.conv2d(x, wt, bias, k, s, p, up2, wino=True), f'{name} against the oracle')
        err = np.abs(got - want).max()
        assert err <= WINO_VS_DIRECT * max(1.0, np.abs(want).max()), err
    elif up2:
        if form == 'direct':
            assert_bits(got, orc.conv2d(x, wt, bias, k, s, p, up2), f'{name} against the oracle')
        bound = 3 * 2.0 ** -24 * S.conv2d_ref(x.astype(np.float64), np.abs(weff), None, s, p, up2)
        over = np.argwhere(np.abs(got - want) > bound)
        assert len(over) == 0, f'{name}: {len(over)} outputs off the sum of their taps, first at {tuple(over[0])}'
        assert np.array_equal(bits(got[want == 0]), bits(np.zeros(int((want == 0).sum()))))
    else:
        assert_bits(got, want.astype(np.float32), f'{name} [{form}] impulse at {where}')


# ------------------------------------------------------------------ window attention
@pytest.mark.parametrize('b,h,w,heads,shift', S.ATT_CASES)
def test_attention_with_zero_logits_is_the_window_mean(cuda_device, b, h, w, heads, shift):
    """q = k = 0, zero bias table, V small distinct integers: the output is EXACTLY the mean of V over the query's window (shift 0) or
    over the keys of its mask region (shift 4; 16, 32 or 64 keys, so 1/n is exact and the masked keys' weights vanish) - exact on the
    oracle too (host test), so equality is demanded, not one ulp."""
    import gpu_utils as G
    qkv, v = S.attention_operands(b, h, w, heads)
    sums, cnt = S.window_mean_ref(v, b, h, w, shift)
    got = G.window_attention(qkv, b, h, w, S.ATT_HEAD_DIM * heads, heads, shift, np.zeros((225, heads), np.float32))
    assert_exact(got, sums.astype(np.float64) / cnt[..., None], f'attention B{b} {h}x{w} heads {heads} shift {shift}', '(image, token, channel)')


# ------------------------------------------------------------------ codebook lookup
@pytest.mark.parametrize('mode', ['gemm', 'twopass'])
@pytest.mark.parametrize('n_e,d,m', S.VQ_CASES)
def test_vq_first_min_on_integer_ties(cuda_device, n_e, d, m, mode):
    """Integer codebook with duplicated codes and integer rows (40 identical rows, an all-zero row, a row equal to a duplicated code):
    the family is full of exact ties; the indices are the independent first-min argmin and z_q is the chosen code bit for bit."""
    import gpu_utils as G
    z, cb = S.vq_operands(n_e, d, m)
    want = S.vq_argmin_ref(z, cb)
    if mode == 'gemm' and n_e % 128:        # the single-pass search takes whole 128-code blocks: 64 codes are refused, loudly (two-pass takes them)
        with pytest.raises(_lib.FemasrError, match='n_e % 128'):
            G.vq(f32(z), f32(cb), mode=mode)
        return
    idx, zq, _, _ = G.vq(f32(z), f32(cb), mode=mode)
    assert_exact(idx, want, f'vq {mode} n_e {n_e} M {m}', '(row,)')
    assert_bits(zq, f32(cb)[want], f'vq {mode} z_q')


# ------------------------------------------------------------------ GroupNorm / LayerNorm on flat maps
def _gn_maps():
    out = []
    for shape in ((2, 13, 21, 64), (1, 1, 1, 32)):
        c = shape[3]
        cg = c // 32
        shared = np.repeat(synth.uniform(51, 'gnshared', (32,), -2.0, 2.0), cg)           # a group's channels share the constant: zero variance
        own = synth.uniform(51, 'gnown', (c,), -2.0, 2.0)                                 # every channel its own: variance between channels only
        out += [(f'zero{shape}', S.feature('zero', shape)), (f'shared{shape}', S.feature('const', shape, shared)),
                (f'own{shape}', S.feature('const', shape, own)), (f'one_pixel{shape}', S.feature('impulse', shape, shared, (0, 0), 3.0)),
                (f'step{shape}', S.feature('step', shape, own))]
    for shape, k in (S.GN_CLAMP_TILED, S.GN_CLAMP_ROWS):
        out.append((f'clamp{shape}', S.feature('const', shape, np.float32(k) / np.float32(255))))
    return out


GN_MAPS = _gn_maps()


@pytest.mark.parametrize('name,x', GN_MAPS, ids=[m[0] for m in GN_MAPS])
def test_groupnorm_on_flat_maps(cuda_device, name, x):
    """Zero or tiny variance inside a group - rstd = 1/sqrt(eps), the `var < 0` clamp of both finalize kernels on the recorded clamp
    cases - bit for bit against the oracle; then the GN + SiLU apply pass on the same coefficients."""
    import gpu_utils as G
    c = x.shape[3]
    gamma, beta = synth.uniform(52, 'gng', (c,), 0.5, 1.5), synth.uniform(52, 'gnb', (c,), -0.5, 0.5)
    a_ref, b_ref = orc.gn_coeffs(x, gamma, beta)
    assert np.isfinite(a_ref).all() and np.isfinite(b_ref).all()
    a, b = G.gn_coeffs(x, gamma, beta)
    assert_bits(a, a_ref, f'{name}: gn a')
    assert_bits(b, b_ref, f'{name}: gn b')
    if name.startswith(('zero', 'shared', 'clamp')):           # zero variance: rstd is 1/sqrt(eps) whatever the constant
        assert_bits(a, np.broadcast_to((np.float32(1.0) / np.sqrt(np.float32(1e-6))) * gamma, a.shape), f'{name}: a = gamma / sqrt(eps)')
    assert_bits(G.gn_silu_apply(x, a_ref, b_ref), orc.scale_shift_silu(x, a_ref, b_ref), f'{name}: gn_silu_apply')


@pytest.mark.parametrize('rows', [1, 5, 65])
def test_layernorm_on_constant_rows(cuda_device, rows):
    """A constant row has zero variance and zero centred values: the result is exactly beta.  The last row carries one differing
    element; it is compared with the oracle bit for bit."""
    import gpu_utils as G
    c = 256
    x = np.repeat(synth.uniform(53, 'lnc', (rows, 1), -3.0, 3.0), c, axis=1)
    x[rows - 1, 77] += np.float32(0.5)
    gamma, beta = synth.uniform(53, 'lng', (c,), 0.5, 1.5), synth.uniform(53, 'lnb', (c,), -0.5, 0.5)
    y = G.layernorm(x, gamma, beta)
    assert_bits(y, orc.layernorm(x, gamma, beta), f'layernorm, {rows} rows')
    if rows > 1:
        assert_bits(y[:-1], np.broadcast_to(beta, (rows - 1, c)), 'constant rows give beta')
    mean, var = S.row_moments(x)
    assert np.all(var[:-1] == 0.0) and var[-1] > 0.0
    stats = G.ln_stats(x)
    assert np.isfinite(stats).all()


# ------------------------------------------------------------------ conv forms with the GN + SiLU prologue on flat / step / impulse maps
def _pro_maps(shape):
    c = shape[3]
    own = synth.uniform(61, 'promap', (c,), -2.0, 2.0)
    return [('zero', S.feature('zero', shape)), ('flat', S.feature('const', shape, own)), ('step', S.feature('step', shape, own)),
            ('impulse', S.feature('impulse', shape, None, None, 2.0)), ('flat_plus_impulse', S.feature('impulse', shape, own, (0, 0), 2.5))]


@pytest.mark.parametrize('kind', ['zero', 'flat', 'step', 'impulse', 'flat_plus_impulse'])
def test_conv_forms_with_gn_silu_prologue_on_flat_maps(cuda_device, kind):
    """The ResBlock conv (GroupNorm apply + SiLU on load, bias + residual on store) on maps whose groups have zero variance, a hard edge
    or one hot pixel.  The strict forms - fp32 halo, Winograd F(4x4), and the x2 Winograd form (which has no prologue: it reads the
    oracle's activated map) - bit for bit against the oracle, signs of zeros included; the fast-activation Winograd, bf16x3 and fp16
    forms within the bounds their own tests state."""
    import gpu_utils as G
    import fp64_ref as R
    shape, cout = (2, 13, 21, 64), 128
    x = dict(_pro_maps(shape))[kind]
    gamma, beta = synth.uniform(62, 'prog', (64,), 0.5, 1.5), synth.uniform(62, 'prob', (64,), -0.5, 0.5)
    a, b = orc.gn_coeffs(x, gamma, beta)
    act = orc.scale_shift_silu(x, a, b)
    wt = synth.uniform(62, 'prow', (3, 3, 64, cout), -0.1, 0.1)
    bias = synth.uniform(62, 'probias', (cout,), -0.5, 0.5)
    r1 = synth.uniform(62, 'pror', shape[:3] + (cout,), -1, 1)
    pro = dict(prologue=_lib.PRO_GN_SILU, pro=(a, b, None), res1=r1)
    ref = orc.conv2d(act, wt, bias, 3, 1, 1, res1=r1)
    assert_bits(G.conv2d(x, wt, bias, 3, 1, 1, **pro), ref, f'{kind}: fp32 halo')
    ref_w = orc.conv2d(act, wt, bias, 3, 1, 1, res1=r1, wino=True)
    y_w = G.conv2d(x, wt, bias, 3, 1, 1, wino=True, **pro)
    assert_bits(y_w, ref_w, f'{kind}: Winograd strict')
    assert np.abs(ref_w - ref).max() <= WINO_VS_DIRECT * max(1.0, np.abs(ref).max())
    y_f = G.conv2d(x, wt, bias, 3, 1, 1, wino=True, fast_act=True, **pro)
    assert np.abs(y_f - y_w).max() <= FAST_ACT_TOL * max(1.0, float(np.abs(y_w).max())), np.abs(y_f - y_w).max()
    r_up = synth.uniform(62, 'proru', (shape[0], 2 * shape[1], 2 * shape[2], cout), -1, 1)
    assert_bits(G.conv2d(act, wt, bias, 3, 1, 1, True, res1=r_up, wino=True), orc.conv2d(act, wt, bias, 3, 1, 1, True, res1=r_up, wino=True),
                f'{kind}: Winograd x2')
    y_b = G.conv2d(x, wt, bias, 3, 1, 1, bf16x3=True, **pro)
    assert np.abs(y_b - ref).max() <= BF16X3_KERNEL_TOL * float(np.abs(ref).max())
    R.check_whole_conv3x3(x, wt, bias, y_b, 'bf16x3', pro=(a, b), res=[r1], what=f'{kind} bf16x3')
    y_h = G.conv2d(x, wt, bias, 3, 1, 1, f16=True, **pro)
    import fp16_ref as F
    pos = F.all_positions(*y_h.shape[:3])
    wo = torch.from_numpy(np.ascontiguousarray(wt.transpose(3, 2, 0, 1)))
    fref, mag, near, rest = F.conv_ref(torch.from_numpy(x), wo.numpy(), bias, pos, pro=(a, b), res=[torch.from_numpy(r1)])
    R.check(torch.from_numpy(y_h).reshape(len(pos), cout), fref, F.conv_bound(mag, near, rest), f'{kind} fp16')


# ------------------------------------------------------------------ network level
_NETS, _REFS, _EMU = {}, {}, {}
MODES = {                       # name: (decoder_math, linear_math)
    'fp32_strict': ('fp32_strict', 'bf16_split'), 'fp32': ('fp32', 'bf16_split'), 'bf16x3': ('bf16x3', 'bf16_split'),
    'decoder_fp16': ('fp16', 'bf16_split'), 'linear_fp32': ('fp32_strict', 'fp32'), 'linear_fp16': ('fp32', 'fp16'),
}
INDEX_EXACT_MODES = [m for m in MODES if m not in ('fp32_strict', 'linear_fp16')]          # ('linear_fp16': test_network_linear_fp16)


def _weights(cfg):
    return synth_weights(cfg, S.NET_SEED, 'trained')


def _net(cfg, mode='fp32_strict'):
    import gpu_utils as G
    if cfg not in _NETS:
        _NETS[cfg] = G.build_net(cfg, _weights(cfg))
    net = _NETS[cfg]
    net.decoder_math, net.linear_math = MODES[mode]
    net.num_streams = 1
    return net


def _ref(cfg, content):
    """(uint8 image, fp32 input, oracle output, oracle indices) of one (config, content): one oracle forward per session."""
    if (cfg, content) not in _REFS:
        u8 = S.image(content, *S.NET_LR[cfg])
        x = S.to_float(u8)
        y, idx = oracle_net(cfg, _weights(cfg)).test(x, return_indices=True)
        _REFS[cfg, content] = (u8, x, y, idx)
    return _REFS[cfg, content]


def _emulation(cfg, content, operand, decoder_operand, forced=None):
    """(image, first lookup's input rows z0, its distance matrix d0) of the CPU emulation (tests/fp16_front_ref.py): operands rounded once
    to fp16, float64 sums; the lookup returns `forced` (default: the oracle's indices)."""
    import fp16_front_ref as FR
    _, x, _, io = _ref(cfg, content)
    forced = io if forced is None else forced
    key = (cfg, content, operand, decoder_operand, forced.tobytes())
    if key not in _EMU:
        net = FR.emulation_net(_weights(cfg), CONFIGS[cfg], operand, forced_indices=forced, decoder_operand=decoder_operand)
        _EMU[key] = (FR.run_net(net, cfg, x)[0], net.z0, net.d0.numpy())
    return _EMU[key]


NET_IDS = [f'{c}-{n}' for c, n in S.NET_CASES]


@pytest.mark.parametrize('cfg,content', S.NET_CASES, ids=NET_IDS)
def test_network_strict_and_byte_path(cuda_device, cfg, content):
    """fp32_strict: the image bit-identical to the oracle's and the indices identical; test_u8 on the uint8 image == tensor2img of the
    oracle's float output byte for byte, RGB and BGR - the outputs leave [0, 1] on these contents (host test), so the clamp and the
    round-half-to-even work."""
    u8, x, yo, io = _ref(cfg, content)
    net = _net(cfg)
    y, idx = net.test_with_indices(torch.from_numpy(x).cuda())
    assert np.array_equal(idx.cpu().numpy(), io), f'{int((idx.cpu().numpy() != io).sum())} indices differ from the oracle'
    assert_bits(y.cpu().numpy(), yo, f'{cfg} {content} fp32_strict')
    assert yo.min() < 0.0 or yo.max() > 1.0
    t8 = torch.from_numpy(u8).cuda()
    assert np.array_equal(net.test_u8(t8).cpu().numpy(), orc.image_f32_to_u8(yo))
    assert np.array_equal(net.test_u8(t8.flip(-1).contiguous(), bgr=True).cpu().numpy(), orc.image_f32_to_u8(yo, bgr=True))


@pytest.mark.parametrize('mode', INDEX_EXACT_MODES)
@pytest.mark.parametrize('cfg,content', S.NET_CASES, ids=NET_IDS)
def test_network_modes_keep_the_indices(cuda_device, cfg, content, mode):
    """The modes whose arithmetic in front of the lookup differs from the oracle's by ulps at most: indices identical to the oracle's (no
    token of these contents is a near tie: host test) and the image within the bound the mode's own network test states - 'fp32' 1e-4
    of the oracle, 'bf16x3' the north-star 1e-3, linear_math 'fp32' 1e-4 of the split arithmetic, decoder_math 'fp16' 2 E with E the
    CPU emulation's deviation on the same content."""
    u8, x, yo, io = _ref(cfg, content)
    assert content not in S.NET_DROPPED
    xt = torch.from_numpy(x).cuda()
    y, idx = _net(cfg, mode).test_with_indices(xt)
    y, idx = y.cpu().numpy(), idx.cpu().numpy()
    d = float(np.abs(y - yo).max())
    print(f'{cfg} {content} {mode}: {int((idx != io).sum())} of {io.size} indices differ, max-abs against the oracle {d:.3e}')
    assert np.array_equal(idx, io), f'{int((idx != io).sum())} of {io.size} indices differ from the oracle'
    if mode == 'fp32':
        assert 0.0 < d < DEFAULT_MODE_TOL, d
    elif mode == 'bf16x3':
        assert 0.0 < d < TOL, d
    elif mode == 'linear_fp32':
        assert d < LINEAR_SWITCH_TOL, d
    elif mode == 'decoder_fp16':
        y32 = _net(cfg, 'fp32').test(xt).cpu().numpy()
        e = float(np.abs(_emulation(cfg, content, None, 'fp16')[0] - _emulation(cfg, content, None, None)[0]).max())
        d16 = float(np.abs(y - y32).max())
        print(f'   fp16 against fp32 {d16:.3e}, emulation E {e:.3e}')
        assert 0.0 < d16 <= 2.0 * e, (d16, e)
    _net(cfg)


@pytest.mark.parametrize('cfg,content', S.NET_CASES, ids=NET_IDS)
def test_network_linear_fp16(cuda_device, cfg, content):
    """linear_math='fp16' rounds the operands of every layer in front of the lookup to fp16, which moves z by ~1e-3 relative - not by
    ulps.  First the mode's own contract (tests/test_gpu_linear_fp16.py) on this content: every flipped token is a near tie of the
    reference distances under the mode's Delta, at most FLIP_CAP of the tokens flip, and the image lies within 2 E + D of the fp32
    emulation run with the GPU's own indices.  Then what this file demands of every mode: indices IDENTICAL to the oracle's - which
    the weight seed was chosen for: under S.NET_SEED the CPU emulation of the mode keeps every index of every content (host test)."""
    import fp16_front_ref as FR
    u8, x, yo, io = _ref(cfg, content)
    xt = torch.from_numpy(x).cuda()
    ys = _net(cfg, 'fp32').test(xt).cpu().numpy()
    y, idx = _net(cfg, 'linear_fp16').test_with_indices(xt)
    y, idx = y.cpu().numpy(), idx.cpu().numpy()
    _net(cfg)
    y32o, z_ref, d_ref = _emulation(cfg, content, None, None)
    _, z_emu, _ = _emulation(cfg, content, 'fp16', None)
    delta = FR.token_delta(z_emu, z_ref)
    flips, bad = FR.near_tie_failures(io, idx, d_ref, _weights(cfg)['quantize_group.0.embedding.weight'], delta)
    y32f = _emulation(cfg, content, None, None, forced=idx)[0]
    e = float(np.abs(_emulation(cfg, content, 'fp16', None, forced=idx)[0] - y32f).max())
    dd = float(np.abs(ys - y32o).max())
    d16 = float(np.abs(y - y32f).max())
    print(f'{cfg} {content} linear_fp16: {flips} of {io.size} tokens flipped, Delta {delta:.3g}; against the fp32 emulation {d16:.3e}, E {e:.3e}, D {dd:.3e}')
    assert flips <= FR.FLIP_CAP * io.size and not bad, (flips, bad)
    assert 0.0 < d16 <= 2.0 * e + dd, (d16, e, dd)
    assert np.array_equal(idx, io), f'{flips} of {io.size} indices differ from the oracle'


    _net(cfg)


@pytest.mark.parametrize('mode', list(MODES))
def test_network_batch_of_flat_and_busy_images(cuda_device, mode):
    """[black, letterbox, white] as one batch gives, per image, the bits of the single-image call - at one stream and at two."""
    xs = [_ref('x4', c)[1] for c in ('black', 'letterbox', 'white')]
    xb = torch.from_numpy(np.concatenate(xs)).cuda()
    net = _net('x4', mode)
    singles = [net.test_with_indices(xb[i:i + 1]) for i in range(3)]
    for streams in (1, 2):
        net.num_streams = streams
        y, idx = net.test_with_indices(xb)
        for i, (yi, ii) in enumerate(singles):
            assert torch.equal(y[i], yi[0]) and torch.equal(idx[i], ii[0]), (mode, streams, i)
    if mode == 'fp32_strict':
        for i, c in enumerate(('black', 'letterbox', 'white')):
            assert_bits(singles[i][0].cpu().numpy(), _ref('x4', c)[2], f'{c} in the batch')
    _net('x4')


@pytest.mark.parametrize('content', ['letterbox', 'step_h'])
def test_tiled_byte_path(cuda_device, content):
    """test_tile_u8 on 40 x 56 with tile 32 / pad 8.  Plain: == tensor2img of test_tile, byte for byte (the equality of
    test_gpu_r6.test_test_tile_u8_equals_the_fp32_tile_path on this content).  blend and color_fix are DEFINED on the byte tiles /
    the byte canvas (rounding comes before the blend), so they are held to their own definitions on this content: the blend to
    tests/blend_ref.py's canvas of the test_u8 tiles, the colour fix to wavelet_color_fix of the plain byte canvas."""
    from blend_ref import BlendRef, check_u8
    from femasr_amd import colorfix, imgproc, tiling
    net = _net('x4')
    h, w, ts, pad = 40, 56, 32, 8
    u8 = torch.from_numpy(S.image(content, h, w)).cuda()
    plain = net.test_tile_u8(u8, ts, pad)
    want = imgproc.output_to_u8(net.test_tile(imgproc.u8_to_input(u8), ts, pad))
    assert plain.shape == (4 * h, 4 * w, 3) and torch.equal(plain, want), int((plain != want).sum())
    assert int(plain.min()) == 0 and int(plain.max()) == 255           # the clamp worked on both sides
    got = net.test_tile_u8(u8, ts, pad, blend=True)
    tiles = tiling.enumerate_tiles(h, w, ts, pad)
    vals = [net.test_u8(u8[t.y0p:t.y1p, t.x0p:t.x1p, :].contiguous())[None].permute(0, 3, 1, 2).cpu().numpy() for t in tiles]
    bad, share = check_u8(got[None].permute(0, 3, 1, 2).cpu().numpy(), BlendRef(tiles, vals, 4, h, w))
    assert bad == 0 and share <= 0.01, (bad, share)
    fixed = net.test_tile_u8(u8, ts, pad, color_fix=True)
    assert torch.equal(fixed, colorfix.wavelet_color_fix(plain.clone(), u8, net.color_fix_levels))


def test_report_run_time(cuda_device):
    print(f'\ntests/test_gpu_structured_inputs.py: {time.time() - T0:.1f} s since import, {len(_REFS)} oracle forwards, {len(_EMU)} emulation forwards')

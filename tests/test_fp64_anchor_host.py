"""CPU checks of tests/fp64_ref.py, the fp64 references and bounds of tests/test_gpu_fp64_anchor.py:
  * each restatement agrees with torch's own fp64 operators at small shapes;
  * each bound accepts a correctly rounded result and REJECTS a deliberately wrong fp64 reference (a border tap dropped, the
    neighbouring channel's bias, a residual omitted, operands rounded once to bf16, the x2 phase swapped, a GroupNorm group off by
    one, the shift mask off by one window, the runner-up code) - host only, no kernel involved;
  * the calibration of C_FORM: the CPU oracle (bit-identical to each strict-mode kernel) at the network's channel counts on reduced
    grids, and every constant >= 4x the worst ratio measured."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fp64_ref as R


def _conv_case(seed, B=2, H=19, W=21, cin=64, cout=96, ksz=3, stride=1, pad=1, up2=False, pro=True, nres=2, in_add=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, H, W, cin), generator=g)
    w = torch.randn((cout, cin, ksz, ksz), generator=g) / math.sqrt(ksz * ksz * cin)
    b = (torch.rand(cout, generator=g) - 0.5) * 0.2
    a_ = (torch.rand(B, cin, generator=g) + 0.5).numpy().astype(np.float32)
    b_ = (torch.rand(B, cin, generator=g) - 0.5).numpy().astype(np.float32)
    hv, wv = (2 * H, 2 * W) if up2 else (H, W)
    ho, wo = (hv + 2 * pad - ksz) // stride + 1, (wv + 2 * pad - ksz) // stride + 1
    res = [torch.randn((B, ho, wo, cout), generator=g) for _ in range(nres)]
    add = torch.randn((B, H, W, cin), generator=g) if in_add else None
    return x, w, b, ((a_, b_) if pro else None), res, add, (ho, wo)


def _torch_fp64(x, w, b, ksz, stride, pad, up2, pro, res, add, act=0):
    t = x.double() + (add.double() if add is not None else 0)
    if pro is not None:
        z = torch.as_tensor(pro[0]).double()[:, None, None, :] * t + torch.as_tensor(pro[1]).double()[:, None, None, :]
        t = F.silu(z)
    t = t.permute(0, 3, 1, 2)
    if up2:
        t = F.interpolate(t, scale_factor=2, mode='nearest')
    y = F.conv2d(t, w.double(), b.double(), stride=stride, padding=pad).permute(0, 2, 3, 1)
    if act == 1:
        y = F.gelu(y)
    for r in res:
        y = y + r.double()
    return y


@pytest.mark.parametrize('kw', [dict(), dict(up2=True, pro=False, in_add=True, nres=1), dict(stride=2, pro=False, nres=0),
                                dict(ksz=4, cin=3, pad=1, pro=False, nres=0), dict(ksz=1, pad=0, pro=False, nres=1)],
                         ids=['pro_res2', 'up2_in_add', 'stride2', 'k4_cin3', 'k1'])
def test_conv_ref_matches_torch_fp64(kw):
    x, w, b, pro, res, add, (ho, wo) = _conv_case(0, **kw)
    ksz, stride, pad, up2 = kw.get('ksz', 3), kw.get('stride', 1), kw.get('pad', 1), kw.get('up2', False)
    pos = R.conv_positions(x.shape[0], ho, wo, 1)
    ref, mag, pt, rest = R.conv_ref(x, w.numpy(), b.numpy(), pos, ksz, stride, pad, up2, pro=pro, in_add=add, res=res)
    full = _torch_fp64(x, w, b, ksz, stride, pad, up2, pro, res, add)
    want = full[pos[:, 0], pos[:, 1], pos[:, 2]]
    assert torch.allclose(ref, want, rtol=1e-12, atol=1e-12)
    assert (mag > 0).all() and (rest > 0).all()


def _rounded(ref):
    return ref.to(torch.float32).to(torch.float64)


CONV_MUTATIONS = [('drop_border_tap', dict()), ('neighbour_bias', dict()), ('drop_residual', dict()),
                  ('bf16_operands', dict(cin=256, cout=256, pro=False, nres=0)), ('phase_swap', dict(up2=True, pro=False, nres=0))]


@pytest.mark.parametrize('form', ['direct', 'wino4', 'wino_up2', 'split3x3', 'bf16x3', 'gemm_fp32'])
@pytest.mark.parametrize('mutation,kw', CONV_MUTATIONS, ids=[m for m, _ in CONV_MUTATIONS])
def test_conv_bound_rejects_wrong_reference(form, mutation, kw):
    """The correctly rounded fp64 result passes; the same check against the mutated reference fails."""
    x, w, b, pro, res, add, (ho, wo) = _conv_case(3, **kw)
    if form == 'wino_up2' and not kw.get('up2'):
        kw = dict(kw, up2=True)
        x, w, b, pro, res, add, (ho, wo) = _conv_case(3, **kw)
        pro = None
    up2 = kw.get('up2', False)
    fast = form == 'bf16x3'          # (its prologue SiLU is the hardware one in every mode: PRO_ERR[True])
    pos = R.conv_positions(x.shape[0], ho, wo, 4)
    ref, mag, pt, rest = R.conv_ref(x, w.numpy(), b.numpy(), pos, 3, 1, 1, up2, pro=pro, res=res, fast_act=fast)
    bound = R.conv_bound(mag, pt, rest, form)
    got = _rounded(ref)
    R.check(got, ref, bound, 'correct')
    bad, bmag, bpt, brest = R.conv_ref(x, w.numpy(), b.numpy(), pos, 3, 1, 1, up2, pro=pro, res=res, fast_act=fast, mutate=mutation)
    assert R.rejects(lambda: R.check(got, bad, R.conv_bound(bmag, bpt, brest, form), mutation)), mutation


# ---------------------------------------------------------------- a CPU model of the specified bf16x3 arithmetic
def _bf16_split(v):
    """hi = bf16_rne(v), lo = bf16_rne(v - hi), the difference taken in fp32 (include/femasr_hip.h, w_bf16x3): float64 tensors holding
    bf16 values."""
    v = v.to(torch.float32)
    hi = v.to(torch.bfloat16).to(torch.float32)
    lo = (v - hi).to(torch.bfloat16).to(torch.float32)
    return hi.to(torch.float64), lo.to(torch.float64)


def bf16x3_model(x, w_oihw, bias, pos, res=(), drop=None):
    """The documented arithmetic of the bf16x3 3x3 conv at the positions `pos`, written from its specification and not from the kernel:
    activations and weights split into hi + lo (two bf16 values each); per 16-deep k-step three matrix products hi_x hi_w, hi_x lo_w,
    lo_x hi_w (bf16 x bf16 is exact in fp32; the 16-term sums are taken exactly here) accumulated one after the other into an fp32
    accumulator; K runs over 32-channel blocks, the 9 taps inside a block, two 16-deep steps inside a tap; then bias and residuals in
    fp32.  drop: 'lo_x*hi_w' or 'hi_x*lo_w' leaves that product out (the mutations the bound must reject).  Returns (S, Cout) fp32."""
    t, ok = R.gather_taps(x, pos, 3, 1, 1, False)                       # (S, 9, C)
    t = t * ok[:, :, None]
    S, _, C = t.shape
    w = torch.as_tensor(np.asarray(w_oihw, np.float32), dtype=torch.float64)          # (O, C, 3, 3)
    wk = w.permute(2, 3, 1, 0).reshape(9, C, w.shape[0])                              # [tap][c][o]
    xh, xl = _bf16_split(t)
    wh, wl = _bf16_split(wk)
    terms = [(xh, wh), (xh, wl), (xl, wh)]
    if drop == 'hi_x*lo_w':
        terms.pop(1)
    elif drop == 'lo_x*hi_w':
        terms.pop(2)
    else:
        assert drop is None
    acc = torch.zeros((S, w.shape[0]), dtype=torch.float32)
    for q in range(C // 32):
        for tap in range(9):
            for s in range(2):
                c0 = q * 32 + 16 * s
                for (a, b) in terms:
                    acc = (acc.to(torch.float64) + a[:, tap, c0:c0 + 16] @ b[tap, c0:c0 + 16]).to(torch.float32)
    y = acc + torch.as_tensor(np.asarray(bias, np.float32))[None]
    p = torch.as_tensor(pos)
    for r in res:
        y = y + r[p[:, 0], p[:, 1], p[:, 2]]
    return y


def _bf16x3_case(seed, cin, cout, silu):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((1, 12, 20, cin), generator=g)
    if silu:          # what a GroupNorm + SiLU prologue hands the matrix cores: one-sided, most values near zero
        x = torch.nn.functional.silu(x * 1.2 + 0.1)
    w = torch.randn((cout, cin, 3, 3), generator=g) / math.sqrt(9 * cin)
    b = (torch.rand(cout, generator=g) - 0.5) * 0.2
    r1 = torch.randn((1, 12, 20, cout), generator=g)
    return x, w, b, r1, R.conv_positions(1, 12, 20, seed)


BF16X3_CAL = [(64, 64), (128, 128), (256, 256), (512, 128)]          # Cin, Cout (the network's decoder-side channel counts)


def test_bf16x3_model_calibrates_its_constant():
    """C_FORM['bf16x3'] >= 4x the worst c the model of the specified arithmetic needs (N(0,1) and SiLU-shaped inputs, Cin 64 .. 512)
    and <= 208, the analytic worst case of the arithmetic (3 x 2^-18 relative for the two representation errors and the dropped
    lo*lo term, + 16 for the fp32 accumulation): a larger constant would say nothing about the split."""
    assert R.C_BF16X3_MAX == 3 * 2.0 ** -18 / R.U + 16.0 == 208.0
    worst = {}
    for i, (cin, cout) in enumerate(BF16X3_CAL):
        for silu in (False, True):
            x, w, b, r1, pos = _bf16x3_case(300 + i, cin, cout, silu)
            ref, mag, pt, rest = R.conv_ref(x, w.numpy(), b.numpy(), pos, 3, 1, 1, False, res=[r1])
            c = _needed_c(bf16x3_model(x, w.numpy(), b.numpy(), pos, res=[r1]), ref, mag, pt, rest)
            worst[(cin, 'silu' if silu else 'randn')] = c
    print('\nbf16x3 model (worst c): ' + ', '.join(f'Cin {k[0]} {k[1]} {v:.3g}' for k, v in worst.items())
          + f" (C_FORM {R.C_FORM['bf16x3']:g}, cap {R.C_BF16X3_MAX:g})")
    assert R.C_FORM['bf16x3'] >= 4.0 * max(worst.values()), worst
    assert R.C_FORM['bf16x3'] <= R.C_BF16X3_MAX


@pytest.mark.parametrize('cin,cout', [(64, 64), (512, 128)])
@pytest.mark.parametrize('drop', ['lo_x*hi_w', 'hi_x*lo_w'])
@pytest.mark.parametrize('silu', [False, True], ids=['randn', 'silu'])
def test_bf16x3_bound_rejects_a_missing_cross_term(cin, cout, drop, silu):
    """The model's output passes the bf16x3 bound against the true fp64 reference; with either cross term left out it is rejected,
    and most of its elements are over the bound one by one (not only the worst one)."""
    x, w, b, r1, pos = _bf16x3_case(400 + cin, cin, cout, silu)
    ref, mag, pt, rest = R.conv_ref(x, w.numpy(), b.numpy(), pos, 3, 1, 1, False, res=[r1])
    bound = R.conv_bound(mag, pt, rest, 'bf16x3')
    R.check(bf16x3_model(x, w.numpy(), b.numpy(), pos, res=[r1]), ref, bound, 'model')
    bad = bf16x3_model(x, w.numpy(), b.numpy(), pos, res=[r1], drop=drop)
    assert R.rejects(lambda: R.check(bad, ref, bound, drop)), drop
    over = float(((bad.to(torch.float64) - ref).abs() > bound).double().mean())
    assert over > 0.5, (drop, cin, over)


def test_gn_bound_rejects_group_off_by_one():
    g = torch.Generator().manual_seed(5)
    x = torch.randn((2, 9, 11, 256), generator=g) * (torch.rand(256, generator=g) + 0.5) + torch.randn(256, generator=g)
    gamma, beta = np.ones(256, np.float32), np.zeros(256, np.float32)
    a, b, ba, bb = R.gn_coeffs_ref(x, gamma, beta)
    R.check(_rounded(a), a, ba, 'gn a')
    R.check(_rounded(b), b, bb, 'gn b')
    a2, b2, ba2, bb2 = R.gn_coeffs_ref(x, gamma, beta, group_shift=1)
    assert R.rejects(lambda: R.check(_rounded(a), a2, ba2, 'gn a off by one'))


def test_layernorm_ref_matches_torch():
    g = torch.Generator().manual_seed(6)
    x = torch.randn((37, 256), generator=g, dtype=torch.float64) * 2 + 0.5
    gamma, beta = np.linspace(0.5, 1.5, 256).astype(np.float32), np.linspace(-0.2, 0.2, 256).astype(np.float32)
    ref, bnd = R.layernorm_ref(x, gamma, beta)
    want = F.layer_norm(x, (256,), torch.as_tensor(gamma).double(), torch.as_tensor(beta).double(), 1e-5)
    assert torch.allclose(ref, want, rtol=1e-12, atol=1e-12)
    R.check(_rounded(ref), ref, bnd, 'ln')


def _attention_torch(qkv, B, H, W, C, heads, shift, table, ws=8):
    """network_swinir.py SwinTransformerBlock attention path (roll, window partition, mask, reverse) in fp64 on whole images."""
    hd = C // heads
    x = qkv.reshape(B, H, W, 3 * C)
    if shift:
        x = torch.roll(x, (-shift, -shift), (1, 2))
    xw = x.reshape(B, H // ws, ws, W // ws, ws, 3 * C).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = xw[0] * hd ** -0.5, xw[1], xw[2]
    att = q @ k.transpose(-2, -1)
    bias = torch.as_tensor(table).double()[torch.as_tensor(R.rel_index(ws)).reshape(-1)].reshape(64, 64, heads).permute(2, 0, 1)
    att = att + bias[None]
    if shift:
        reg = torch.as_tensor(R.region_ids(H, W, ws, shift)).reshape(H // ws, ws, W // ws, ws).permute(0, 2, 1, 3).reshape(-1, 64)
        m = torch.where(reg[:, :, None] != reg[:, None, :], -100.0, 0.0).double()
        att = att.reshape(B, -1, heads, 64, 64) + m[None, :, None]
        att = att.reshape(-1, heads, 64, 64)
    o = (att.softmax(-1) @ v).transpose(1, 2).reshape(B, H // ws, W // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)
    if shift:
        o = torch.roll(o, (shift, shift), (1, 2))
    return o.reshape(B * H * W, C)


@pytest.mark.parametrize('shift', [0, 4])
def test_attention_ref_matches_swin_and_rejects_mask_shift(shift):
    B, H, W, C = 2, 24, 32, 256
    g = torch.Generator().manual_seed(8 + shift)
    qkv = torch.randn((B * H * W, 3 * C), generator=g, dtype=torch.float64)
    table = (np.random.default_rng(1).standard_normal((225, 8)) * 0.5).astype(np.float32)
    wins = R.attention_windows(B, H, W, 8, 2)
    rows, ref, bnd = R.attention_ref(qkv, B, H, W, C, 8, shift, table, wins)
    full = _attention_torch(qkv, B, H, W, C, 8, shift, table)
    assert torch.allclose(ref, full[torch.as_tensor(rows)], rtol=1e-10, atol=1e-12)
    R.check(_rounded(ref), ref, bnd, 'attn')
    if shift:
        _, bad, bb = R.attention_ref(qkv, B, H, W, C, 8, shift, table, wins, mask_shift=1)
        assert R.rejects(lambda: R.check(_rounded(ref), bad, bb, 'mask off by one window'))


def test_vq_check_rejects_runner_up():
    rng = np.random.default_rng(9)
    cb = rng.standard_normal((1024, 64)).astype(np.float32)
    z = torch.as_tensor(cb[rng.integers(0, 1024, 500)] + 0.5 * rng.standard_normal((500, 64)).astype(np.float32))
    zd = z.double()
    d = (zd * zd).sum(1, keepdim=True) + (torch.as_tensor(cb).double() ** 2).sum(1)[None] - 2 * zd @ torch.as_tensor(cb).double().T
    best = d.argmin(1)
    zq = torch.as_tensor(cb)[best]
    rows = R.vq_rows(z, cb, 0, n=100, nclose=20)
    R.vq_check(z, cb, best, zq, rows, 'correct')
    second = d.topk(2, largest=False).indices[:, 1]
    assert R.rejects(lambda: R.vq_check(z, cb, second, torch.as_tensor(cb)[second], rows, 'runner-up'))


# ---------------------------------------------------------------- calibration of C_FORM with the oracle (strict-mode arithmetic)
def _needed_c(got, ref, mag, pt, rest):
    """Per element: the c with |got - ref| = c u mag + 2u rest + pt (the non-c terms taken first); the worst over elements."""
    err = (torch.as_tensor(got, dtype=torch.float64) - ref).abs()
    return float(((err - 2 * R.U * rest - pt).clamp_min(0) / (R.U * mag)).max())


CAL = [  # form, (B, H, W, Cin), Cout, oracle call
    ('direct', (2, 24, 40, 64), 64), ('direct', (1, 20, 24, 256), 256),
    ('wino4', (2, 24, 40, 64), 64), ('wino4', (1, 20, 36, 128), 128), ('wino4', (1, 16, 24, 256), 256),
    ('wino_up2', (1, 10, 12, 256), 128), ('wino_up2', (1, 9, 10, 128), 64),
    ('split3x3', (1, 16, 24, 256), 256),
    ('split1x1', (1, 300, 1, 256), 768), ('split1x1', (1, 300, 1, 1024), 256),
    ('gemm_fp32', (2, 19, 23, 3), 256),
    # linear_math 'fp32': the LDS-DMA GEMM (orc.linear) at the K and Cout of the network's 1x1 layers, a few hundred rows each
    ('gemm_fp32', (1, 300, 1, 256), 768, dict(ksz=1)), ('gemm_fp32', (1, 333, 1, 256), 256, dict(ksz=1)),            # qkv, proj
    ('gemm_fp32', (1, 300, 1, 256), 1024, dict(ksz=1, act=1)), ('gemm_fp32', (1, 270, 1, 1024), 256, dict(ksz=1)),   # fc1 + GELU, fc2
    ('gemm_fp32', (1, 300, 1, 256), 512, dict(ksz=1)),                                                               # before_quant
    # decoder_math 'fp32_direct' / linear_math 'fp32': the x2 convs as phase filters, the stride-2 encoder convs (conv_igemm)
    ('direct', (1, 10, 12, 256), 128, dict(up2=True)), ('direct', (1, 9, 10, 128), 64, dict(up2=True)),
    ('direct', (1, 24, 40, 64), 128, dict(stride=2)), ('direct', (1, 20, 24, 128), 256, dict(stride=2)),
]


def test_calibration():
    from oracle import oracle as orc
    worst = {}
    rows = []
    for i, (form, (B, H, W, cin), cout, *opt) in enumerate(CAL):
        opt = opt[0] if opt else {}
        rng = np.random.default_rng(100 + i)
        ksz = opt.get('ksz', 1 if form == 'split1x1' else (4 if form == 'gemm_fp32' else 3))
        pad = 0 if ksz == 1 else 1
        up2 = form == 'wino_up2' or opt.get('up2', False)
        stride, act = opt.get('stride', 1), opt.get('act', 0)
        x = rng.standard_normal((B, H, W, cin)).astype(np.float32)
        w = (rng.standard_normal((cout, cin, ksz, ksz)) / math.sqrt(ksz * ksz * cin)).astype(np.float32)
        b = ((rng.random(cout) - 0.5) * 0.2).astype(np.float32)
        w_khwc = np.ascontiguousarray(w.transpose(2, 3, 1, 0))
        hv, wv = (2 * H, 2 * W) if up2 else (H, W)
        ho, wo = (hv + 2 * pad - ksz) // stride + 1, (wv + 2 * pad - ksz) // stride + 1
        r1 = rng.standard_normal((B, ho, wo, cout)).astype(np.float32)
        if form == 'split3x3':
            y = orc.conv3x3_bf16s(x, w_khwc, b, r1, None, 1)
        elif form == 'split1x1':
            y = orc.linear_bf16s(x.reshape(-1, cin), w.reshape(cout, cin), b, 0, r1.reshape(-1, cout)).reshape(B, ho, wo, cout)
        elif form == 'gemm_fp32' and ksz == 1:
            y = orc.linear(x.reshape(-1, cin), np.ascontiguousarray(w.reshape(cout, cin).T), b, act, r1.reshape(-1, cout)).reshape(B, ho, wo, cout)
        else:
            y = orc.conv2d(x, w_khwc, b, ksz, stride, pad, up2, act, r1, None, wino=form in ('wino4', 'wino_up2'))
        pos = R.conv_positions(B, ho, wo, i)
        ref, mag, pt, rest = R.conv_ref(torch.as_tensor(x), w, b, pos, ksz, stride, pad, up2, res=[torch.as_tensor(r1)], act=act)
        got = torch.as_tensor(y[pos[:, 0], pos[:, 1], pos[:, 2]])
        c = _needed_c(got, ref, mag, pt, rest)
        rows.append(f"  {form:10s} {cin:4d}->{cout:4d} k{ksz}s{stride}{' x2' if up2 else ''}{' gelu' if act else ''}: {c:.3g}")
        worst[form] = max(worst.get(form, 0.0), c)
    print('\ncalibration rows (the c each case needs):\n' + '\n'.join(rows))
    print('\ncalibration (worst c per form): ' + ', '.join(f'{k} {v:.3g} (C_FORM {R.C_FORM[k]:g})' for k, v in worst.items()))
    for k, v in worst.items():
        assert R.C_FORM[k] >= 4.0 * v, (k, v, R.C_FORM[k])


def test_conv_variant_hook_names_and_refusals():
    """femasr_debug_conv_variant_name (no GPU needed): the slot of a given form and variant, and refusals of what it cannot name."""
    import ctypes
    from femasr_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    a = _lib.ConvArgs()
    assert lib.femasr_debug_conv_variant_name(ctypes.byref(a), buf, len(buf)) != 0          # empty shape, stride 0
    a.B, a.H, a.W, a.Cin, a.Cout, a.ksz, a.stride, a.pad, a.Ho, a.Wo = 6, 144, 144, 256, 256, 3, 1, 1, 144, 144
    a.w, a.w_wino, a.prologue, a.fast_act, a.res1 = 1, 1, 1, 1, 1
    _lib.check(lib.femasr_debug_conv_variant_name(ctypes.byref(a), buf, len(buf)))
    assert buf.value.decode() == 'conv3x3_wino4<2x16x16px x64,FEMASR_PRO_GN_SILU,true,res=1,waves=8>'
    assert lib.femasr_debug_conv_variant_name(ctypes.byref(a), buf, len(buf.value)) != 0     # no room for the terminating zero
    a.w_wino, a.w_bf16s, a.prologue, a.res1 = None, 1, 0, None
    _lib.check(lib.femasr_debug_conv_variant_name(ctypes.byref(a), buf, len(buf)))
    assert buf.value.decode() == 'conv3x3_bf16s<128px x128,9Cin split GEMM,nres=0>'


# ---------------------------------------------------------------- the launch inventories (host: the variant hook needs no GPU)
# sha256 of repr(workload_layers(...)) per sub-batch and of the sorted conv case keys of inventory(), as computed before
# workload_layers took rectangular inputs (the pad entry's new w_in / Hp / Wp fields left out of the layer digest)
BENCH_PINS = {
    'x4_b16_128': ({5: '822b1c42561b97fbf2f60ef74556a9033ec34732bcbca7124d87c74c1663f70a',
                    6: 'b12619c5ecea4ce05821ad18fab3cfa3993c6a0670cc8131118d5fc0e59c5b1e'},
                   '124cb55adb9a16cd54719dfec9150361681af7f283688d28ca5ab075750f62b9', 68, 20),
    'x2_b32_256': ({10: '9df8b635732f56be10a0e256ffdb2eee7014d5f9a79d2c07481671d3fffac1cc',
                    11: 'd468e3db67389cf9f956c057bd85e7c6884e1be2cc99a1b069a8a3cc518788c0'},
                   'e6bbc84ca2e5e51d97a328c53f4010fc105ed9cfebf2a958805e9562ba9a7eca', 76, 20),
    'hq_b8_512': ({2: '3397daec009b7ddc6e6af8d798dc1a6417846cb6f8f469486ab5afeb8b839860',
                   3: '2bd175bda29ac8a5d5f23650f081b571952eec0c2e00d6e8d6f37dcd548f4bbf'},
                  'fb20f7ac81ac2d67fcd0a098833b99009ba3facf480d2d241c34ea6080f3b8d9', 74, 14),
}


def _digest(obj):
    import hashlib
    return hashlib.sha256(repr(obj).encode()).hexdigest()


@pytest.mark.parametrize('wl_name', list(R.WORKLOADS))
def test_bench_inventory_unchanged_by_rectangular_layers(wl_name):
    import anchor_cases as A
    layers, conv_keys, nconv, nsmall = BENCH_PINS[wl_name]
    assert R.sub_batches(R.WORKLOADS[wl_name]['batch'], R.BENCH_STREAMS) == sorted(layers)
    for sub_b, want in layers.items():
        L = [{k: v for k, v in l.items() if not (l['kind'] == 'pad' and k in ('w_in', 'Hp', 'Wp'))} for l in A._layers(wl_name, sub_b)]
        assert _digest(L) == want, (wl_name, sub_b)
    convs, small = A.inventory(wl_name)
    assert (_digest(sorted(convs)), len(convs), len(small)) == (conv_keys, nconv, nsmall)
    for l in A._layers(wl_name, sorted(layers)[0]):
        if l['kind'] == 'pad':
            assert (l['Hp'], l['Wp'], l['w_in']) == (l['H'], l['W'], l['h_in'])


def test_product_workloads_are_the_cli_defaults():
    """The table is derived from tiling.enumerate_tiles / shape_classes at (240, 16), max_tile_batch 16, streams 1, 2, 3."""
    from femasr_amd.archs.femasr_arch import FeMaSRNet
    import inspect
    sig = inspect.signature(FeMaSRNet.test_tile).parameters
    assert (sig['tile_size'].default, sig['tile_pad'].default) == (R.CLI_TILE, R.CLI_PAD)
    assert R.tiled_calls(1440, 1440) == {(256, 256): [4], (256, 272): [8], (272, 256): [8], (272, 272): [16]}
    big = R.tiled_calls(1356, 2040)
    assert big[(272, 272)] == [12, 16] and (172, 136) in big and (272, 136) in big
    W = R.PRODUCT_WORKLOADS
    assert W['tiled1440x1440_win272x272']['sub_batches'] == [5, 6, 8, 16]
    assert W['tiled1356x2040_win272x272']['sub_batches'] == [4, 5, 6, 8, 12, 16]
    assert not set(W) & set(R.WORKLOADS)
    for n in ('whole599x599_x4', 'whole339x510_x4', 'whole16x600_x4', 'whole599x599_x2'):
        assert W[n]['sub_batches'] == [1] and W[n]['hw'][0] * W[n]['hw'][1] < 600 * 600


def _out_bytes(case):
    import anchor_cases as A
    L = case['L']
    a = A._conv_args(L, case['form'], case['fast'])
    return 4 * L['B'] * a.Ho * a.Wo * L['cout']


def test_product_inventory_conditions():
    import anchor_cases as A
    convs, small = A.product_inventory()
    assert convs and small
    bench = set()
    for wl in R.WORKLOADS:
        bench |= set(A.inventory(wl)[0])
    assert not set(convs) & bench                               # only launches the bench inventory does not hold
    cases = list(convs.values())

    def has(pred):
        return any(pred(c) for c in cases)
    halo = lambda c: c['form'] == 'direct' and c['slot'].startswith('conv3x3_halo<')
    assert has(lambda c: c['form'] == 'wino4') and has(lambda c: c['form'] == 'wino_up2')
    assert has(lambda c: halo(c) and 'up2=false' in c['slot'])
    assert has(lambda c: halo(c) and 'up2=true' in c['slot'] and c['L']['up2'])          # x2 as 4 phase filters
    assert has(lambda c: c['form'] == 'split3x3') and has(lambda c: c['form'] == 'split1x1')
    assert has(lambda c: c['form'] == 'direct' and c['L']['ksz'] == 4 and c['L']['cin'] == 3)     # in_conv (fp32 implicit GEMM)
    assert has(lambda c: c['slot'].startswith('conv3x3_cout3<') and c['L']['key'] == 'out_conv')
    assert has(lambda c: c['L']['kind'] == 'conv' and c['L']['ksz'] == 3 and c['L']['H'] != c['L']['W'])     # rectangular
    assert any(L['kind'] == 'attn' and L['H'] != L['W'] for L in small.values())
    assert any(L['kind'] == 'pad' and L['Hp'] != L['Wp'] for L in small.values())
    assert any(L['kind'] == 'ln' and L['rows'] == 16 * 144 * 144 for L in small.values())
    nb = [_out_bytes(c) for c in cases]
    assert any(b > 2 ** 32 for b in nb)
    assert any(2 ** 31 < b < 2 ** 32 for b in nb)
    assert any(0.9 * 2 ** 31 <= b < 2 ** 31 for b in nb)
    # the whole-image branch at 599x599 (608^2 after test()'s pad): the mixed plan on both sides of the Winograd per-image limit
    w599, _ = A.inventory('whole599x599_x4')
    res = [c for c in w599.values() if c['L']['pro'] and c['L']['behind']]
    got = {(c['L']['cin'], c['L']['H'], c['form'], c['slot'].split('<')[0]) for c in res}
    assert (256, 608, 'wino4', 'conv3x3_wino4') in got
    assert (128, 1216, 'direct', 'conv3x3_halo') in got and (64, 2432, 'direct', 'conv3x3_halo') in got
    assert not any(c['form'] == 'wino4' and c['L']['cin'] < 256 for c in res)
    up = {(c['L']['cout'], c['form'], 'up2=true' in c['slot']) for c in w599.values() if c['L']['up2'] and c['L']['cout'] in (128, 64)}
    assert up == {(128, 'direct', True), (64, 'direct', True)}


def test_positions_cover_the_images_where_offsets_wrap():
    """B = 16 of 1152^2 x 64 fp32 (5.4 GB): a multiple of 2^31 bytes falls into images 6 and 12; B = 8: image 6; under 2^31: none."""
    ib = 1152 * 1152 * 64 * 4
    assert R.straddle_images(6, ib) == [] and R.straddle_images(8, ib) == [6, 7] and R.straddle_images(16, ib) == [6, 7, 12, 13]
    for B in (8, 16):
        for k in range(1, B * ib // 2 ** 31 + 1):
            n = k * 2 ** 31 // ib
            assert n * ib <= k * 2 ** 31 < (n + 1) * ib and n in R.straddle_images(B, ib) and min(n + 1, B - 1) in R.straddle_images(B, ib)
    assert R.straddle_images(4, 2 ** 30) == [1, 2, 3]           # the boundary is an image seam: the image before, at and after it
    imgs = R.straddle_images(16, ib)
    pos = R.conv_positions(16, 1152, 1152, 3, images=imgs)
    for n in [0, 15] + imgs:
        p = pos[pos[:, 0] == n]
        ys, xs = set(p[:, 1].tolist()), set(p[:, 2].tolist())
        assert {0, 1151} <= ys and {0, 1151} <= xs, n                                    # corners and borders
        assert {7, 8, 15, 16, 1144, 1151} & ys and {15, 16, 1136, 1151} & xs, n          # tile seams, the last tile
        have = set(map(tuple, p[:, 1:].tolist()))           # the whole structured grid (no subsampling at six images)
        assert all((y, x) in have for y in R.axis_samples(1152, (8, 16)) for x in R.axis_samples(1152, (16,))), n
    # without images= the sampling is what it was: first and last image only
    old = R.conv_positions(16, 1152, 1152, 3)
    assert len(old[(old[:, 0] != 0) & (old[:, 0] != 15)]) <= 64
    wins = R.attention_windows(16, 72, 72, 8, 1, images=imgs)
    assert {n for n, _, _ in wins} >= set([0, 15] + imgs)


def test_halo_kernels_leave_at_2_to_31_input_elements():
    """The halo form, the out_conv kernel and the bf16x3 halo form hold the input patch offset as a 32-bit ELEMENT offset; the
    shape rule they share (femasr_conv_halo_eligible / femasr_conv_bf16x3_shape_ok: B*H*W*Cin < 2^31) sends a larger input to the
    generic implicit-GEMM form, which indexes with 64 bits, or refuses (bf16x3: before any HIP call) - marker pointers only."""
    import ctypes
    from femasr_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)

    def name(B, H, W, cin, cout, up2=0, pro=0):
        a = _lib.ConvArgs()
        a.B, a.H, a.W, a.Cin, a.Cout, a.ksz, a.stride, a.pad, a.up2, a.prologue = B, H, W, cin, cout, 3, 1, 1, up2, pro
        a.Ho, a.Wo = (2 * H, 2 * W) if up2 else (H, W)
        a.w, a.w_up2 = 1, (1 if up2 else None)
        _lib.check(lib.femasr_debug_conv_variant_name(ctypes.byref(a), buf, len(buf)))
        return buf.value.decode()
    # 64 channels x 2048^2 = 2^28 elements per image: 7 images are under 2^31 elements, 8 are at it
    assert name(7, 2048, 2048, 64, 64, pro=1).startswith('conv3x3_halo<')
    assert name(7, 2048, 2048, 64, 3).startswith('conv3x3_cout3<')
    assert name(7, 2048, 2048, 64, 64, up2=1).startswith('conv3x3_halo<') and 'up2=true' in name(7, 2048, 2048, 64, 64, up2=1)
    for B in (8, 16, 18, 256):          # 2^31, 2^32, past 2^32 (the unsigned wrap), far past it
        for kw in (dict(cout=64, pro=1), dict(cout=3), dict(cout=64, up2=1)):
            n = name(B, 2048, 2048, 64, **kw)
            assert n.startswith('conv_igemm<'), (B, kw, n)
    # the example of a public knob set too high: 256 tiles of 128^2, out_conv input 256 x 576^2 x 64 = 5.4 G elements
    assert name(256, 576, 576, 64, 3).startswith('conv_igemm<')
    a = _lib.ConvArgs()
    a.B, a.H, a.W, a.Cin, a.Cout, a.ksz, a.stride, a.pad, a.Ho, a.Wo = 8, 2048, 2048, 64, 64, 3, 1, 1, 2048, 2048
    a.in_, a.w, a.bias, a.out, a.w_bf16x3 = 1, 1, 1, 1, 1
    assert lib.femasr_conv2d(None, ctypes.byref(a)) != 0 and b'bf16x3' in lib.femasr_last_error()
    a.B = 7
    _lib.check(lib.femasr_debug_conv_variant_name(ctypes.byref(a), buf, len(buf)))      # eligible below the limit


# ---------------------------------------------------------------- the inventories of the non-default modes
BF16X3_REACHABLE = [          # typed in: g_v16 rows 0-2, 6-11, 15-17 of kernels_conv_bf16.hip (what femasr_conv_bf16x3_pick_variant returns)
    'conv3x3_halo_bf16x3<8x16x128,FEMASR_PRO_NONE,up2=false,waves=2x2>',
    'conv3x3_halo_bf16x3<8x16x128,FEMASR_PRO_GN_SILU,up2=false,waves=2x2>',
    'conv3x3_halo_bf16x3<8x16x128,FEMASR_PRO_NONE,up2=true,waves=2x2>',
    'conv3x3_halo_bf16x3<8x16x32,FEMASR_PRO_NONE,up2=false,waves=4x1>',
    'conv3x3_halo_bf16x3<8x16x32,FEMASR_PRO_GN_SILU,up2=false,waves=4x1>',
    'conv3x3_halo_bf16x3<8x16x32,FEMASR_PRO_NONE,up2=true,waves=4x1>',
    'conv3x3_halo_bf16x3<8x16x256,FEMASR_PRO_NONE,up2=false,waves=1x4>',
    'conv3x3_halo_bf16x3<8x16x256,FEMASR_PRO_GN_SILU,up2=false,waves=1x4>',
    'conv3x3_halo_bf16x3<8x16x256,FEMASR_PRO_NONE,up2=true,waves=1x4>',
    'conv3x3_halo_bf16x3<8x16x64,FEMASR_PRO_NONE,up2=false,waves=2x2>',
    'conv3x3_halo_bf16x3<8x16x64,FEMASR_PRO_GN_SILU,up2=false,waves=2x2>',
    'conv3x3_halo_bf16x3<8x16x64,FEMASR_PRO_NONE,up2=true,waves=2x2>',
]


def _mode_cases(dm, lm):
    """Every case tests/test_gpu_mode_anchor.py launches for one mode: bench workloads + product shapes (before de-duplication)."""
    import anchor_cases as A
    out = {}
    for wl in R.WORKLOADS:
        out.update(A.inventory(wl, modes=(dm,), linear_math=lm, split_res2=True)[0])
    for n, subs in A.MODE_PRODUCT.items():
        out.update(A.inventory(n, modes=(dm,), linear_math=lm, sub_batches=subs, split_res2=True)[0])
    return out


def test_bf16x3_inventory_puts_every_conv_behind_the_lookup_on_the_matrix_cores():
    import anchor_cases as A
    for wl in R.WORKLOADS:
        convs, _ = A.inventory(wl, modes=('bf16x3',))
        behind = [c for c in convs.values() if c['L']['behind']]
        assert len(behind) >= 20
        for c in behind:
            if c['L']['key'] == 'out_conv':
                assert c['form'] == 'direct' and c['slot'].startswith('conv3x3_cout3<'), c['slot']
            else:
                assert c['form'] == 'bf16x3' and c['slot'].startswith('conv3x3_halo_bf16x3<'), (c['L']['key'], c['form'], c['slot'])
                assert c['slot'] in BF16X3_REACHABLE
        for c in convs.values():          # in front of the lookup nothing changes with decoder_math
            assert c['L']['behind'] or c['form'] != 'bf16x3'
    # beyond the kernel's size limit the planner's choice is the direct form (64-bit generic kernel): 2 x 4096^2 x 64 is exactly 2^31
    L = dict(B=2, H=4096, W=4096, cin=64, cout=64, ksz=3, stride=1, pad=1, up2=False, pro=True, act=0, behind=True)
    assert R.conv_form(L, 'bf16x3', 'bf16_split') == 'direct' and R.conv_form(dict(L, H=4094), 'bf16x3', 'bf16_split') == 'bf16x3'
    assert R.conv_form(dict(L, B=1, H=2048, W=2048, cin=128, up2=True, pro=False), 'bf16x3', 'bf16_split') == 'bf16x3'      # 2^29 in, 2^30 out
    assert R.conv_form(dict(L, B=2, H=2048, W=2048, cin=128, up2=True, pro=False), 'bf16x3', 'bf16_split') == 'direct'      # 2^31 out
    assert R.conv_form(dict(L, up2=True, B=1, H=64, W=64), 'bf16x3', 'bf16_split') == 'direct'                               # prologue with x2


def test_bf16x3_instantiations_are_all_launched():
    """Each of the 12 reachable instantiations has a case in what the mode module launches: in a bench or product inventory, or - for
    the ones no listed workload reaches - among anchor_cases.bf16x3_unit_cases(), which hold exactly those."""
    import anchor_cases as A
    assert len(set(BF16X3_REACHABLE)) == 12
    reached = {c['slot'] for c in _mode_cases('bf16x3', 'bf16_split').values() if c['form'] == 'bf16x3'}
    assert reached <= set(BF16X3_REACHABLE)
    unit = {c['slot'] for c in A.bf16x3_unit_cases()}
    missing = [n for n in BF16X3_REACHABLE if n not in reached | unit]
    print('\nbf16x3 instantiations no listed workload reaches (unit shapes): ' + ', '.join(sorted(set(BF16X3_REACHABLE) - reached)))
    assert not missing, f'no listed workload and no unit shape reaches: {missing}'
    assert unit == set(BF16X3_REACHABLE) - reached, 'the unit shapes are for the instantiations no workload reaches, and only those'
    assert len(reached) == 7


def test_direct_and_fp32_linear_inventories_hold_no_other_form():
    import anchor_cases as A
    direct = _mode_cases('fp32_direct', 'bf16_split')
    assert direct and not [c['slot'] for c in direct.values() if c['form'].startswith('wino') or c['form'] == 'bf16x3']
    assert any(c['L']['up2'] and 'up2=true' in c['slot'] and c['slot'].startswith('conv3x3_halo<') for c in direct.values())   # phase filters
    assert any(c['L']['nres'] == 2 and c['L']['pro'] and c['slot'].startswith('conv3x3_halo<') for c in direct.values())
    lin = _mode_cases('fp32', 'fp32')
    assert lin and not [c['slot'] for c in lin.values() if c['form'].startswith('split')]
    gemm = [c for c in lin.values() if R.gemm_fp32_layer(c['L'])]
    assert {(c['L']['cin'], c['L']['cout']) for c in gemm} >= {(256, 768), (256, 256), (256, 1024), (1024, 256), (256, 512)}
    assert all(c['slot'].startswith('gemm_dma<') for c in gemm), sorted({c['slot'] for c in gemm})
    assert max(c['L']['H'] for c in gemm) == 16 * 144 * 144 == 331776          # the CLI's 16 windows (82 944 rows and up at the bench's sub-batches)
    assert any(c['L']['stride'] == 2 and c['slot'].startswith('conv_igemm<') for c in lin.values())
    assert any(c['L']['act'] == 1 for c in gemm)


def test_skip_schedule_follows_the_mode():
    """run_tail: the encoder skip of decoder stage i + 1 is the in_add of that stage's x2 conv when the conv is in the wino_up2 form,
    otherwise the second residual of stage i's last conv.  LQ workloads: every decoder stage but the last hands a skip to the next;
    HQ: no skips.  (The slot names of the halo, bf16x3 and GEMM kernels do not tell the residual count, so the profile-slot coverage
    test on the GPU cannot see this schedule: this host test, written from model.hip run_tail, is what holds it.)"""
    import anchor_cases as A
    for wl_name, wl in R.WORKLOADS.items():
        sub_b = R.sub_batches(wl['batch'], R.BENCH_STREAMS)[0]
        by_mode = {dm: {l['key']: l for l in A._layers(wl_name, sub_b, dm) if l['kind'] == 'conv'} for dm in ('fp32', 'fp32_strict', 'fp32_direct', 'bf16x3')}
        assert by_mode['fp32'] == by_mode['fp32_strict'] and by_mode['fp32_direct'] == by_mode['bf16x3']
        wino, direct = by_mode['fp32'], by_mode['fp32_direct']
        assert list(wino) == list(direct)
        diff = sorted(k for k in wino if wino[k] != direct[k])
        depth = sum(1 for k in wino if k.startswith('decoder_group.') and k.endswith('.block.1'))
        if not wl['cfg']['LQ_stage']:
            assert not diff and not any(l['in_add'] or l['nres'] == 2 for l in wino.values())
            continue
        want = sorted([f'decoder_group.{i}.block.3.conv.5' for i in range(depth - 1)] + [f'decoder_group.{i + 1}.block.1' for i in range(depth - 1)])
        assert diff == want, (wl_name, diff)
        for i in range(depth - 1):
            a, b = f'decoder_group.{i}.block.3.conv.5', f'decoder_group.{i + 1}.block.1'
            assert (wino[a]['nres'], wino[b]['in_add']) == (1, True) and (direct[a]['nres'], direct[b]['in_add']) == (2, False)
            assert {k: v for k, v in wino[a].items() if k != 'nres'} == {k: v for k, v in direct[a].items() if k != 'nres'}
        assert not any(l['in_add'] for l in direct.values())
    # the schedule follows the FORM, not the mode's name: past the Winograd limit the default mode folds the skip into res2 as well
    big = {l['key']: l for l in A._layers('whole599x599_x4', 1, 'fp32') if l['kind'] == 'conv'}
    assert big['decoder_group.1.block.3.conv.5']['nres'] == 2 and not big['decoder_group.2.block.1']['in_add']


def test_mode_inventory_adds_only_what_the_default_inventories_lack():
    import anchor_cases as A
    default = set()
    for wl in R.WORKLOADS:
        default |= set(A.inventory(wl)[0])
    n = {}
    for dm, lm in A.MODES:
        convs, small = A.mode_inventory(list(R.WORKLOADS), dm, lm)
        assert convs and not set(convs) & default
        assert not small          # (workload_layers lists the moments pass of every GroupNorm in every mode: the default inventories hold them)
        assert not A.mode_inventory(dict(A.MODE_PRODUCT), dm, lm)[1]
        n[dm, lm] = len(convs)
        prod, _ = A.mode_inventory(dict(A.MODE_PRODUCT), dm, lm)
        assert prod and not set(prod) & (default | set(A.product_inventory(dict(A.MODE_PRODUCT))[0]))
        if lm == 'bf16_split':          # the 16-window launches behind the lookup: 5.4 GB tensors, past 2^32 bytes
            assert any(4 * c['L']['B'] * c['L']['H'] * c['L']['W'] * c['L']['cin'] > 2 ** 32 for c in prod.values())
        else:                           # the Swin layers at 16 windows: 331 776 rows
            assert any(c['L']['H'] == 331776 and c['L']['cin'] == 1024 for c in prod.values())
        res2 = [c for k, c in {**convs, **prod}.items() if c['L']['nres'] == 2]
        assert res2 and all(k[-1] == 'res2' for k, c in {**convs, **prod}.items() if c['L']['nres'] == 2)
    print('\nmode inventories (bench shapes, new cases): ' + ', '.join(f'{k[0]}/{k[1]} {v}' for k, v in n.items()))
    # gemm_fp32_layer cases take the constant calibrated for the LDS-DMA GEMM
    lin, _ = A.mode_inventory(list(R.WORKLOADS), 'fp32', 'fp32')
    assert any(R.gemm_fp32_layer(c['L']) and c['form'] == 'direct' for c in lin.values())

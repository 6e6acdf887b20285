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


@pytest.mark.parametrize('form', ['direct', 'wino4', 'wino_up2', 'split3x3'])
@pytest.mark.parametrize('mutation,kw', CONV_MUTATIONS, ids=[m for m, _ in CONV_MUTATIONS])
def test_conv_bound_rejects_wrong_reference(form, mutation, kw):
    """The correctly rounded fp64 result passes; the same check against the mutated reference fails."""
    x, w, b, pro, res, add, (ho, wo) = _conv_case(3, **kw)
    if form == 'wino_up2' and not kw.get('up2'):
        kw = dict(kw, up2=True)
        x, w, b, pro, res, add, (ho, wo) = _conv_case(3, **kw)
        pro = None
    up2 = kw.get('up2', False)
    pos = R.conv_positions(x.shape[0], ho, wo, 4)
    ref, mag, pt, rest = R.conv_ref(x, w.numpy(), b.numpy(), pos, 3, 1, 1, up2, pro=pro, res=res)
    bound = R.conv_bound(mag, pt, rest, form)
    got = _rounded(ref)
    R.check(got, ref, bound, 'correct')
    bad, bmag, bpt, brest = R.conv_ref(x, w.numpy(), b.numpy(), pos, 3, 1, 1, up2, pro=pro, res=res, mutate=mutation)
    assert R.rejects(lambda: R.check(got, bad, R.conv_bound(bmag, bpt, brest, form), mutation)), mutation


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
]


def test_calibration():
    from oracle import oracle as orc
    worst = {}
    for i, (form, (B, H, W, cin), cout) in enumerate(CAL):
        rng = np.random.default_rng(100 + i)
        ksz = 1 if form == 'split1x1' else (4 if form == 'gemm_fp32' else 3)
        pad = 0 if ksz == 1 else 1
        up2 = form == 'wino_up2'
        x = rng.standard_normal((B, H, W, cin)).astype(np.float32)
        w = (rng.standard_normal((cout, cin, ksz, ksz)) / math.sqrt(ksz * ksz * cin)).astype(np.float32)
        b = ((rng.random(cout) - 0.5) * 0.2).astype(np.float32)
        w_khwc = np.ascontiguousarray(w.transpose(2, 3, 1, 0))
        hv, wv = (2 * H, 2 * W) if up2 else (H, W)
        ho, wo = hv + 2 * pad - ksz + 1, wv + 2 * pad - ksz + 1
        r1 = rng.standard_normal((B, ho, wo, cout)).astype(np.float32)
        if form == 'split3x3':
            y = orc.conv3x3_bf16s(x, w_khwc, b, r1, None, 1)
        elif form == 'split1x1':
            y = orc.linear_bf16s(x.reshape(-1, cin), w.reshape(cout, cin), b, 0, r1.reshape(-1, cout)).reshape(B, ho, wo, cout)
        else:
            y = orc.conv2d(x, w_khwc, b, ksz, 1, pad, up2, 0, r1, None, wino=form in ('wino4', 'wino_up2'))
        pos = R.conv_positions(B, ho, wo, i)
        ref, mag, pt, rest = R.conv_ref(torch.as_tensor(x), w, b, pos, ksz, 1, pad, up2, res=[torch.as_tensor(r1)])
        got = torch.as_tensor(y[pos[:, 0], pos[:, 1], pos[:, 2]])
        worst[form] = max(worst.get(form, 0.0), _needed_c(got, ref, mag, pt, rest))
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

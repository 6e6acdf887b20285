"""CPU: the checker of decoder_math='fp16' (tests/fp16_ref.py) exercised against CPU models before it judges a GPU, the network-level
condition that separates fp16 grade from bf16 grade, and the Python surface of the mode.

The constant stays at C_F16 = 128 (fp64_ref.C_FORM['bf16x3']): both wrong models are rejected at it, at K = 9*64 and K = 9*256, and the
accepting model's worst ratio leaves far more than the required 4x of room (asserted below)."""
import numpy as np
import pytest
import torch

import fp16_ref as F
import fp64_ref as R

# (Cin, Cout, H, W): K = 9*64 and 9*256; two images, every output element checked
SHAPES = {'K576': (64, 32, 6, 9), 'K2304': (256, 32, 5, 7)}
_CASES = {}


def _case(name, pro):
    key = (name, pro)
    if key not in _CASES:
        cin, cout, h, w = SHAPES[name]
        g = torch.Generator().manual_seed(1234 + cin + int(pro))
        x = torch.randn((2, h, w, cin), generator=g)
        if pro:
            x = x * (0.5 + torch.rand(cin, generator=g)) + (torch.rand(cin, generator=g) - 0.5)
        wt = (torch.randn((cout, cin, 3, 3), generator=g) / np.sqrt(9 * cin)).numpy()
        bias = ((torch.rand(cout, generator=g) - 0.5) * 0.2).numpy()
        res = [torch.randn((2, h, w, cout), generator=g)]
        ab = None
        if pro:
            rng = np.random.default_rng(7)
            a, b, _, _ = R.gn_coeffs_ref(x, rng.uniform(0.5, 1.5, cin).astype(np.float32), rng.uniform(-0.3, 0.3, cin).astype(np.float32))
            ab = (a.float().numpy(), b.float().numpy())
        pos = F.all_positions(2, h, w)
        ref, mag, near, rest = F.conv_ref(x, wt, bias, pos, pro=ab, res=res)
        _CASES[key] = dict(x=x, w=wt, bias=bias, res=res, pro=ab, pos=pos, ref=ref, mag=mag, near=near, rest=rest)
    return _CASES[key]


def _model(c, operand):
    return F.model_fp32_sequential(c['x'], c['w'], c['bias'], c['pos'], pro=c['pro'], res=c['res'], operand=operand)


def test_rounding_helpers_agree_with_numpy_and_torch():
    g = torch.Generator().manual_seed(5)
    v = torch.cat([torch.randn(4096, generator=g, dtype=torch.float64) * s for s in (1e-7, 1e-4, 1.0, 300.0)] +
                  [torch.tensor([0.0, 65504.0, 65519.9, 1e5, -1e5, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -14, 1.0 + 2.0 ** -11])])
    want = torch.from_numpy(np.clip(v.numpy(), -65504.0, 65504.0).astype(np.float16).astype(np.float64))      # numpy rounds double -> half directly
    assert torch.equal(F.fp16_rne(v), want)
    assert float(F.fp16_rne(torch.tensor([1e5], dtype=torch.float64))) == 65504.0                               # finite in, finite out
    f32 = v.float()
    assert torch.equal(F.bf16_rne(f32.double()), f32.to(torch.bfloat16).double())
    tr = F.fp16_trunc(v)
    assert bool((tr.abs() <= v.clamp(-65504, 65504).abs()).all()) and bool(((tr - F.fp16_rne(v)).abs() <= F.ulp16(v)).all())
    # a value sitting 1e-9 relative off a midpoint is `near` for any error above that, one a quarter ulp away is not
    mid = torch.tensor([1.0 + 2.0 ** -11, 0.375 + 2.0 ** -13], dtype=torch.float64)
    assert bool((F.boundary_distance(mid * (1 + 1e-12)) < 1e-9).all())
    assert bool((F.boundary_distance(torch.tensor([1.0 + 2.0 ** -12], dtype=torch.float64)) == 2.0 ** -12).all())


@pytest.mark.parametrize('pro', [False, True], ids=['plain', 'gn_silu'])
@pytest.mark.parametrize('name', list(SHAPES))
def test_checker_accepts_the_fp32_sequential_model(name, pro):
    c = _case(name, pro)
    worst = R.check(_model(c, 'fp16'), c['ref'], F.conv_bound(c['mag'], c['near'], c['rest']), f'{name} model')
    print(f'{name} pro={pro}: fp32 sequential model worst err/bound {worst:.3g}, near elements {int((c["near"] > 0).sum())}')
    if not pro:
        assert not bool((c['near'] != 0).any())         # no prologue: the rounded operands are exact functions of the inputs
        # the room the constant has to leave over the accepting model: worst c the model needs, from err <= c u mag + 2u rest
        need = float((((_model(c, 'fp16').double() - c['ref']).abs() - 2 * R.U * c['rest']).clamp_min(0) / (R.U * c['mag'])).max())
        assert 4.0 * need <= F.C_F16, need


@pytest.mark.parametrize('operand', ['fp16_trunc', 'bf16'])
@pytest.mark.parametrize('name', list(SHAPES))
def test_checker_rejects_the_wrong_models(name, operand):
    c = _case(name, False)
    bound = F.conv_bound(c['mag'], c['near'], c['rest'])
    got = _model(c, operand)
    assert R.rejects(lambda: R.check(got, c['ref'], bound, f'{name} {operand}'))
    over = float(((got.double() - c['ref']).abs() > bound).double().mean())
    print(f'{name} {operand}: {100 * over:.1f} % of the elements over their bound')


def test_near_term_is_needed_and_sufficient_with_the_prologue():
    """With the GN + SiLU prologue the fp32 evaluation of the model flips a few roundings against the fp64 reference: the bound without the
    near term is exceeded only where near is set (if anywhere), and with it everything passes."""
    c = _case('K576', True)
    got = _model(c, 'fp16').double()
    err = (got - c['ref']).abs()
    bare = F.conv_bound(c['mag'], torch.zeros_like(c['near']), c['rest'])
    assert bool(((err <= bare) | (c['near'] > 0)).all())
    assert bool((err <= F.conv_bound(c['mag'], c['near'], c['rest'])).all())


# ---------------------------------------------------------------- the network condition
TABLE = {'x4_small_trained': (1.62e-3, 67.6, 8.9), 'hq_small_trained': (4.4e-4, 81.0, 6.4)}     # fp16 max abs, PSNR (peak 1), bf16 / fp16


@pytest.mark.parametrize('name', list(TABLE))
def test_emulation_reproduces_the_recorded_figures_and_separates_the_grades(name):
    e = F.emulated_images(name)
    y32, i32 = e[None]
    d16 = float(np.abs(e['fp16'][0] - y32).max())
    db16 = float(np.abs(e['bf16'][0] - y32).max())
    p16 = F.psnr(e['fp16'][0], y32, 1.0)
    print(f'{name}: fp16 max abs {d16:.3g} ({p16:.1f} dB), bf16 max abs {db16:.3g} ({F.psnr(e["bf16"][0], y32, 1.0):.1f} dB), ratio {db16 / d16:.2f}')
    assert np.array_equal(e['fp16'][1], i32) and np.array_equal(e['bf16'][1], i32)           # nothing in front of a lookup changes
    want, want_db, _ = TABLE[name]
    assert want / 1.5 <= d16 <= want * 1.5, d16
    assert abs(p16 - want_db) <= 20 * np.log10(1.5), p16                                        # the rms error within the same factor
    assert db16 > 2.0 * d16, (db16, d16)          # so `<= 2 E` on the GPU holds fp16 grade and refuses bf16 grade


# ---------------------------------------------------------------- the Python surface
def test_python_surface_knows_the_mode():
    from femasr_amd import _lib, inference
    from femasr_amd.archs import build_network
    from femasr_amd.archs.femasr_arch import FeMaSRNet
    net = build_network(dict(type='FeMaSRNet', codebook_params=[[32, 1024, 512]], LQ_stage=True, scale_factor=4, decoder_math='fp16'))
    assert net.decoder_math == 'fp16' and FeMaSRNet.DECODER_MATH['fp16'] == 4
    assert FeMaSRNet.DECODER_MATH == {'fp32': 0, 'bf16x3': 1, 'fp32_direct': 2, 'fp32_strict': 3, 'fp16': 4}
    with pytest.raises(ValueError, match='decoder_math'):
        build_network(dict(type='FeMaSRNet', codebook_params=[[32, 1024, 512]], LQ_stage=True, scale_factor=4, decoder_math='fp8'))
    assert inference.build_parser().parse_args(['--decoder-math', 'fp16']).decoder_math == 'fp16'
    with pytest.raises(SystemExit):
        inference.build_parser().parse_args(['--decoder-math', 'fp8'])
    assert _lib.ABI_VERSION == 107 and _lib.ConvArgs._fields_[-1][0] == 'w_f16'
    assert {'femasr_repack_oihw_f16', 'femasr_packed_weight_f16_bytes'} <= set(_lib.SIGNATURES)


def test_model_option_reaches_the_network():
    """`network_g: decoder_math: fp16` of an options file lands on the built network (FeMaSRModel builds network_g through build_network)."""
    from femasr_amd.archs import build_network
    opt = dict(type='FeMaSRNet', codebook_params=[[32, 1024, 512]], LQ_stage=False, decoder_math='fp16')
    assert build_network(opt).decoder_math == 'fp16'

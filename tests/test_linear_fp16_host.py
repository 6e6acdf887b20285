"""CPU: the checker of linear_math='fp16' (tests/fp16_front_ref.py) exercised against CPU models before it judges a GPU, the network-level
emulation with the near-tie rule and its control, and the Python surface of the mode.

The GEMM constant stays at C = fp64_ref.C_FORM['bf16x3'] = 128: at K = 64 and K = 1024 the checker accepts the model with one sequential fp32
accumulator and rejects, as whole cases, the models with truncating conversion and with bf16 operands."""
import numpy as np
import pytest
import torch

import fp16_front_ref as FR
import fp16_ref as F16
import fp64_ref as R

# (K, N, M)
SHAPES = {'K64': (64, 48, 70), 'K1024': (1024, 40, 33)}
_CASES = {}


def _case(name):
    if name not in _CASES:
        k, n, m = SHAPES[name]
        g = torch.Generator().manual_seed(4321 + k)
        a = torch.randn((m, k), generator=g) * (0.5 + torch.rand(k, generator=g))
        w = torch.randn((n, k), generator=g) / np.sqrt(k)
        bias = (torch.rand(n, generator=g) - 0.5) * 0.2
        res = torch.randn((m, n), generator=g)
        ref, mag, rest = FR.gemm_ref(a, w, bias, res)
        _CASES[name] = dict(a=a, w=w, bias=bias, res=res, ref=ref, mag=mag, rest=rest)
    return _CASES[name]


@pytest.mark.parametrize('name', list(SHAPES))
def test_checker_accepts_the_fp32_sequential_model(name):
    c = _case(name)
    got = FR.model_fp32_sequential(c['a'], c['w'], c['bias'], c['res'])
    worst = R.check(got, c['ref'], FR.gemm_bound(c['mag'], c['rest']), f'{name} model')
    need = float((((got.double() - c['ref']).abs() - 2 * R.U * c['rest']).clamp_min(0) / (R.U * c['mag'])).max())
    print(f'{name}: fp32 sequential model worst err/bound {worst:.3g}, the c it needs {need:.3g} of {FR.C_GEMM}')
    assert 4.0 * need <= FR.C_GEMM, need


@pytest.mark.parametrize('operand', ['fp16_trunc', 'bf16'])
@pytest.mark.parametrize('name', list(SHAPES))
def test_checker_rejects_the_wrong_models(name, operand):
    c = _case(name)
    bound = FR.gemm_bound(c['mag'], c['rest'])
    got = FR.model_fp32_sequential(c['a'], c['w'], c['bias'], c['res'], operand=operand)
    assert R.rejects(lambda: R.check(got, c['ref'], bound, f'{name} {operand}'))
    over = float(((got.double() - c['ref']).abs() > bound).double().mean())
    print(f'{name} {operand}: {100 * over:.1f} % of the elements over their bound')


def test_gemm_ref_without_bias_and_residual():
    c = _case('K64')
    ref, mag, rest = FR.gemm_ref(c['a'], c['w'])
    assert torch.equal(rest, ref.abs()) and bool((mag >= ref.abs()).all())
    R.check(FR.model_fp32_sequential(c['a'], c['w']), ref, FR.gemm_bound(mag, rest), 'K64 bare')


# ---------------------------------------------------------------- the network-level emulation
NET_CASES = ['x4_small_trained', 'x2_small_trained', 'hq_small_trained']


@pytest.mark.parametrize('name', NET_CASES)
def test_emulation_flips_few_tokens_and_each_is_a_near_tie(name):
    ref, emu = FR.emulated(name, None), FR.emulated(name, 'fp16')
    tokens = ref['idx'].size
    delta = FR.token_delta(emu['z0'], ref['z0'])
    flips, bad = FR.near_tie_failures(ref['idx'], emu['idx'], ref['d0'], FR.codebook0(name), delta)
    d = float(np.abs(emu['y'] - ref['y']).max())
    print(f'{name}: {tokens} tokens, {flips} flipped, image max abs {d:.3g} ({F16.psnr(emu["y"], ref["y"], 1.0):.1f} dB), Delta {delta:.3g}')
    assert flips <= FR.FLIP_CAP * tokens, (flips, tokens)
    assert not bad, bad
    assert d > 0.0                                       # the mode is another arithmetic: the image moves even without a flip


def test_bf16_operands_are_worse_than_fp16():
    name = 'x4_small_trained'
    ref, e16, eb = FR.emulated(name, None), FR.emulated(name, 'fp16'), FR.emulated(name, 'bf16')
    f16, fb = int((e16['idx'] != ref['idx']).sum()), int((eb['idx'] != ref['idx']).sum())
    p16, pb = F16.psnr(e16['y'], ref['y'], 1.0), F16.psnr(eb['y'], ref['y'], 1.0)
    print(f'{name}: fp16 {f16} flips {p16:.1f} dB, bf16 {fb} flips {pb:.1f} dB')
    assert fb > f16 or pb < p16


@pytest.mark.parametrize('name', NET_CASES)
def test_near_tie_rule_rejects_random_codes(name):
    """The control: 1 % of the indices replaced by random other codes is no set of near ties."""
    ref, emu = FR.emulated(name, None), FR.emulated(name, 'fp16')
    rng = np.random.default_rng(17)
    idx = ref['idx'].reshape(-1).copy()
    n = max(1, int(round(0.01 * idx.size)))
    n_e = ref['d0'].shape[1]
    for t in rng.choice(idx.size, n, replace=False):
        idx[t] = (idx[t] + 1 + rng.integers(0, n_e - 1)) % n_e
    flips, bad = FR.near_tie_failures(ref['idx'], idx, ref['d0'], FR.codebook0(name), FR.token_delta(emu['z0'], ref['z0']))
    assert flips == n and bad, (flips, bad)


def test_forced_indices_reach_the_decoder():
    """emulation_net(forced_indices=...): the lookup returns the forced codes; forcing a net's own indices changes nothing."""
    name = 'hq_small_trained'
    ref = FR.emulated(name, None)
    same = FR.emulated(name, None, forced=ref['idx'], tag='own')
    assert np.array_equal(same['y'], ref['y']) and np.array_equal(same['idx'], ref['idx'])
    other = ref['idx'].copy()
    other.reshape(-1)[0] = (other.reshape(-1)[0] + 1) % ref['d0'].shape[1]
    moved = FR.emulated(name, None, forced=other, tag='one_changed')
    assert np.array_equal(moved['idx'], other) and not np.array_equal(moved['y'], ref['y'])
    assert np.array_equal(moved['d0'], ref['d0'])       # the recorded distances are the net's own, whatever is forced


# ---------------------------------------------------------------- the Python surface
def test_python_surface_knows_the_mode():
    from femasr_amd import _lib, inference
    from femasr_amd.archs import build_network
    from femasr_amd.archs.femasr_arch import FeMaSRNet
    opt = dict(type='FeMaSRNet', codebook_params=[[32, 1024, 512]], LQ_stage=True, scale_factor=4)
    net = build_network(dict(opt, linear_math='fp16'))
    assert net.linear_math == 'fp16' and FeMaSRNet.LINEAR_MATH == {'fp32': 0, 'bf16_split': 1, 'fp16': 2}
    assert build_network(opt).linear_math == 'bf16_split'                      # the default does not change
    with pytest.raises(ValueError, match="linear_math must be 'bf16_split', 'fp32' or 'fp16'"):
        build_network(dict(opt, linear_math='fp8'))
    assert {'femasr_repack_k1_f16', 'femasr_packed_weight_k1_f16_bytes'} <= set(_lib.SIGNATURES)
    assert _lib.ConvArgs._fields_[-1][0] == 'w_f16'                            # the k1 meaning adds no field
    p = inference.build_parser()
    a = p.parse_args([])
    assert (a.linear_math, a.decoder_math) == ('bf16_split', 'fp32')
    a = p.parse_args(['--half'])
    assert (a.linear_math, a.decoder_math) == ('fp16', 'fp16')
    a = p.parse_args(['--linear-math', 'fp16'])
    assert (a.linear_math, a.decoder_math) == ('fp16', 'fp32')
    a = p.parse_args(['--half', '--decoder-math', 'fp32'])                     # a later flag overrides its side
    assert (a.linear_math, a.decoder_math) == ('fp16', 'fp32')
    with pytest.raises(SystemExit):
        p.parse_args(['--linear-math', 'fp8'])


def test_model_option_reaches_the_network():
    """`network_g: linear_math: fp16` of an options file lands on the built network (FeMaSRModel and femasr_amd.test build network_g through
    build_network)."""
    from femasr_amd.archs import build_network
    opt = dict(type='FeMaSRNet', codebook_params=[[32, 1024, 512]], LQ_stage=False, linear_math='fp16', decoder_math='fp16')
    net = build_network(opt)
    assert (net.linear_math, net.decoder_math) == ('fp16', 'fp16')

"""Pins the CPU oracle (oracle/) against golden vectors produced by the REFERENCE itself
(tests/golden/make_golden.py imports /root/reference and records its outputs).
Tolerance: 1e-3 max-abs fp32 on outputs (north-star bound); VQ indices bit-exact, with the
documented near-tie allowance (helpers.check_indices_near_tie) — every committed fixture
currently matches with ZERO mismatches, which the tests assert."""
import numpy as np
import pytest

from femasr_amd import synth
from helpers import (assert_golden_probes, cfg_name_of, check_indices_near_tie, load_golden, oracle_net, synth_weights)

TOL = 1e-3


def _run(name, linear_math='bf16_split'):
    g = load_golden(name)
    cn = cfg_name_of(g)
    net = oracle_net(cn, synth_weights(cn, int(g['seed']), str(g['codebook'])), linear_math)
    x = synth.synth_input(int(g['input_seed']), tuple(g['in_shape']))
    return g, net, x


@pytest.mark.parametrize('linear_math', ['bf16_split', 'fp32'])
@pytest.mark.parametrize('name', ['x4_small_init', 'x4_small_trained', 'x2_small_trained'])
def test_test_path_matches_reference(name, linear_math):
    """Both arithmetics of the 1x1 / Linear layers against the reference: the product default and the fp32 chain."""
    g, net, x = _run(name, linear_math)
    net.probes = {}
    y, idx = net.test(x, return_indices=True)
    assert y.shape == tuple(g['out_shape'])
    assert np.abs(y - g['output']).max() < TOL
    nbad, nacc = check_indices_near_tie(idx, g)
    assert nbad == 0, f'{nbad} index mismatches ({nacc} would be near-tie acceptable)'
    assert idx.dtype == np.int64 and idx.shape == g['vq_indices'].shape
    assert_golden_probes(g, net.probes, f'{name} {linear_math}')


def test_hq_forward_matches_reference():
    g, net, x = _run('hq_small_trained')
    net.probes = {}
    y, idx = net.forward(x)
    assert_golden_probes(g, net.probes, 'hq_small_trained')
    assert np.abs(y - g['output']).max() < TOL
    assert np.array_equal(idx, g['vq_indices'])


def test_test_tile_matches_reference():
    g, net, x = _run('x4_tiled_trained', 'fp32')
    y = net.test_tile(x, int(g['kw_tile_size']), int(g['kw_tile_pad']))
    assert y.shape == tuple(g['out_shape'])
    assert np.abs(y - g['output']).max() < TOL


def test_decode_indices_matches_reference():
    g = load_golden('hq_decode_indices')
    net = oracle_net('hq', synth_weights('hq', int(g['seed']), str(g['codebook'])))
    y = net.decode_indices(g['indices'])
    assert np.abs(y - g['output']).max() < TOL


def test_full_tile_128_matches_reference():
    """One full-size x4 tile (128x128 -> 512x512, 964 GFLOP).  In the fp32-chain arithmetic by default (~15 s of CPU); FEMASR_SLOW_TESTS=1
    runs it in the PRODUCT DEFAULT arithmetic (linear_math 'bf16_split': the linears and the 3x3 convs in front of the lookup through the
    restated matrix instruction, ~3 min on 8 cores; verified in round 6: 0 index mismatches).  The default arithmetic is pinned on the CPU
    in every run by the real image tests/test_oracle_golden_r2.py::test_cli_arithmetic_on_testset_png[png_chip] and by every
    small fixture; the GPU suite runs this tile in the default."""
    import os
    lm = 'bf16_split' if os.environ.get('FEMASR_SLOW_TESTS') == '1' else 'fp32'
    g, net, x = _run('x4_tile128_trained', lm)
    net.probes = {}
    y, idx = net.test(x, return_indices=True)
    assert_golden_probes(g, net.probes, f'x4_tile128_trained {lm}')
    st = int(g['out_stride'])
    assert np.abs(y[:, :, ::st, ::st] - g['output']).max() < TOL
    assert abs(float(y.astype(np.float64).mean()) - float(g['out_mean'])) < 1e-5
    nbad, _ = check_indices_near_tie(idx, g)
    assert nbad == 0


@pytest.mark.parametrize('name', ['x4_small_trained', 'x2_small_trained'])
def test_direct_form_oracle_matches_reference(name):
    """OracleNet(winograd=False) -- the arithmetic of decoder_math='fp32_direct' (every conv in the direct form) -- against the
    same reference goldens, and the two restatements against each other: identical VQ indices, outputs within fp32 rounding."""
    from oracle import oracle as orc
    from helpers import CONFIGS
    g, net, x = _run(name, 'fp32')
    cn = cfg_name_of(g)
    cfg = CONFIGS[cn]
    direct = orc.OracleNet(synth_weights(cn, int(g['seed']), str(g['codebook'])), codebook_params=cfg['codebook_params'],
                           LQ_stage=cfg['LQ_stage'], scale_factor=cfg.get('scale_factor', 4), winograd=False, linear_math='fp32')
    yd, idd = direct.test(x, return_indices=True)
    yw, idw = net.test(x, return_indices=True)
    assert np.abs(yd - g['output']).max() < TOL
    assert check_indices_near_tie(idd, g)[0] == 0
    assert np.array_equal(idd, idw)
    assert 0 < np.abs(yd - yw).max() < 1e-4

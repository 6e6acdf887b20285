"""LPIPS host logic without a GPU: the weight loader's name mapping, the size rules against torch, and the fp64 restatement."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_ref
from femasr_amd import lpips as L
from femasr_amd import synth


def _state(net, seed=5):
    return {k: torch.from_numpy(v) for k, v in synth.lpips_state(L.expected_shapes(net), seed).items()}


def _slice_of(key):
    return key.split('.')[1]


@pytest.mark.parametrize('net', ['alex', 'vgg'])
def test_loader_maps_all_layouts_to_the_same_tensors(net, tmp_path):
    sd = _state(net)
    # 1: one file, lpips / pyiqa names, BasicSR-style nesting and DataParallel prefixes, plus a scaling-layer buffer to ignore
    one = {'params': {'module.' + k: v for k, v in sd.items()}}
    one['params']['module.scaling_layer.shift'] = torch.zeros(1, 3, 1, 1)
    torch.save(one, str(tmp_path / 'one.pth'))
    # 2: torchvision backbone (features.I.*, with classifier weights to ignore) + a head file
    tv = {f'features.{k.split(".")[2]}.{k.split(".")[3]}': v for k, v in sd.items() if k.startswith('net.')}
    tv['classifier.1.weight'] = torch.zeros(4, 4)
    torch.save({'state_dict': tv}, str(tmp_path / 'tv.pth'))
    torch.save({k: v for k, v in sd.items() if k.startswith('lin')}, str(tmp_path / 'heads.pth'))
    # 3: the heads under their ModuleList name lins.K
    torch.save({k.replace('lin', 'lins.', 1) if k.startswith('lin') else k: v for k, v in sd.items()}, str(tmp_path / 'lins.pth'))
    got = [L.load_lpips_weights(net, str(tmp_path / 'one.pth')),
           L.load_lpips_weights(net, str(tmp_path / 'heads.pth'), backbone_model_path=str(tmp_path / 'tv.pth')),
           L.load_lpips_weights(net, str(tmp_path / 'lins.pth'))]
    for g in got:
        assert list(g) == list(L.expected_shapes(net))
        for k in sd:
            assert torch.equal(g[k], sd[k]), k
    m = L.LPIPS(net, pretrained_model_path=str(tmp_path / 'one.pth'))
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_loader_names_missing_and_misshaped_keys():
    sd = _state('alex')
    part = {k: v for k, v in sd.items() if k not in ('net.slice3.6.bias', 'lin4.model.1.weight')}
    with pytest.raises(KeyError) as e:
        L.canonical_state_dict('alex', part)
    assert 'net.slice3.6.bias' in str(e.value) and 'lin4.model.1.weight' in str(e.value)
    with pytest.raises(KeyError, match='net.slice1.0.weight'):
        L.canonical_state_dict('alex', {'lin0.model.1.weight': sd['lin0.model.1.weight']})
    bad = dict(sd)
    bad['net.slice2.3.weight'] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(ValueError, match=r'net\.slice2\.3\.weight'):
        L.canonical_state_dict('alex', bad)
    with pytest.raises(KeyError):       # a VGG file is not an AlexNet file
        L.canonical_state_dict('alex', _state('vgg'))


def _torch_taps(net, h, w):
    """Tap sizes by running the restatement's layer list on the meta device (torch's own size rules; raises where torch does)."""
    shapes = L.expected_shapes(net)
    state = {k: torch.empty(s, device='meta') for k, s in shapes.items()}
    taps = lpips_ref.features(state, net, torch.empty(1, 3, h, w, device='meta'), dtype=torch.float32)
    return [(t.shape[2], t.shape[3], t.shape[1]) for t in taps]


@pytest.mark.parametrize('net,hw', [('alex', (31, 31)), ('alex', (33, 47)), ('alex', (97, 131)), ('alex', (255, 129)),
                                    ('vgg', (16, 16)), ('vgg', (17, 31)), ('vgg', (97, 131)), ('vgg', (63, 255))])
def test_tap_shapes_match_torch(net, hw):
    assert L.tap_shapes(net, *hw) == _torch_taps(net, *hw)


@pytest.mark.parametrize('net,small', [('alex', (30, 64)), ('alex', (64, 30)), ('vgg', (15, 40)), ('vgg', (40, 15))])
def test_minimum_size_matches_torch(net, small):
    with pytest.raises(RuntimeError):
        _torch_taps(net, *small)
    with pytest.raises(ValueError, match=str(L.MIN_SIDE[net])):
        L.tap_shapes(net, *small)
    L.tap_shapes(net, L.MIN_SIDE[net], L.MIN_SIDE[net])


@pytest.mark.parametrize('net,hw', [('alex', (64, 96)), ('vgg', (32, 48))])
def test_restatement_properties(net, hw):
    sd = {k: v.numpy() for k, v in _state(net).items()}
    a = synth.synth_input(1, (2, 3) + hw)
    b = synth.synth_input(2, (2, 3) + hw)
    tot, terms = lpips_ref.lpips(sd, net, a, a)
    assert np.all(tot == 0.0) and np.all(terms == 0.0)
    tab, terms_ab = lpips_ref.lpips(sd, net, a, b)
    tba, _ = lpips_ref.lpips(sd, net, b, a)
    assert np.array_equal(tab, tba)
    assert np.all(tab > 0) and np.all(terms_ab >= 1e-3 * tab[:, None]), terms_ab / tab[:, None]     # no dead tap on the synthetic weights


def test_restatement_head_is_the_definition():
    rng = np.random.RandomState(0)
    f0, f1 = rng.rand(2, 64, 5, 7), rng.rand(2, 64, 5, 7)
    w = rng.rand(1, 64, 1, 1) / 64
    n0 = f0 / (np.sqrt((f0 ** 2).sum(1, keepdims=True)) + 1e-10)
    n1 = f1 / (np.sqrt((f1 ** 2).sum(1, keepdims=True)) + 1e-10)
    want = F.conv2d(torch.from_numpy((n0 - n1) ** 2), torch.from_numpy(w)).mean((1, 2, 3)).numpy()
    np.testing.assert_allclose(lpips_ref.head(torch.from_numpy(f0), torch.from_numpy(f1), w).numpy(), want, rtol=1e-14)


def test_module_refuses_unknown_keywords_and_warns_without_weights():
    with pytest.raises(TypeError):
        L.LPIPS('alex', pretrained_model_pth='x.pth')           # a typo must not build a randomly initialised metric
    with pytest.warns(UserWarning, match='without weights'):
        L.LPIPS('vgg')
    with pytest.raises(ValueError, match='pretrained_model_path'):
        L.LPIPS('alex', backbone_model_path='features.pth')

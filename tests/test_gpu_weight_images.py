"""-m gpu: the weight images a handle keeps per conv form (csrc/common.h ConvFormDesc, model.hip layer_forms) and femasr_conv2d's choice of form.

A layer holds an image for every form that a mode the handle has EVER selected can give it: from creation the forms of decoder_math
'fp32' / 'bf16x3' / 'fp32_direct' / 'fp32_strict' x linear_math 'fp32' / 'bf16_split'; the two fp16 forms join when their mode is first
selected, built from the handle's fp32 images.  femasr_debug_weight_image_bytes counts the bytes per form; the expected totals follow from
the key table and the public *_bytes functions.  The order in which the modes are selected must not show in the result.
"""
import ctypes
import re

import pytest
import torch

from anchor_cases import _slot
from femasr_amd import _lib

pytestmark = pytest.mark.gpu

DIRECT, BF16X3, WINO, WINO_UP2, SPLIT, F16, GEMM_F16 = range(7)       # ConvForm (csrc/common.h)
ENCODE_DEPTH = 1        # config 'x4': blocks.0 = down conv + two ResBlocks, blocks.1 = the Swin stage, blocks.2 / .3 = the up-blocks


def _case():
    import gpu_utils as G
    from femasr_amd import synth
    from helpers import cfg_name_of, load_golden, synth_weights
    g = load_golden('x4_small_trained')
    assert cfg_name_of(g) == 'x4'
    w = synth_weights('x4', int(g['seed']), str(g['codebook']))
    x = torch.from_numpy(synth.synth_input(int(g['input_seed']), tuple(g['in_shape']))).cuda()
    return G, w, x


def _bytes(net):
    lib, h = net._native(torch.device('cuda', torch.cuda.current_device()))       # pushes the weights, then the modes
    out = []
    for f in range(7):
        n = ctypes.c_size_t()
        _lib.check(lib.femasr_debug_weight_image_bytes(h, f, ctypes.byref(n)))
        out.append(int(n.value))
    return out


def _layers(net):
    """(key, shape) of the conv / linear weights of the handle, from femasr_weight_info."""
    lib, h = net._native(torch.device('cuda', torch.cuda.current_device()))
    out = []
    for i in range(lib.femasr_num_weights(h)):
        key, shape, ndim = ctypes.c_char_p(), (ctypes.c_int64 * 4)(), ctypes.c_int()
        _lib.check(lib.femasr_weight_info(h, i, ctypes.byref(key), ctypes.byref(shape), ctypes.byref(ndim)))
        k = key.value.decode()
        linear = ndim.value == 2 and k.endswith('.weight') and ('.attn.' in k or '.mlp.' in k)
        if ndim.value == 4 or linear:
            out.append((k, tuple(shape)))
    return out


def test_image_inventory(cuda_device):
    G, w, x = _case()
    lib = _lib.load()
    net = G.build_net('x4', w, decoder_math='fp32')
    b0 = _bytes(net)
    print('default modes:', b0)
    assert b0[F16] == 0 and b0[GEMM_F16] == 0
    assert all(b0[f] > 0 for f in (DIRECT, BF16X3, WINO, WINO_UP2, SPLIT))

    net.decoder_math = 'fp16'
    b1 = _bytes(net)
    print("decoder_math='fp16':", b1)
    # the bf16x3 form's layers by the same shape rule; a tile of 32 k x 32 columns is 1024 halfwords against 2048 (hi and lo)
    assert b1[F16] * 2 == b1[BF16X3] and b1[GEMM_F16] == 0
    assert [b1[f] for f in (DIRECT, BF16X3, WINO, WINO_UP2, SPLIT)] == [b0[f] for f in (DIRECT, BF16X3, WINO, WINO_UP2, SPLIT)]

    net.linear_math = 'fp16'
    b2 = _bytes(net)
    print("linear_math='fp16' as well:", b2)
    layers = _layers(net)
    k1 = [s for k, s in layers if s[2] == 1 and s[3] == 1 and s[1] % 64 == 0]
    assert k1 and b2[GEMM_F16] == sum(int(lib.femasr_packed_weight_k1_f16_bytes(s[0], s[1])) for s in k1)
    # the stride-1 3x3 convs in front of the lookup: the encoder's ResBlock convs and the conv behind each RSTB - not the stride-2 down
    # convs (blocks.N.0), not the LQ encoder's up-blocks (behind every lookup: they belong to decoder_math's set, counted above)
    front = [s for k, s in layers
             if (m := re.match(r'multiscale_encoder\.blocks\.(\d+)\.(.+)\.weight$', k)) and int(m.group(1)) <= ENCODE_DEPTH
             and s[2] == 3 and (re.match(r'[12]\.conv\.[25]$', m.group(2)) or re.match(r'swin_blks\.\d\.conv$', m.group(2)))]
    assert len(front) == 4 * ENCODE_DEPTH + 4
    assert b2[F16] - b1[F16] == sum(int(lib.femasr_packed_weight_f16_bytes(s[0], s[1], 3, 3)) for s in front) > 0
    assert [b2[f] for f in (DIRECT, BF16X3, WINO, WINO_UP2, SPLIT)] == [b0[f] for f in (DIRECT, BF16X3, WINO, WINO_UP2, SPLIT)]

    # re-selecting a mode and re-setting the weights change no number
    net.decoder_math, net.linear_math = 'fp32', 'bf16_split'
    assert _bytes(net) == b2
    net.decoder_math, net.linear_math = 'fp16', 'fp16'
    assert _bytes(net) == b2
    net.invalidate_weights()
    assert _bytes(net) == b2
    n = ctypes.c_size_t()
    assert lib.femasr_debug_weight_image_bytes(net._handle, 7, ctypes.byref(n)) == -1


def test_selection_order_does_not_show(cuda_device):
    G, w, x = _case()
    both = G.build_net('x4', w, decoder_math='fp16', linear_math='fp16')
    y, idx = both.test_with_indices(x)

    dec_first = G.build_net('x4', w, decoder_math='fp32')
    y0, i0 = dec_first.test_with_indices(x)
    dec_first.decoder_math = 'fp16'
    dec_first.test_with_indices(x)                               # a forward between the two switches
    dec_first.linear_math = 'fp16'
    lin_first = G.build_net('x4', w, decoder_math='fp32')
    lin_first.test_with_indices(x)
    lin_first.linear_math = 'fp16'
    lin_first.test_with_indices(x)
    lin_first.decoder_math = 'fp16'
    there_and_back = G.build_net('x4', w, decoder_math='fp16', linear_math='fp16')
    there_and_back.test_with_indices(x)
    there_and_back.decoder_math, there_and_back.linear_math = 'fp32', 'bf16_split'
    yb, ib = there_and_back.test_with_indices(x)
    assert torch.equal(yb, y0) and torch.equal(ib, i0)           # the defaults' bits, from a handle that holds the fp16 images
    there_and_back.decoder_math, there_and_back.linear_math = 'fp16', 'fp16'

    for name, net in (('decoder first', dec_first), ('linear first', lin_first), ('there and back', there_and_back)):
        yn, i_n = net.test_with_indices(x)
        assert torch.equal(yn, y) and torch.equal(i_n, idx), name
    assert not torch.equal(y, y0)
    dec_first.decoder_math, dec_first.linear_math = 'fp32', 'bf16_split'
    yd, i_d = dec_first.test_with_indices(x)
    assert torch.equal(yd, y0) and torch.equal(i_d, i0)


def _args(cin=64, cout=64, ksz=3, stride=1, **images):
    a = _lib.ConvArgs()
    a.B, a.H, a.W, a.Cin, a.Cout, a.ksz, a.stride, a.pad = 1, 8, 16, cin, cout, ksz, stride, ksz // 2
    a.Ho, a.Wo = 8 // stride, 16 // stride
    for k, v in images.items():
        setattr(a, k, v)
    return a


def test_conv2d_precedence_among_the_images_given(cuda_device):
    """femasr_debug_conv_variant_name picks the form as femasr_conv2d does and launches nothing: the pointers are never read."""
    assert _slot(_args(w=1)).startswith('conv')
    assert _slot(_args(w=1, w_bf16x3=1, w_f16=1)).startswith('conv3x3_halo_bf16x3<')
    assert _slot(_args(w=1, w_f16=1, w_wino=1)).startswith('conv3x3_halo_f16<')
    assert _slot(_args(w=1, w_wino=1)).startswith('conv3x3_wino4')
    up2 = _args(w=1, w_wino=1, up2=1)
    up2.Ho, up2.Wo = 16, 32
    assert _slot(up2).startswith('conv3x3_wino_up2<')
    split = {_slot(_args(ksz=1, w=1, w_bf16s=1, **{other: 1})) for other in ('w_bf16x3', 'w_f16', 'w_wino')}
    assert len(split) == 1 and split.pop().startswith('gemm_bf16s')
    assert _slot(_args(ksz=1, w=1, w_f16=1)).startswith('gemm_f16')


REFUSALS = [        # a form given on a shape it refuses: FEMASR_ERR_INVALID with the form's message, nothing launched
    (dict(w_bf16s=1, stride=4), b'conv2d: w_bf16s given but the layer is neither a 1x1 stride-1 layer nor a 3x3 pad-1 conv of stride 1 or 2, with Cin % 64 == 0 and no prologue'),
    (dict(w_bf16x3=1, cin=48), b'conv2d: w_bf16x3 given but the layer is not eligible for the bf16x3 path'),
    (dict(w_f16=1, cin=48), b'conv2d: w_f16 given but the layer is not eligible for the fp16 path (the bf16x3 shape rule)'),
    (dict(w_f16=1, ksz=1, cin=32), b'conv2d: w_f16 given with ksz = 1 but the layer is not a 1x1 stride-1 layer with Cin % 64 == 0 and no prologue'),
    (dict(w_wino=1, up2=1, cout=32), b'conv2d: w_wino given with up2 but the layer is not a 3x3 stride-1 pad-1 conv with Cin % 32 == 0, Cout % 64 == 0, no prologue'),
    (dict(w_wino=1, cout=32), b'conv2d: w_wino given but the layer is not a 3x3 stride-1 pad-1 conv with Cin % 32 == 0, Cout % 64 == 0'),
]


@pytest.mark.parametrize('case', REFUSALS, ids=[next(iter(c[0])) + ('_k1' if c[0].get('ksz') == 1 else '_up2' if c[0].get('up2') else '') for c in REFUSALS])
def test_conv2d_refuses_a_form_on_a_shape_outside_its_rule(cuda_device, case):
    kw, message = case
    lib = _lib.load()
    a = _args(w=1, **kw)
    assert lib.femasr_conv2d(None, ctypes.byref(a)) == -1
    assert lib.femasr_last_error() == message

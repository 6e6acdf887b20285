"""The final resample of the output image (femasr_amd/resample.py) without a GPU: the definition, the size arithmetic, the
command line's two flags and the header.  The definition is held to femasr_model.imresize, the project's MATLAB bicubic, bit for bit where
that one can express the case; the GPU side is held to the definition in test_gpu_resample.py."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from femasr_amd import _lib, inference, resample as RS
from femasr_amd.models.femasr_model import imresize, imresize_tables
from resample_utils import step_image, tie_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_identity_is_bit_exact():
    img = np.random.default_rng(1).integers(0, 256, (13, 17, 3), dtype=np.uint8)
    out = RS.resample_ref(img, 13, 17)
    assert out.dtype == np.uint8 and out.shape == img.shape and np.array_equal(out, img)
    w, idx = imresize_tables(13, 13, 1.0, True)
    assert w.shape[1] == 4 and np.array_equal(np.sort(w, axis=1)[:, -1], np.ones(13)) and np.array_equal((w != 0).sum(1), np.ones(13))
    assert np.array_equal(RS.resample_ref(img[..., 0], 13, 17), img[..., 0])      # (H,W) stays (H,W)


@pytest.mark.parametrize('v', [0, 1, 127, 128, 254, 255])
def test_flat_images_stay_flat(v):
    img = np.full((11, 13), v, np.uint8)
    for oh, ow in ((8, 10), (17, 20), (3, 4)):
        out = RS.resample_ref(img, oh, ow)
        assert out.shape == (oh, ow) and (out == v).all(), (v, oh, ow, np.unique(out))


def test_both_clips_are_reached():
    vals = RS.resample_values(step_image(), 24, 24)
    assert vals.min() < -15 and vals.max() > 270, (vals.min(), vals.max())         # -15.9 and 270.9
    out = RS.resample_ref(step_image(), 24, 24)
    assert out.min() == 0 and out.max() == 255
    assert (out[vals < 0] == 0).all() and (out[vals > 255] == 255).all()


def test_a_true_tie_rounds_to_even():
    vals = RS.resample_values(tie_image(), 3, 3)
    assert vals[1, 1, 0] == 151.5 and vals[1, 1, 1] == 120.5, vals[1, 1]           # exactly on .5, one below an even byte and one above
    out = RS.resample_ref(tie_image(), 3, 3)
    assert out[1, 1, 0] == 152 and out[1, 1, 1] == 120, out[1, 1]                  # half to even: up, and down


def test_consistent_with_imresize():
    img = np.random.default_rng(2).integers(0, 256, (16, 16), dtype=np.uint8)
    vals = RS.resample_values(img, 12, 12)
    want = imresize(img.astype(np.float64), 0.75)
    assert want.shape == (12, 12) and np.array_equal(vals.view(np.int64), want.view(np.int64))
    rgb = np.random.default_rng(3).integers(0, 256, (16, 16, 3), dtype=np.uint8)
    vals = RS.resample_values(rgb, 12, 12)
    for c in range(3):                                                              # every channel on its own
        assert np.array_equal(vals[..., c], imresize(rgb[..., c].astype(np.float64), 0.75))


def test_refusals():
    for n, o in ((8, 1), (4, 1), (1, 4), (1, 1)):
        with pytest.raises(ValueError):
            imresize_tables(n, o, o / n, True)
        for shape, size in (((n, 16), (o, 16)), ((16, n), (16, o))):
            with pytest.raises(RS.ResampleTooSmall):
                RS.resample_ref(np.zeros(shape, np.uint8), *size)
    assert issubclass(RS.ResampleTooSmall, ValueError) and issubclass(RS.ResampleRatio, ValueError)
    assert imresize_tables(24, 3, 3 / 24, True)[0].shape == (3, 32)
    for n, o in ((24, 3), (3, 24), (2, 16)):
        assert RS.resample_ref(np.full((n, n, 2), 9, np.uint8), o, o).shape == (o, o, 2)
    for bad in (np.zeros((4, 4), np.float32), np.zeros((4, 4, 5), np.uint8), np.zeros((4,), np.uint8), np.zeros((0, 4), np.uint8)):
        with pytest.raises(ValueError):
            RS.resample_ref(bad, 4, 4)
    with pytest.raises(ValueError):
        RS.resample_ref(np.zeros((4, 4), np.uint8), 0, 4)
    RS.check_ratio(16, 16, 2, 128)
    for size in ((1, 16), (16, 129)):
        with pytest.raises(RS.ResampleRatio) as e:
            RS.check_ratio(16, 16, *size)
        assert '1/8 .. 8' in str(e.value)


def test_target_size():
    assert RS.target_size(100, 100, 4, Fraction('1.1')) == (110, 110)
    assert RS.target_size(100, 100, 4, '1.1') == (110, 110)
    assert RS.target_size(137, 9, 4, 3) == (411, 27)
    assert RS.target_size(101, 7, 4, Fraction('1.5')) == (152, 11)
    assert RS.target_size(101, 7, 4, Fraction(3, 2)) == (152, 11)
    assert RS.target_size(33, 44, 4, final_size=(50, 70)) == (70, 50)                # (W, H) in, (out_h, out_w) out; the aspect ratio may change
    assert RS.target_size(33, 44, 4) == (132, 176) and RS.target_size(33, 44, 2) == (66, 88)
    with pytest.raises(ValueError):
        RS.target_size(33, 44, 4, Fraction(3), (50, 70))
    for bad in (1.1, 0, Fraction(-1)):
        with pytest.raises(ValueError):
            RS.target_size(33, 44, 4, bad)
    with pytest.raises(ValueError):
        RS.target_size(33, 44, 4, final_size=(0, 70))


def test_parser(capsys):
    ap = inference.build_parser()
    a = ap.parse_args([])
    assert a.final_scale is None and a.final_size is None and a.out_scale == 4
    a = ap.parse_args(['--final-scale', '1.1'])
    assert a.final_scale == Fraction(11, 10) and a.final_size is None
    assert ap.parse_args(['--final-scale', '3/2']).final_scale == Fraction(3, 2) and ap.parse_args(['--final-scale', '3']).final_scale == 3
    a = ap.parse_args(['--final-size', '3840x2160'])
    assert a.final_size == (3840, 2160) and a.final_scale is None
    for bad in (['--final-scale', '3', '--final-size', '10x10'], ['--final-size', '10'], ['--final-size', '10x'], ['--final-size', '0x10'],
                ['--final-size', '10x10x3'], ['--final-size', 'axb'], ['--final-scale', 'x'], ['--final-scale', '0'], ['--final-scale', '-2']):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    capsys.readouterr()
    assert not [o for act in ap._actions for o in act.option_strings if 'outscale' in o.replace('_', '').replace('-', '') and o not in ('--out_scale',)]
    helps = {o: act.help for act in ap._actions for o in act.option_strings}
    assert 'NETWORK' in helps['--final-scale'] and '--out_scale' in helps['--final-scale']


def test_header_and_binding():
    assert '#include "femasr_hip_resample.h"' in open(os.path.join(ROOT, 'include', 'femasr_hip.h')).read()
    hdr = open(os.path.join(ROOT, 'include', 'femasr_hip_resample.h')).read()
    assert set(re.findall(r'^int\s+(femasr_[a-z0-9_]+)\s*\(', hdr, re.M)) == set(_lib.RESAMPLE_SIGNATURES) == {'femasr_resample_u8', 'femasr_resample_tile'}
    m = re.search(r'^int\s+femasr_resample_u8\s*\(([^;]*)\)\s*;', hdr, re.M | re.S)
    names = [a.strip().rsplit(' ', 1)[1].lstrip('*') for a in m.group(1).replace('\n', ' ').split(',')]
    assert names == ['stream', 'src', 'H', 'W', 'C', 'dst', 'out_h', 'out_w', 'w_h', 'idx_h', 'taps_h', 'w_w', 'idx_w', 'taps_w']
    assert len(_lib.RESAMPLE_SIGNATURES['femasr_resample_u8'][1]) == len(names)
    lib = _lib.load()
    assert lib.femasr_resample_tile() == RS.TILE and lib.femasr_version() == _lib.ABI_VERSION == 107
    from femasr_amd.csrc import build
    assert 'resample.hip' in build.SOURCES and '../../include/femasr_hip_resample.h' in build.HEADERS


def test_entry_refusals_need_no_gpu():
    """Everything femasr_resample_u8 refuses is refused before any launch - so also on a machine without a GPU."""
    import ctypes
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    call = lambda **kw: lib.femasr_resample_u8(*[kw.get(k, d) for k, d in (('stream', None), ('src', p), ('H', 8), ('W', 8), ('C', 3), ('dst', p), ('out_h', 8),
                                                                           ('out_w', 8), ('w_h', p), ('idx_h', p), ('taps_h', 4), ('w_w', p), ('idx_w', p), ('taps_w', 4))])
    for kw in (dict(C=0), dict(C=5), dict(src=None), dict(dst=None), dict(w_h=None), dict(idx_w=None), dict(H=0), dict(out_w=0), dict(taps_h=0),
               dict(taps_w=0), dict(taps_w=6000), dict(W=1 << 30, C=4), dict(out_w=(1 << 31) - 100)):
        assert call(**kw) == -1, kw                                                 # FEMASR_ERR_INVALID
        assert b'resample_u8' in lib.femasr_last_error()

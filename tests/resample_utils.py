"""Guarded wrapper of the entry point of include/femasr_hip_resample.h, in the manner of tests/encode_utils.py: every operand a region of
one guard arena (tests/guard_arena.py) at its exact size, the call made once per poison.  And the small images both resample test files use."""
import numpy as np
import torch

import guard_arena as GA
import gpu_utils as G
from femasr_amd import _lib
from femasr_amd.models.femasr_model import imresize_tables


def step_image():
    """16x16, 0 left of the middle and 255 right of it: the bicubic over- and undershoots at the edge."""
    img = np.zeros((16, 16), np.uint8)
    img[:, 8:] = 255
    return img


TIE_SEED = 8        # the centre of the 3x3 result is the mean of the four pixels: 151.5 in channel 0 (up to 152), 120.5 in channel 1 (down to 120)


def tie_image():
    return np.random.default_rng(TIE_SEED).integers(0, 256, (2, 2, 2), dtype=np.uint8)


def resample_entry(img, out_h, out_w, tables=None):
    """uint8 (H,W,C) array -> (out_h,out_w,C) array through femasr_resample_u8 under both poisons (guard_arena.run_twice): the image, the four
    tables and the output are regions of one arena, no byte outside the output may change and the output may not depend on the poison.
    tables: (w_h, idx_h, w_w, idx_w) of the caller's own in place of imresize_tables'."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w, c = img.shape
    wh, ih, ww, iw = tables or (imresize_tables(h, out_h, out_h / h, True) + imresize_tables(w, out_w, out_w / w, True))
    wh, ww = np.ascontiguousarray(wh, np.float64), np.ascontiguousarray(ww, np.float64)
    ih, iw = np.ascontiguousarray(ih, np.int32), np.ascontiguousarray(iw, np.int32)
    assert wh.shape == ih.shape == (out_h, wh.shape[1]) and ww.shape == iw.shape == (out_w, ww.shape[1])
    what = f'resample_u8 {h}x{w}x{c} -> {out_h}x{out_w}'

    def go():
        ops = G.Operands(what).inp('img', img).inp('wh', wh).inp('ih', ih).inp('ww', ww).inp('iw', iw).out('dst', out_h * out_w * c).build()
        _lib.check(_lib.load().femasr_resample_u8(None, ops.p('img'), h, w, c, ops.p('dst'), out_h, out_w, ops.p('wh'), ops.p('ih'), wh.shape[1],
                                                  ops.p('ww'), ops.p('iw'), ww.shape[1]))
        ops.check()
        return ops.get('dst', torch.uint8, (out_h, out_w, c)).cpu().numpy()
    return GA.run_twice(go, what)

"""Guarded wrappers of the entry points of include/femasr_hip_dists.h, in the manner of tests/gpu_utils.py: every operand a region of one
guard arena (tests/guard_arena.py), the workspaces at the size the library's own query gives."""
import numpy as np
import torch

import gpu_utils as G
from femasr_amd import _lib
from femasr_amd import dists as D


def l2pool(f_nhwc):
    """float32 (B2,H,W,C) numpy -> (B2,ceil(H/2),ceil(W/2),C) numpy through femasr_dists_l2pool."""
    f = np.ascontiguousarray(f_nhwc, np.float32)
    b2, h, w, c = f.shape
    hp, wp = (h + 1) // 2, (w + 1) // 2
    ops = G.Operands(f'dists_l2pool {f.shape}').inp('f', f).out('out', 4 * b2 * hp * wp * c).build()
    _lib.check(_lib.load().femasr_dists_l2pool(None, ops.p('f'), b2, h, w, c, ops.p('out')))
    ops.check()
    return ops.get('out', torch.float32, (b2, hp, wp, c)).cpu().numpy()


def moments(f_nhwc):
    """float32 (2B,H,W,C) numpy (pair b = images b, b + B) -> sums (B,5,C) float64 numpy through femasr_dists_moments."""
    f = np.ascontiguousarray(f_nhwc, np.float32)
    b2, h, w, c = f.shape
    b = b2 // 2
    ops = G.Operands(f'dists_moments {f.shape}').inp('f', f).out('sums', 8 * b * 5 * c)
    ops.scratch('ws', G.qp('femasr_dists_moments_workspace_bytes', b, h, w, c)).build()
    _lib.check(_lib.load().femasr_dists_moments(None, ops.p('f'), b, h, w, c, ops.p('ws'), ops.r['ws'].nbytes, ops.p('sums')))
    ops.check()
    return ops.get('sums', torch.float64, (b, 5, c)).cpu().numpy()


def moments_input(x_nchw, y_nchw):
    """float32 (B,3,H,W) numpy pair -> sums (B,5,3) float64 numpy through femasr_dists_moments_input."""
    x, y = np.ascontiguousarray(x_nchw, np.float32), np.ascontiguousarray(y_nchw, np.float32)
    b, _, h, w = x.shape
    ops = G.Operands(f'dists_moments_input {x.shape}').inp('x', x).inp('y', y).out('sums', 8 * b * 5 * 3)
    ops.scratch('ws', G.qp('femasr_dists_moments_workspace_bytes', b, h, w, 3)).build()
    _lib.check(_lib.load().femasr_dists_moments_input(None, ops.p('x'), ops.p('y'), b, h, w, ops.p('ws'), ops.r['ws'].nbytes, ops.p('sums')))
    ops.check()
    return ops.get('sums', torch.float64, (b, 5, 3)).cpu().numpy()


def forward(module, x, y):
    """femasr_dists_forward of a DISTS module on float32 (B,3,H,W) tensors between guard bands, with an exact-size workspace.
    Returns (scores (B,), terms (B,6,2)) numpy."""
    lib, h = module._native(x.device)
    b, _, hh, ww = x.shape
    ops = G.Operands(f'dists_forward {tuple(x.shape)}', x.device).inp('x', x.contiguous()).inp('y', y.contiguous())
    ops.out('scores', 8 * b).out('terms', 8 * b * 12).scratch('ws', G.qp('femasr_dists_workspace_bytes', h, b, hh, ww)).build()
    _lib.check(lib.femasr_dists_forward(h, None, ops.p('x'), ops.p('y'), b, hh, ww, ops.p('ws'), ops.r['ws'].nbytes, ops.p('scores'),
                                        ops.p('terms')))
    ops.check()
    return ops.get('scores', torch.float64).cpu().numpy(), ops.get('terms', torch.float64, (b, 6, 2)).cpu().numpy()


def features(module, x, y):
    """The five stage maps of femasr_dists_features: [(2B,h_k,w_k,C_k) float32 numpy], x in images 0..B-1, y in B..2B-1."""
    lib, h = module._native(x.device)
    b, _, hh, ww = x.shape
    shapes = D.map_shapes(hh, ww)[1:]
    ops = G.Operands(f'dists_features {tuple(x.shape)}', x.device).inp('x', x.contiguous()).inp('y', y.contiguous())
    ops.out('features', 4 * sum(2 * b * a * c * d for a, c, d in shapes))
    ops.scratch('ws', G.qp('femasr_dists_workspace_bytes', h, b, hh, ww)).build()
    _lib.check(lib.femasr_dists_features(h, None, ops.p('x'), ops.p('y'), b, hh, ww, ops.p('ws'), ops.r['ws'].nbytes, ops.p('features')))
    ops.check()
    flat, maps, off = ops.get('features', torch.float32).cpu().numpy(), [], 0
    for a, c, d in shapes:
        n = 2 * b * a * c * d
        maps.append(flat[off:off + n].reshape(2 * b, a, c, d))
        off += n
    return maps

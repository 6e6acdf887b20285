"""Guarded wrappers of the entry points of include/femasr_hip_encode.h, in the manner of tests/gpu_utils.py: every operand a region of one
guard arena (tests/guard_arena.py) at the size the library's own query gives."""
import ctypes

import numpy as np
import torch

import gpu_utils as G
from femasr_amd import _lib


def index_histogram(indices, n_e, offset8=False):
    """int64 (G, M) array -> (counts (G, n_e), invalid (G,)) numpy through femasr_index_histogram, every operand at its exact size.
    offset8: the indices start 8 bytes into their region - a base on 8 but not on 16 bytes (regions start on 256)."""
    idx = np.ascontiguousarray(indices, np.int64)
    g, m = idx.shape
    data = np.concatenate((np.full(1, 7, np.int64), idx.reshape(-1))) if offset8 else idx
    ops = G.Operands(f'index_histogram G {g} M {m} n_e {n_e}{" +8" if offset8 else ""}').inp('idx', data)
    ops.out('counts', 8 * g * n_e).out('invalid', 8 * g).scratch('ws', G.qp('femasr_index_histogram_workspace_bytes', g, m, n_e)).build()
    src = ctypes.c_void_p(ops.addr('idx') + (8 if offset8 else 0))
    _lib.check(_lib.load().femasr_index_histogram(None, src, g, m, n_e, ops.p('counts'), ops.p('invalid'), ops.p('ws'), ops.r['ws'].nbytes))
    ops.check()
    return ops.get('counts', torch.int64, (g, n_e)).cpu().numpy(), ops.get('invalid', torch.int64).cpu().numpy()


def encode(net, x, pad_mode, bgr=False, ws_short=0):
    """femasr_encode of a built FeMaSRNet on x (fp32 (B,3,H,W) or uint8 (B,H,W,3) tensor) between guard bands, with the workspace
    femasr_encode_workspace_bytes asks for less `ws_short` bytes.  Returns (rc, [index maps (B,1,qh,qw)] as numpy)."""
    from femasr_amd.archs.femasr_arch import _FP32, _U8
    u8 = x.dtype == torch.uint8
    fmt = _U8 if u8 else _FP32
    lib, h = net._native(x.device)
    b, _, hh, ww = fmt.bchw(x)
    _, qhw = net._geometry(lib, h, fmt, b, hh, ww, pad_mode)
    ops = G.Operands(f'encode {tuple(x.shape)} pad {pad_mode}', x.device).inp('x', x.contiguous())
    ops.out('indices', 8 * sum(b * a * c for a, c in qhw))
    ops.scratch('ws', G.qp('femasr_encode_workspace_bytes', h, b, hh, ww, pad_mode) - ws_short).build()
    rc = lib.femasr_encode(h, None, ops.p('x'), int(u8), int(bgr), b, hh, ww, pad_mode, ops.p('indices'), ops.p('ws'), ops.r['ws'].nbytes)
    ops.check()
    flat, maps, off = ops.get('indices', torch.int64).cpu().numpy(), [], 0
    for qh, qw in qhw:
        maps.append(flat[off:off + b * qh * qw].reshape(b, 1, qh, qw))
        off += b * qh * qw
    return rc, maps

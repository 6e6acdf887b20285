"""FeMaSRNet on MI355X: the reference's module surface over libfemasr_hip.so.

Drop-in for basicsr/archs/femasr_arch.py:214-479 on the INFERENCE path:
same class name, registered in ARCH_REGISTRY the same way, same keyword-only
constructor (femasr_arch.py:216-228), same methods (`test`, `test_tile`,
`forward`, `encode_and_decode`, `decode_indices`), same public attributes and
the same state-dict keys/shapes, so `load_state_dict(torch.load(p)['params'],
strict=False)` (inference_femasr.py:40) works on released checkpoints.

The torch sub-modules below are PARAMETER HOLDERS only: they give the state
dict its names, shapes and default initialisation.  No torch op computes
anything on the path — every forward goes through the C ABI
(include/femasr_hip.h) into the HIP kernels, and raises if the extension or a
GPU is missing (no CPU / eager fallback).
"""
import ctypes
import functools
import inspect
import math
from typing import Callable, NamedTuple

import numpy as np
import torch
from torch import nn

from .. import _lib
from .. import tiling
from ..registry import ARCH_REGISTRY

_CHANNELS = {8: 256, 16: 256, 32: 256, 64: 256, 128: 128, 256: 64, 512: 32}   # femasr_arch.py:244-252


# --------------------------------------------------------------------------- parameter holders
class _Holder(nn.Module):
    def forward(self, *a, **k):  # pragma: no cover - never used on the product path
        raise RuntimeError('parameter holder: computation happens in libfemasr_hip.so')


def _seq(*mods):
    """Numbered children like nn.Sequential, without its forward."""
    h = _Holder()
    for i, m in enumerate(mods):
        if m is not None:
            h.add_module(str(i), m)
    return h


def _norm(c):               # fema_utils.py:5-29 NormLayer('gn') -> .norm = GroupNorm(32, c, eps=1e-6)
    h = _Holder()
    h.norm = nn.GroupNorm(32, c, eps=1e-6, affine=True)
    return h


def _resblock(c):           # fema_utils.py:65-84: conv = Sequential(norm, act, conv, norm, act, conv)
    h = _Holder()
    h.conv = _seq(_norm(c), None, nn.Conv2d(c, c, 3, 1, 1), _norm(c), None, nn.Conv2d(c, c, 3, 1, 1))
    return h


def _swin_block(dim, heads, ws, shift, res=(32, 32)):   # network_swinir.py:164-237
    h = _Holder()
    h.norm1 = nn.LayerNorm(dim)
    attn = _Holder()
    attn.relative_position_bias_table = nn.Parameter(torch.zeros((2 * ws - 1) * (2 * ws - 1), heads))
    nn.init.trunc_normal_(attn.relative_position_bias_table, std=.02)
    ys, xs = np.divmod(np.arange(ws * ws), ws)
    rel = (ys[:, None] - ys[None, :] + ws - 1) * (2 * ws - 1) + (xs[:, None] - xs[None, :] + ws - 1)
    attn.register_buffer('relative_position_index', torch.from_numpy(rel.astype(np.int64)))
    attn.qkv = nn.Linear(dim, dim * 3)
    attn.proj = nn.Linear(dim, dim)
    h.attn = attn
    h.norm2 = nn.LayerNorm(dim)
    mlp = _Holder()
    mlp.fc1 = nn.Linear(dim, dim * 4)
    mlp.fc2 = nn.Linear(dim * 4, dim)
    h.mlp = mlp
    if shift > 0:           # persistent buffer in checkpoints (16x64x64 for the (32,32) construction size)
        hh, ww = res
        lab = np.zeros((hh, ww), np.float32)
        sl = (slice(0, -ws), slice(-ws, -shift), slice(-shift, None))
        cnt = 0
        for a in sl:
            for b in sl:
                lab[a, b] = cnt
                cnt += 1
        win = lab.reshape(hh // ws, ws, ww // ws, ws).transpose(0, 2, 1, 3).reshape(-1, ws * ws)
        diff = win[:, None, :] - win[:, :, None]
        h.register_buffer('attn_mask', torch.from_numpy(np.where(diff != 0, -100.0, 0.0).astype(np.float32)))
    else:
        h.register_buffer('attn_mask', None)
    return h


def _rstb(dim=256, depth=6, heads=8, ws=8):             # network_swinir.py:419-482
    h = _Holder()
    grp = _Holder()
    grp.blocks = _seq(*[_swin_block(dim, heads, ws, 0 if i % 2 == 0 else ws // 2) for i in range(depth)])
    h.residual_group = grp
    h.conv = nn.Conv2d(dim, dim, 3, 1, 1)
    return h


def _up_block(cin, cout):   # Upsample, Conv, ResBlock, ResBlock  (femasr_arch.py:171-176, 201-206)
    return _seq(None, nn.Conv2d(cin, cout, 3, 1, 1), _resblock(cout), _resblock(cout))


# --------------------------------------------------------------------------- tile formats
class _TileFormat(NamedTuple):
    """Everything that differs between the two image formats the tiled path runs in; the schedule (`FeMaSRNet._tiled`), the
    extract / paste helpers and the native forward call are written once against it.  Tensor shapes: tiling.tile_shape(dtype, ...)."""
    dtype: torch.dtype
    bchw: Callable          # tensor -> (batch, channel, height, width)
    window: Callable        # (tensor, y0, y1, x0, x1) -> the view [y0:y1, x0:x1] of every image (host tensors)
    native_bc: Callable     # (batch, channel) -> how the native tile calls take them (the uint8 kernels are RGB only)
    extract: str            # native symbols
    paste: str
    blend: str              # the opt-in overlap-blend paste (test_tile(..., blend=True))
    forward: str


_FP32 = _TileFormat(torch.float32, lambda t: tuple(t.shape), lambda t, y0, y1, x0, x1: t[:, :, y0:y1, x0:x1], lambda b, c: (b, c),
                    'femasr_extract_tiles', 'femasr_paste_tiles', 'femasr_blend_tiles', 'femasr_forward')                 # (B, C, H, W): test / test_tile
_U8 = _TileFormat(torch.uint8, lambda t: (t.shape[0], t.shape[3], t.shape[1], t.shape[2]), lambda t, y0, y1, x0, x1: t[:, y0:y1, x0:x1, :],
                  lambda b, c: (b,), 'femasr_extract_tiles_u8', 'femasr_paste_tiles_u8', 'femasr_blend_tiles_u8', 'femasr_forward_u8')   # (B, H, W, 3): test_u8 / test_tile_u8


def _takes_out(fn):
    """False when `fn` (`test` / `test_u8`, possibly replaced by a stand-in: the CPU-side tests of the host logic) has no `out=`."""
    try:
        return 'out' in inspect.signature(fn).parameters
    except (TypeError, ValueError):
        return False


# --------------------------------------------------------------------------- the arch
@ARCH_REGISTRY.register()
class FeMaSRNet(nn.Module):
    def __init__(self, *, in_channel=3, codebook_params=None, gt_resolution=256, LQ_stage=False,
                 norm_type='gn', act_type='silu', use_quantize=True, scale_factor=4,
                 use_semantic_loss=False, use_residual=True, **ignore_kwargs):
        super().__init__()
        codebook_params = np.array(codebook_params)
        if codebook_params.ndim != 2 or codebook_params.shape[1] != 3 or not 1 <= codebook_params.shape[0] <= _lib.MAX_CODEBOOKS:
            raise ValueError(f'codebook_params must be rows of [scale, n_e, e_dim] (1..{_lib.MAX_CODEBOOKS} rows)')
        if norm_type != 'gn' or act_type != 'silu':
            raise NotImplementedError("MI355X path builds norm_type='gn', act_type='silu' (the published configs)")
        self.codebook_scale = codebook_params[:, 0]
        codebook_emb_num = codebook_params[:, 1].astype(int)
        codebook_emb_dim = codebook_params[:, 2].astype(int)
        self.use_quantize = use_quantize
        self.in_channel = in_channel
        self.gt_res = gt_resolution
        self.LQ_stage = LQ_stage
        self.scale_factor = scale_factor if LQ_stage else 1
        self.use_residual = use_residual
        # accepted for signature compatibility; the VGG branch is training-only and is forced off
        # inside test() by the reference as well (femasr_arch.py:451-452)
        self.use_semantic_loss = False
        self.max_depth = int(np.log2(gt_resolution // self.codebook_scale[0]))
        encode_depth = int(np.log2(gt_resolution // self.scale_factor // self.codebook_scale[0]))
        self._encode_depth = encode_depth

        # ---- parameter tree (names == reference state-dict keys)
        enc = _Holder()
        res = gt_resolution // self.scale_factor
        enc.in_conv = nn.Conv2d(in_channel, _CHANNELS[res], 4, padding=1)
        blocks = []
        for _ in range(encode_depth):
            ci, co = _CHANNELS[res], _CHANNELS[res // 2]
            blocks.append(_seq(nn.Conv2d(ci, co, 3, stride=2, padding=1), _resblock(co), _resblock(co)))
            res //= 2
        if LQ_stage:
            swin = _Holder()
            swin.swin_blks = _seq(*[_rstb() for _ in range(4)])
            blocks.append(swin)
            for _ in range(2):
                blocks.append(_up_block(_CHANNELS[res], _CHANNELS[res * 2]))
                res *= 2
        enc.blocks = _seq(*blocks)
        self.multiscale_encoder = enc

        dec = []
        out_ch = None
        for i in range(self.max_depth):
            r = gt_resolution // 2 ** self.max_depth * 2 ** i
            blk = _Holder()
            blk.block = _up_block(_CHANNELS[r], _CHANNELS[r * 2])
            dec.append(blk)
            out_ch = _CHANNELS[r * 2]
        self.decoder_group = _seq(*dec)
        self.out_conv = nn.Conv2d(out_ch, 3, 3, 1, 1)

        # multi-scale vector quantisers (femasr_arch.py:277-300)
        quant, before, after = [], [], []
        for k in range(codebook_params.shape[0]):
            n_e, e_dim = int(codebook_emb_num[k]), int(codebook_emb_dim[k])
            q = _Holder()
            q.embedding = nn.Embedding(n_e, e_dim)
            q.embedding.weight.data.uniform_(-1.0 / n_e, 1.0 / n_e)       # femasr_arch.py:33
            quant.append(q)
            qc = _CHANNELS[int(self.codebook_scale[k])]
            before.append(nn.Conv2d(qc if k == 0 else 2 * qc, e_dim, 1))
            aq = _Holder()                                              # CombineQuantBlock (fema_utils.py:87-99)
            aq.conv = nn.Conv2d(e_dim if k == 0 else int(codebook_emb_dim[k - 1]) + e_dim, qc, 3, 1, 1)
            after.append(aq)
        self.quantize_group = _seq(*quant)
        self.before_quant_group = _seq(*before)
        self.after_quant_group = _seq(*after)
        self._cb = [(int(s_), int(n), int(d)) for s_, n, d in zip(self.codebook_scale, codebook_emb_num, codebook_emb_dim)]

        for p in self.parameters():
            p.requires_grad_(False)
        self._handle = None
        self._handle_device = None
        self._pushed = {}
        self._weights_dirty = True      # set by load_state_dict / .to() / invalidate_weights(): re-scan the state dict
        self._ws = None
        self.max_tile_batch = 16        # tiles per batched test() call inside test_tile
        self.num_streams = 1            # sub-batch streams inside one forward (femasr_set_streams)
        self._streams_set = None
        # 'fp32' (default): every layer fp32; the convs BEHIND the codebook lookup in the Winograd F(4x4,3x3) form, the SiLU of
        #   their GroupNorm prologue on the hardware exp2 / rcp units (image within ~1e-5 of the oracle, VQ indices bit-exact)
        # 'fp32_strict': the same with the IEEE-exact SiLU - bit-identical to the oracle (OracleNet())
        # 'fp32_direct': every conv in the direct form - bit-identical to OracleNet(winograd=False)
        # 'bf16x3': the convs behind the lookup on the bf16 matrix cores with a 3-term hi/lo split (within the 1e-3 bound)
        # 'fp16': the same convs on the fp16 matrix cores in ONE pass - the fast mode.  VQ indices identical to every other mode; the image
        #   is half-precision grade (about 5e-4 of its range from the fp32 image), NOT within the 1e-3 bound of the modes above
        self.decoder_math = ignore_kwargs.get('decoder_math', 'fp32')       # (an extension key of this build in `network_g`)
        self._check_decoder_math()
        # arithmetic of the 1x1 convs / nn.Linear layers (Swin qkv / proj / fc1 / fc2, before_quant):
        # 'bf16_split' (default): fp32-grade product on the bf16 matrix pipe - operands split exactly into three bf16 terms, six partial
        #   products, fp32 accumulation; ~3x closer to fp64 than the fp32 chain, bit-identical to OracleNet() (csrc/kernels_gemm_bf16.hip)
        # 'fp32': one fp32 fmaf chain per output on the fp32 MFMA - bit-identical to OracleNet(linear_math='fp32')
        # 'fp16' (opt-in): the same layers - and the stride-1 3x3 convs in front of the lookup - in ONE fp16 pass: input and weight rounded once to
        #   fp16, fp32 accumulation (csrc/kernels_gemm_f16.hip, kernels_conv_f16.hip).  The first mode in which VQ indices may DIFFER from the
        #   other modes: a token whose two nearest codes are nearly tied can flip (0 - 2 % of the tokens on the test cases), the image changes by
        #   up to ~0.1 of unit range where one does and is NOT within the 1e-3 bound anywhere.  Deterministic and bit-identical across
        #   batch size, streams, graph replay and tiling within the mode.  With decoder_math='fp16' the whole network is half-precision grade
        self.linear_math = ignore_kwargs.get('linear_math', 'bf16_split')
        self._check_linear_math()
        # True: each (shape, mode) class is captured once into a hipGraph (torch.cuda.CUDAGraph around femasr_forward, which
        # is capture-safe: no allocation / synchronisation inside) and replayed; inputs are copied into the graph's static
        # buffer and the outputs are copies of its static outputs.  Only pays when the ~330 launches are host-bound (tiny
        # batches); results are bit-identical (images and every index map: tests/test_gpu_graph_streams.py).  A cached graph
        # stays valid across weight changes (the handle repacks into the SAME allocations, see _release) and is dropped by
        # invalidate_weights(), by a new native handle and by the cache bound in _run.  Not with enable_profile(True): _run refuses.
        self.use_graph = False
        self._graphs = {}
        self._profile_on = False        # what enable_profile() last set on the live handle (a new handle starts with it off)
        # levels of the opt-in wavelet colour fix (`color_fix=True` on test / test_u8 / test_tile / test_tile_u8; femasr_amd/colorfix.py,
        # DESIGN.md 16): the blur that separates "coarse" (taken from the upsampled input) from "detail" (the network's) reaches 2^levels - 1
        # pixels to either side
        self.color_fix_levels = 5
        self.debug_wino_limits = None   # tests only: (log2_total, log2_image) for this net's planner (include/femasr_hip_debug.h)

    DECODER_MATH = {'fp32': 0, 'bf16x3': 1, 'fp32_direct': 2, 'fp32_strict': 3, 'fp16': 4}      # femasr_set_decoder_math: the FEMASR_DECODER_MATH_* values of include/femasr_hip.h

    def _check_decoder_math(self):
        if self.decoder_math not in self.DECODER_MATH:
            raise ValueError(f"decoder_math must be 'fp32', 'fp32_strict', 'fp32_direct', 'bf16x3' or 'fp16', got {self.decoder_math!r}")

    LINEAR_MATH = {'fp32': 0, 'bf16_split': 1, 'fp16': 2}      # femasr_set_linear_math: the FEMASR_LINEAR_MATH_* values of include/femasr_hip.h

    def _check_linear_math(self):
        if self.linear_math not in self.LINEAR_MATH:
            raise ValueError(f"linear_math must be 'bf16_split', 'fp32' or 'fp16', got {self.linear_math!r}")

    # ------------------------------------------------------------------ weight change tracking
    # The native handle holds REPACKED COPIES of the weights.  Changes made through the nn.Module API are seen
    # (load_state_dict, .to()/.cuda()/.float(), any in-place op on a parameter, which bumps its version counter);
    # writes through `.data` (p.data.copy_(...)) are invisible to torch's version counter: call invalidate_weights().
    def invalidate_weights(self):
        """Force every weight to be re-pushed to the native handle on the next forward."""
        self._pushed = {}
        self._weights_dirty = True
        self._graphs = {}

    def _load_from_state_dict(self, *args, **kwargs):
        self._weights_dirty = True
        return super()._load_from_state_dict(*args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self._weights_dirty = True
        return super().load_state_dict(*args, **kwargs)

    def _apply(self, fn, *args, **kwargs):
        self._weights_dirty = True
        return super()._apply(fn, *args, **kwargs)

    # ------------------------------------------------------------------ native handle
    def _native(self, device):
        """Create / refresh the C handle and push any changed weights."""
        if device.type != 'cuda':
            raise _lib.FemasrError('FeMaSRNet (MI355X build) runs on a GPU device only; move the module and '
                                   'inputs to cuda. There is no CPU fallback.')
        lib = _lib.load()
        dev_index = device.index if device.index is not None else torch.cuda.current_device()
        if self._handle is None or self._handle_device != dev_index:
            self._release()
            cfg = _lib.Config()
            cfg.in_channel, cfg.gt_resolution, cfg.lq_stage = self.in_channel, self.gt_res, int(self.LQ_stage)
            cfg.scale_factor, cfg.use_quantize, cfg.use_residual = int(self.scale_factor), int(self.use_quantize), int(self.use_residual)
            cfg.n_codebooks = len(self._cb)
            for k, (sc, n_e, e_dim) in enumerate(self._cb):
                cfg.codebook_scale[k], cfg.n_e[k], cfg.e_dim[k] = sc, n_e, e_dim
            cfg.device = dev_index
            h = ctypes.c_void_p()
            _lib.check(lib.femasr_create(ctypes.byref(cfg), ctypes.byref(h)))
            self._handle, self._handle_device, self._pushed = h, dev_index, {}
            self._weights_dirty = True
            self._profile_on = False
        # the walk over the (~480-tensor) state dict only runs when something may have changed; otherwise a cheap scan of
        # the parameters' version counters (in-place updates) decides
        if not self._weights_dirty:
            self._weights_dirty = self._param_stamp() != self._version_sum
        if self._weights_dirty:
            dirty = False
            for key, t in self.state_dict().items():
                if key.endswith('relative_position_index') or key.endswith('attn_mask'):
                    continue
                if t.device.type != 'cuda':
                    raise _lib.FemasrError(f'parameter {key} is on {t.device}; call .to("cuda") on the module')
                stamp = (t.data_ptr(), t._version)
                if self._pushed.get(key) == stamp:
                    continue
                if not dirty:
                    torch.cuda.synchronize(device)
                    dirty = True
                src = t.detach().to(torch.float32).contiguous()
                shape = (ctypes.c_int64 * src.dim())(*src.shape)
                _lib.check(lib.femasr_set_weight(self._handle, key.encode(), _lib.ptr(src), shape, src.dim()))
                self._pushed[key] = stamp
            if dirty:
                _lib.check(lib.femasr_finalize_weights(self._handle))
            self._version_sum = self._param_stamp()
            self._weights_dirty = False
        if self._streams_set != (self._handle.value, self.num_streams, self.decoder_math, self.linear_math, self.debug_wino_limits):
            self._check_decoder_math()
            self._check_linear_math()
            _lib.check(lib.femasr_set_linear_math(self._handle, self.LINEAR_MATH[self.linear_math]))
            _lib.check(lib.femasr_set_streams(self._handle, int(self.num_streams)))
            _lib.check(lib.femasr_set_decoder_math(self._handle, self.DECODER_MATH[self.decoder_math]))
            lim = (0, 0) if self.debug_wino_limits is None else self.debug_wino_limits      # (0, 0): the handle's defaults again
            _lib.check(lib.femasr_debug_set_wino_limits(self._handle, int(lim[0]), int(lim[1])))
            self._streams_set = (self._handle.value, self.num_streams, self.decoder_math, self.linear_math, self.debug_wino_limits)
        return lib, self._handle

    def _param_stamp(self):
        """Cheap change detector over the parameters: in-place updates bump `_version`; a replaced Parameter object or rebound
        storage (`mod.weight = nn.Parameter(t)`, `p.data = t`, `p.set_()`) changes `data_ptr()`.  Writes through `.data` views
        stay invisible to both: FeMaSRNet.invalidate_weights()."""
        acc = 0
        for p_ in self.parameters():
            acc = (acc * 1000003 + p_._version * 7919 + p_.data_ptr()) & 0xFFFFFFFFFFFFFFFF
        return acc

    def _release(self):
        if getattr(self, '_handle', None) is not None:
            # Captured graphs bake pointers into the handle's repacked weights: drop them with it.  They are NOT dropped when
            # weights change (load_state_dict, .to(), in-place updates): femasr_set_weight / femasr_finalize_weights repack into
            # the allocations made at the first push - repacked weight buffers are never reallocated while a handle lives - so a
            # replay reads the new weights.  tests/test_gpu_graph_streams.py::test_weights_changed_under_a_live_graph holds that
            # invariant: a launcher that frees and reallocates has to clear `_graphs` wherever `_weights_dirty` leads to a push.
            self._graphs = {}
            _lib.load().femasr_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _workspace(self, query, h, dims, device):
        """The scratch tensor of the native calls, at least as large as `query(h, *dims, &bytes)` asks for (grown, never shrunk)."""
        nbytes = ctypes.c_size_t()
        _lib.check(query(h, *dims, ctypes.byref(nbytes)))
        if self._ws is None or self._ws.numel() < nbytes.value or self._ws.device != device:
            self._ws = None
            self._ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=device)
        return self._ws

    @staticmethod
    def _stream(device):
        return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)

    def enable_profile(self, on=True):
        lib, h = self._native(next(self.parameters()).device)
        _lib.check(lib.femasr_profile_enable(h, int(on)))
        _lib.check(lib.femasr_profile_reset(h))
        self._profile_on = bool(on)

    def profile(self):
        """{kernel name: (ms, launches, flops, bytes)} since the last reset (HIP events on the launch stream)."""
        lib, h = self._native(next(self.parameters()).device)
        out = {}
        for s in range(lib.femasr_profile_slots(h)):
            ms, n, fl, by = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
            _lib.check(lib.femasr_profile_get(h, s, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl), ctypes.byref(by)))
            if n.value:
                out[lib.femasr_profile_name(h, s).decode()] = (ms.value, n.value, fl.value, by.value)
        return out

    # ------------------------------------------------------------------ the path
    def _forward_native(self, lib, h, fmt, x, pad_mode, out=None, flags=(), indices=True):
        """One `femasr_forward` / `femasr_forward_u8` (the format's) on the current stream: output geometry, workspace and result
        tensor (`out`, when given, is validated and written in place).  `flags`: the native arguments in front of `pad_mode`
        (`femasr_forward_u8`'s bgr).  Returns (out, all VQ indices as one flat tensor or None, workspace, [(qh, qw)] per codebook)."""
        b, _, hh, ww = fmt.bchw(x)
        shape, qhw = self._geometry(lib, h, fmt, b, hh, ww, pad_mode)
        ws = self._workspace(lib.femasr_workspace_bytes, h, (b, hh, ww, pad_mode), x.device)
        if out is None:
            out = torch.empty(shape, dtype=fmt.dtype, device=x.device)
        else:
            self._check_out(out, shape, fmt.dtype, x.device)
        idx_all = torch.empty((sum(b * a * c for a, c in qhw),), dtype=torch.int64, device=x.device) if indices else None
        _lib.check(getattr(lib, fmt.forward)(h, self._stream(x.device), _lib.ptr(x), b, hh, ww, *flags, pad_mode, _lib.ptr(out),
                                             None if idx_all is None else _lib.ptr(idx_all), _lib.ptr(ws), ws.numel()))
        return out, idx_all, ws, qhw

    @staticmethod
    def _geometry(lib, h, fmt, b, hh, ww, pad_mode):
        """(shape of the result tensor in the format's layout, [(qh, qw)] per codebook) of a forward on b images of hh x ww."""
        oh, ow, nq = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        qh, qw = (ctypes.c_int * _lib.MAX_CODEBOOKS)(), (ctypes.c_int * _lib.MAX_CODEBOOKS)()
        _lib.check(lib.femasr_forward_shapes(h, hh, ww, pad_mode, ctypes.byref(oh), ctypes.byref(ow), ctypes.byref(nq),
                                             ctypes.byref(qh), ctypes.byref(qw)))
        return tiling.tile_shape(fmt.dtype, b, 3, oh.value, ow.value), [(qh[k], qw[k]) for k in range(nq.value)]

    @staticmethod
    def _check_out(out, shape, dtype, device):
        if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != device or not out.is_contiguous():
            raise ValueError(f'out= must be a contiguous {dtype} tensor of shape {tuple(shape)} on {device}, got '
                             f'{tuple(out.shape)} {out.dtype} on {out.device}')

    def _run(self, x, pad_mode, out=None):
        if x.dim() != 4 or x.shape[1] != self.in_channel:
            raise ValueError(f'expected (B,{self.in_channel},H,W), got {tuple(x.shape)}')
        lib, h = self._native(x.device)
        x = x.detach().to(torch.float32).contiguous()
        b, _, hh, ww = x.shape
        if self.use_graph:
            if self._profile_on:
                # the profiler's event pairs would be recorded INTO the capture and never on a stream: profile() would then wait
                # on events that no replay ever signals.  Refused here, before anything is captured.
                raise _lib.FemasrError('use_graph = True cannot be combined with enable_profile(True): per-kernel events cannot be '
                                       'read back from a replayed hipGraph; call enable_profile(False) or set use_graph = False')
            if out is not None:                                                      # (as the eager call: refused before any launch or capture)
                self._check_out(out, self._geometry(lib, h, _FP32, b, hh, ww, pad_mode)[0], _FP32.dtype, x.device)
            key = (b, hh, ww, pad_mode, self.num_streams, self.decoder_math, self.linear_math, x.device.index)
            ent = self._graphs.get(key)
            if ent is None:
                if len(self._graphs) > 8:
                    self._graphs.clear()
                xs = x.clone()
                self._forward_native(lib, h, _FP32, xs, pad_mode)                    # warm-up: lazy one-time setup outside capture
                torch.cuda.synchronize(x.device)
                g = torch.cuda.CUDAGraph()
                self._ws = None                                                      # the graph owns its workspace
                with torch.cuda.graph(g):
                    so, si, sw, qhw = self._forward_native(lib, h, _FP32, xs, pad_mode)
                self._ws = None
                ent = self._graphs[key] = (g, xs, so, si, sw, qhw)
            g, xs, so, si, _, qhw = ent
            xs.copy_(x)
            g.replay()
            out, idx_all = (so.clone() if out is None else out.copy_(so)), si.clone()
        else:
            out, idx_all, _, qhw = self._forward_native(lib, h, _FP32, x, pad_mode, out)
        idx, off = [], 0
        for qh, qw in qhw:
            idx.append(idx_all[off:off + b * qh * qw].view(b, 1, qh, qw))
            off += b * qh * qw
        return out, idx

    @torch.no_grad()
    def test_u8(self, img_u8, bgr=False, out=None, color_fix=False, self_ensemble=False):
        """The CLI arithmetic of inference_femasr.py:50-67 on the device in ONE native call: uint8 (H,W,3) or (B,H,W,3) image(s) ->
        uint8 (sH,sW,3) / (B,sH,sW,3); decode (`/255.`) is fused into the forward's mirror-pad kernel and tensor2img (clamp, x255,
        round half to even) into its crop kernel (femasr_forward_u8) - the same bits as imgproc.u8_to_input -> test() ->
        imgproc.output_to_u8, without the two fp32 NCHW images in between.  `out`: a contiguous uint8 (B,sH,sW,3) tensor the crop
        kernel stores into (the tiled / multi-GPU callers pass slices of their result or all-gather send buffers).
        color_fix=True (NOT the reference's arithmetic, off by default): the wavelet colour fix of the result's BYTES against the input's
        (femasr_amd.colorfix.wavelet_color_fix, `color_fix_levels` levels), in place on the result.
        self_ensemble=True (NOT the reference's arithmetic, off by default): the x8 geometric self-ensemble (`_ensemble`) of the BYTES of
        eight `test_u8` results, S / 8 rounded half to even - deliberately not the quantised fp32 ensemble; a colour fix comes after it."""
        if img_u8.device.type != 'cuda':
            raise _lib.FemasrError('test_u8: tensor must be on the GPU (no CPU fallback)')
        x, single = self._u8_batch(img_u8)
        if self_ensemble:
            out = self._ensemble(_U8, functools.partial(self._test_u8, bgr=bgr), x, out)
        else:
            out = self._test_u8(x, bgr, out)
        if color_fix:
            self._color_fix(out, x)
        return out[0] if single else out

    def _test_u8(self, x, bgr=False, out=None):
        """The plain uint8 forward on a contiguous (B,H,W,3) batch."""
        lib, h = self._native(x.device)
        return self._forward_native(lib, h, _U8, x, 1, out, flags=(int(bool(bgr)),), indices=False)[0]

    def _test(self, x, out=None):
        """The plain fp32 forward with test()'s pad / crop geometry."""
        return self._run(x, 1, out)[0]

    def _ensemble(self, fmt, run, x, out=None):
        """The opt-in x8 geometric self-ensemble of `run` (the plain `test` / `test_u8`, `run(batch[, out=])`) on the contiguous image batch
        `x` in tile format `fmt`: expand -> forwards -> merge (femasr_amd/ensemble.py; ONE launch each on the GPU, the torch definition on
        host tensors - the CPU-side tests of the schedule).  The variants of one shape class ((H,W) and (W,H); ONE class of eight when
        H == W) run in calls of at most max(1, max_tile_batch // B) whole variants, each writing straight into its place of the result
        buffers; the result does not depend on that split (the forward is bitwise independent of the batch size).  The
        merge writes into `out` when one is given."""
        from .. import ensemble
        b = fmt.bchw(x)[0]
        xs, xt = ensemble.expand(x)
        ys, yt = ensemble.result_buffers(x, self.scale_factor)
        xa, ya = ensemble.as_batch(xs, xt), ensemble.as_batch(ys, yt)
        per = max(1, self.max_tile_batch // max(1, b))
        in_place = _takes_out(run)
        for src, dst in ([(xa, ya)] if xa is not None and ya is not None else [(xs, ys), (xt, yt)]):
            for i in range(0, src.shape[0], per):
                d = dst[i:i + per].flatten(0, 1)
                y = run(src[i:i + per].flatten(0, 1), out=d) if in_place else run(src[i:i + per].flatten(0, 1))
                if y.data_ptr() != d.data_ptr():
                    d.copy_(y)
        return ensemble.merge(ys, yt, out)

    def _color_fix(self, canvas, x):
        """The opt-in wavelet colour fix of a finished result against the whole input, in place (femasr_amd/colorfix.py)."""
        from ..colorfix import wavelet_color_fix
        return wavelet_color_fix(canvas, x, self.color_fix_levels, out=canvas)

    @staticmethod
    def _u8_batch(img_u8):
        """uint8 (H,W,3) or (B,H,W,3) -> (contiguous (B,H,W,3), whether the caller's image had no batch axis)."""
        single = img_u8.dim() == 3
        x = img_u8.unsqueeze(0) if single else img_u8
        if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3:
            raise ValueError(f'expected uint8 (H,W,3) or (B,H,W,3), got {img_u8.dtype} {tuple(img_u8.shape)}')
        return x.contiguous(), single

    @torch.no_grad()
    def encode_and_decode(self, input, gt_indices=None, current_iter=None):
        """`gt_indices` (one (B,1,h,w) index map per codebook) only changes the LOSS in the reference - VectorQuantizer.forward
        computes z_q and the returned indices from its own argmin either way (femasr_arch.py:64-66,69-91,95,339-342) - so an
        inference build serves the call and ignores it: image and indices are those of forward(input); the losses are zeros."""
        if gt_indices is not None:
            n_cb = len(self._cb)
            if not isinstance(gt_indices, (list, tuple)) or len(gt_indices) < n_cb:
                raise ValueError(f'gt_indices must hold one index map per codebook ({n_cb}), as FeMaSRNet.forward returns them')
        out, idx = self._run(input, 0)
        zero = out.new_zeros(())
        return out, zero, zero, idx

    @torch.no_grad()
    def forward(self, input, gt_indices=None):
        """(dec, codebook_loss, semantic_loss, [indices]) like femasr_arch.py:470-479 (losses are 0 in inference)."""
        return self.encode_and_decode(input, gt_indices)

    @torch.no_grad()
    def test(self, input, out=None, color_fix=False, self_ensemble=False):
        """femasr_arch.py:449-468: mirror-pad to (h//wsz+1)*wsz, run, crop to (h*s, w*s).  `out` (not in the reference): a
        contiguous float32 (B, 3, h*s, w*s) tensor the result is written INTO by the last kernel of the forward - the tiled /
        multi-GPU callers pass slices of their result or all-gather send buffers, so no copy follows.
        color_fix=True (not in the reference, off by default): the wavelet colour fix of the result against `input`
        (femasr_amd.colorfix.wavelet_color_fix, `color_fix_levels` levels), after the forward - outside the captured graph with
        `use_graph` - and in place on the result.
        self_ensemble=True (not in the reference, off by default): the x8 geometric self-ensemble (`_ensemble`, femasr_amd/ensemble.py,
        DESIGN.md 18): this forward on the eight flips / transposes of `input`, mapped back and averaged in a fixed fp32 order, at eight
        times the compute; a colour fix comes after it."""
        if self_ensemble:
            if input.dim() != 4 or input.shape[1] != self.in_channel:
                raise ValueError(f'expected (B,{self.in_channel},H,W), got {tuple(input.shape)}')
            y = self._ensemble(_FP32, self._test, input.detach().to(torch.float32).contiguous(), out)
        else:
            y = self._test(input, out)
        if color_fix:
            self._color_fix(y, input.detach().to(torch.float32).contiguous())
        return y

    @torch.no_grad()
    def test_with_indices(self, input):
        """(output, index map of the first codebook) through test()'s pad / crop geometry."""
        out, idx = self._run(input, 1)
        return out, idx[0]

    @torch.no_grad()
    def test_with_all_indices(self, input):
        return self._run(input, 1)

    @torch.no_grad()
    def decode_indices(self, indices):
        assert len(indices.shape) == 4, f'shape of indices must be (b, 1, h, w), but got {indices.shape}'
        dev = next(self.parameters()).device
        lib, h = self._native(dev)
        idx = indices.to(device=dev, dtype=torch.int64).contiguous()
        b, _, qh, qw = idx.shape
        ws = self._workspace(lib.femasr_decode_workspace_bytes, h, (b, qh, qw), dev)
        up = 2 ** self.max_depth
        out = torch.empty((b, 3, qh * up, qw * up), dtype=torch.float32, device=dev)
        _lib.check(lib.femasr_decode_indices(h, self._stream(dev), _lib.ptr(idx), b, qh, qw, _lib.ptr(out), _lib.ptr(ws), ws.numel()))
        return out

    # ------------------------------------------------------------------ the network as an encoder
    def _encode_native(self, x, in_u8, bgr, pad_mode):
        """One `femasr_encode` on the current stream: forward's launch schedule cut behind the last codebook lookup.
        `x`: contiguous fp32 (B,3,H,W) or uint8 (B,H,W,3).  Returns the index maps, views of one flat tensor."""
        fmt = _U8 if in_u8 else _FP32
        lib, h = self._native(x.device)
        b, _, hh, ww = fmt.bchw(x)
        _, qhw = self._geometry(lib, h, fmt, b, hh, ww, pad_mode)
        ws = self._workspace(lib.femasr_encode_workspace_bytes, h, (b, hh, ww, pad_mode), x.device)
        idx_all = torch.empty((sum(b * a * c for a, c in qhw),), dtype=torch.int64, device=x.device)
        _lib.check(lib.femasr_encode(h, self._stream(x.device), _lib.ptr(x), int(in_u8), int(bool(bgr)), b, hh, ww, pad_mode,
                                     _lib.ptr(idx_all), _lib.ptr(ws), ws.numel()))
        idx, off = [], 0
        for qh, qw in qhw:
            idx.append(idx_all[off:off + b * qh * qw].view(b, 1, qh, qw))
            off += b * qh * qw
        return idx

    @torch.no_grad()
    def encode_indices(self, input, pad=False):
        """Image batch -> the VQ index maps alone, one (B,1,qh,qw) int64 map per codebook: the network as an encoder (the frozen HQ net
        that makes `gt_indices`, basicsr/models/femasr_model.py:145-146; vis_codebook.py).  pad=False: `forward`'s geometry, the result
        equals `forward(input)[3]`; pad=True: `test()`'s mirror pad, the result equals `test_with_all_indices(input)[1]` - bit for bit:
        every launch in front of a lookup is the forward's, and nothing behind the last lookup runs (no after_quant conv, no decoder stage,
        no out_conv, no image; in LQ nets no encoder up-block that only feeds decoder skips).  `linear_math` and `num_streams` act as in the
        forward; `decoder_math` cannot change an index and, with one codebook, selects nothing that runs.  Always eager, also with
        `use_graph = True` (the call is short; it is capture-safe for a caller who captures it by hand: set `_ws = None` around the
        capture, as `_run` does, so that the graph owns its workspace)."""
        if input.dim() != 4 or input.shape[1] != self.in_channel:
            raise ValueError(f'expected (B,{self.in_channel},H,W), got {tuple(input.shape)}')
        if input.device.type != 'cuda':
            raise _lib.FemasrError('encode_indices: tensor must be on the GPU (no CPU fallback)')
        return self._encode_native(input.detach().to(torch.float32).contiguous(), False, False, int(bool(pad)))

    @torch.no_grad()
    def encode_indices_u8(self, img_u8, bgr=False, pad=True):
        """`encode_indices` on uint8 (H,W,3) or (B,H,W,3) image(s) on the GPU: the decode (`/255.`, bgr=True: cv2's channel order) is fused
        into the mirror-pad kernel as in `test_u8`, so the maps are those of `encode_indices(imgproc.u8_to_input(img), pad)`.  Eager."""
        if img_u8.device.type != 'cuda':
            raise _lib.FemasrError('encode_indices_u8: tensor must be on the GPU (no CPU fallback)')
        x, _ = self._u8_batch(img_u8)
        return self._encode_native(x, True, bgr, int(bool(pad)))

    # ------------------------------------------------------------------ tiled inference
    @torch.no_grad()
    def test_tile(self, input, tile_size=240, tile_pad=16, rank=0, world_size=1, gather=None, paste=True, blend=False, color_fix=False,
                  self_ensemble=False):
        """Reference semantics of femasr_arch.py:387-447 (overlap-discard paste onto a zero canvas), but
        tiles of one shape class run as batched `test()` calls, and with world_size > 1 each rank
        computes a contiguous share of every class; `gather(results, classes, batch, channel, scale) -> list per rank`
        supplies the collective (femasr_amd.distributed.TileExchange: ONE RCCL all-gather on persistent buffers the tiles were
        written into).  A gather that is passed is used at world_size == 1 too (one rank of a real collective); world_size > 1
        without one is a ValueError.  paste=False (ranks other than the one that needs the image): take part in the collective,
        skip the canvas (returns None).
        blend=True (NOT the reference's arithmetic, hence off by default): instead of discarding the halos, every canvas pixel is the
        weighted mean of the upscaled windows that contain it (linear ramps across the overlaps: tiling.blend_weight_1d)
        - no seams where neighbouring bodies meet.  The tiles, their batching and the collective are the same; only the last step
        differs (ONE femasr_blend_tiles launch instead of the per-class pastes).  Needs 2 * tile_pad <= tile_size (ValueError).
        color_fix=True (NOT the reference's arithmetic either, off by default): after the paste or the blend, on the pasting ranks, the
        wavelet colour fix of the WHOLE canvas against the WHOLE input (femasr_amd/colorfix.py): everything coarser than
        ~2^color_fix_levels pixels comes from the bicubically upsampled input, which knows nothing of tiles - the per-tile tone offsets
        that `blend` only turns into ramps go away.  Defined on canvas and input alone, so independent of the partition and the ranks.
        self_ensemble=True (NOT the reference's arithmetic, off by default): every tile is the x8 geometric self-ensemble of its crop
        (`test(crop, self_ensemble=True)`) - per TILE, so the tile grid, the partition, the gather payload, the paste, `blend`
        and `color_fix` are what they are without it; batched calls hold max_tile_batch // (8 * batch) tiles' worth of variants."""
        return self._tiled(input.contiguous().float(), _FP32, self.test, tile_size, tile_pad, rank, world_size, gather, paste, blend, color_fix,
                           self_ensemble)

    @torch.no_grad()
    def test_tile_u8(self, img_u8, tile_size=240, tile_pad=16, rank=0, world_size=1, gather=None, paste=True, bgr=False, blend=False,
                     color_fix=False, self_ensemble=False):
        """`test_tile` on uint8 images end to end (round 6; the CLI's tiled branch, inference_femasr.py:58-67 with femasr_arch.py:387-447):
        uint8 (H,W,3) / (B,H,W,3) in -> uint8 (sH,sW,3) / (B,sH,sW,3) out.  Tiles are cropped as uint8, every batched call is ONE
        `test_u8` (decode fused into the mirror-pad kernel, tensor2img into the crop kernel, which stores straight into the result /
        all-gather send buffer), the all-gather and the paste move one byte per value (a quarter of the fp32 path's xGMI and canvas
        traffic; no 805-MB fp32 canvas at 8192^2).  Bit-identical to output_to_u8(test_tile(u8_to_input(img))): tensor2img is
        element-wise and every output pixel comes from exactly one tile.
        blend=True: as in `test_tile`, on the BYTES the tiles hold after tensor2img (the all-gather payload stays one byte per value):
        the weighted mean of the covering windows' bytes, rounded half to even - not tensor2img of the fp32 blend.
        color_fix=True: as in `test_tile`, on the canvas BYTES against the input bytes (planes byte / 255, the result rounded half to even):
        no fp32 canvas is held, the fix works through the planes in groups of bounded size.
        self_ensemble=True: as in `test_tile`, every tile the ensemble of the BYTES of eight `test_u8` results (S / 8, half to even)."""
        x, single = self._u8_batch(img_u8)
        output = self._tiled(x, _U8, functools.partial(self.test_u8, bgr=bgr), tile_size, tile_pad, rank, world_size, gather, paste, blend,
                             color_fix, self_ensemble)
        return output[0] if single and output is not None else output

    def _tiled(self, x, fmt, run, tile_size, tile_pad, rank, world_size, gather, paste, blend=False, color_fix=False, self_ensemble=False):
        """The tile schedule of `test_tile` and `test_tile_u8`: `x` is the contiguous image batch in tile format `fmt`,
        `run(crops[, out=])` the batched call on the crops of one shape class.  Returns the canvas (None with paste=False).
        self_ensemble: `run` becomes its x8 ensemble form (`_ensemble`), on an eighth as many tiles per call."""
        if blend:
            tiling.check_blend(tile_size, tile_pad)             # before any work
        batch, channel, height, width = fmt.bchw(x)
        s = self.scale_factor
        classes = tiling.shape_classes(tiling.enumerate_tiles(height, width, tile_size, tile_pad))
        owned_all = tiling.assign(classes, world_size, s)          # (once per call: every rank's share - the paste below indexes it)
        mine = owned_all[rank]
        # `time_split = True`: record where the call's time goes (events on the current stream; read back in `last_split_ms`
        # = {'compute', 'gather', 'paste', 'tiles_owned'} after a synchronize) - bench.py --workload tile2048 reports it per rank
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if (getattr(self, 'time_split', False) and x.is_cuda) else None
        if ev:
            ev[0].record()
        # One result buffer per shape class, written in place by the batched calls (`out=`).  With a gather object that owns
        # persistent send buffers (femasr_amd.distributed.TileExchange.send_views) the buffers ARE this rank's all-gather send slab.
        # A gather that is passed is used, in a world of one as well (one rank of a real collective: the same slab, gather and paste).
        alloc = getattr(gather, 'send_views', None) if gather is not None else None
        if alloc is not None:
            results = alloc(classes, batch, channel, s, fmt.dtype, x.device)
        else:
            results = {hw: torch.empty(tiling.tile_shape(fmt.dtype, len(tl) * batch, channel, hw[0] * s, hw[1] * s), dtype=fmt.dtype,
                                       device=x.device) for hw, tl in mine.items()}
        per_call = max(1, self.max_tile_batch // batch)
        if self_ensemble:
            per_call = max(1, self.max_tile_batch // (8 * batch))
            run = functools.partial(self._ensemble, fmt, run)
        in_place = _takes_out(run)
        for hw, tl in mine.items():
            for i in range(0, len(tl), per_call):
                chunk = tl[i:i + per_call]
                dst = results[hw][i * batch:(i + len(chunk)) * batch]
                crops = self._extract_tiles(fmt, x, chunk, hw)
                y = run(crops, out=dst) if in_place else run(crops)
                if y.data_ptr() != dst.data_ptr():
                    dst.copy_(y)
        if ev:
            ev[1].record()
        if world_size > 1 and gather is None:
            raise ValueError('world_size > 1 needs a gather callable')
        if gather is not None:
            per_rank = gather(results, classes, batch, channel, s)
        else:
            per_rank = [results]
        if ev:
            ev[2].record()
        output = None
        if paste and blend:
            output = self._blend_tiles(fmt, x, per_rank, owned_all, batch, channel, height, width, tile_size, s)
        elif paste:
            output = x.new_zeros(tiling.tile_shape(fmt.dtype, batch, channel, height * s, width * s))
            for r, res in enumerate(per_rank):
                for hw, tl in owned_all[r].items():
                    if tl:
                        self._paste_tiles(fmt, output, res[hw], tl, batch, s)
        if color_fix and output is not None:
            self._color_fix(output, x)                  # (the one post-paste step: whole canvas against whole input; counted as 'paste')
        if ev:
            ev[3].record()
            self._split_events = (ev, sum(len(tl) for tl in mine.values()))
        return output

    @property
    def last_split_ms(self):
        """{'compute', 'gather', 'paste'} milliseconds of the last `test_tile` / `test_tile_u8` call made with `time_split = True`
        (synchronises)."""
        rec = getattr(self, '_split_events', None)
        if rec is None:
            return None
        ev, owned = rec
        ev[3].synchronize()
        return {'compute': round(ev[0].elapsed_time(ev[1]), 3), 'gather': round(ev[1].elapsed_time(ev[2]), 3),
                'paste': round(ev[2].elapsed_time(ev[3]), 3), 'tiles_owned': owned}

    @staticmethod
    def _extract_tiles(fmt, x, chunk, hw):
        """torch.cat of the reference's crops `input[:, :, y0p:y1p, x0p:x1p]` (femasr_arch.py:412-426; uint8: `img[:, y0p:y1p,
        x0p:x1p, :]`) for the tiles of one shape class, tile-major: one launch of the format's extract kernel on the GPU (host
        tensors: plain slicing, used by the CPU-side tests of the partition / gather logic only)."""
        if not x.is_cuda:
            return torch.cat([fmt.window(x, t.y0p, t.y1p, t.x0p, t.x1p) for t in chunk], 0)
        b, c, h, w = fmt.bchw(x)
        yx = torch.tensor([v for t in chunk for v in (t.y0p, t.x0p)], dtype=torch.int32).to(x.device, non_blocking=True)
        out = torch.empty(tiling.tile_shape(fmt.dtype, len(chunk) * b, c, hw[0], hw[1]), dtype=fmt.dtype, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(getattr(_lib.load(), fmt.extract)(torch.cuda.current_stream().cuda_stream, x.data_ptr(), *fmt.native_bc(b, c), h, w,
                                                         yx.data_ptr(), len(chunk), hw[0], hw[1], out.data_ptr()))
        return out

    @staticmethod
    def _paste_tiles(fmt, output, block, tl, batch, s):
        """`output[:, :, dst] = output_tile[:, :, src]` (femasr_arch.py:443-446) for all tiles of one shape class and rank."""
        if not output.is_cuda:
            for k, t in enumerate(tl):
                fmt.window(output, *t.out_dst(s))[...] = fmt.window(block[k * batch:(k + 1) * batch], *t.out_src(s))
            return
        block = block.contiguous().to(fmt.dtype)
        rects, hmax = [], 0
        for t in tl:
            ys, ye, xs, xe = t.out_src(s)
            dy0, _, dx0, _ = t.out_dst(s)
            rects += [ys, xs, dy0, dx0, ye - ys, xe - xs]
            hmax = max(hmax, ye - ys)
        rd = torch.tensor(rects, dtype=torch.int32).to(output.device, non_blocking=True)
        _, c, th, tw = fmt.bchw(block)
        _, _, oh, ow = fmt.bchw(output)
        with torch.cuda.device(output.device):
            _lib.check(getattr(_lib.load(), fmt.paste)(torch.cuda.current_stream().cuda_stream, block.data_ptr(), *fmt.native_bc(batch, c),
                                                       len(tl), th, tw, rd.data_ptr(), hmax, oh, ow, output.data_ptr()))

    @staticmethod
    def _blend_tiles(fmt, x, per_rank, owned_all, batch, channel, height, width, tile_size, s):
        """The overlap-blend canvas of `test_tile(..., blend=True)` from every rank's tiles: out = sum_k w_k v_k / sum_k w_k over the
        windows k that contain the pixel, in row-major tile order (tiling.blend_weight_1d).  GPU: ONE gather-form launch
        over the whole canvas, fed by a table of tile addresses (the tiles stay where the batched calls / the all-gather left them) and
        the geometry table.  Host tensors (the CPU-side tests of the partition / gather logic): the same definition as a torch loop,
        fp32 in the kernel's operation order."""
        where = {}                                  # tile number -> (the block of its rank and class, its place in that block)
        for r, res in enumerate(per_rank):
            for hw, tl in owned_all[r].items():
                for k, t in enumerate(tl):
                    where[t.index] = (t, res[hw], k)
        tiles = [where[i][0] for i in range(len(where))]
        shape = tiling.tile_shape(fmt.dtype, batch, channel, height * s, width * s)
        if not x.is_cuda:
            def w32(length, lead, trail):
                i = torch.arange(length, dtype=torch.int32)
                one = torch.ones(length)
                wl = one if lead == 0 else torch.minimum(one, (2 * i + 1).float() / float(4 * lead))
                wr = one if trail == 0 else torch.minimum(one, (2 * (length - 1 - i) + 1).float() / float(4 * trail))
                return torch.minimum(wl, wr)
            acc = torch.zeros(shape)
            den = torch.zeros(tiling.tile_shape(fmt.dtype, 1, 1, height * s, width * s))
            for t, block, k in (where[i] for i in range(len(where))):
                ay, ax, th, tw, ly, ry, lx, rx = tiling.blend_geom(t, s)
                w = (w32(th, ly, ry)[:, None] * w32(tw, lx, rx)[None, :]).reshape(tiling.tile_shape(fmt.dtype, 1, 1, th, tw))
                fmt.window(acc, ay, ay + th, ax, ax + tw).add_(w * block[k * batch:(k + 1) * batch].float())
                fmt.window(den, ay, ay + th, ax, ax + tw).add_(w)
            out = acc / den
            return out if fmt.dtype.is_floating_point else out.clamp_(0, 255).round_().to(fmt.dtype)
        output = torch.empty(shape, dtype=fmt.dtype, device=x.device)          # every element is written once: nothing to zero
        blocks, ptrs = {}, []
        for t, block, k in (where[i] for i in range(len(where))):
            blk = blocks.setdefault(id(block), block.contiguous().to(fmt.dtype))        # (kept alive until the launch is enqueued)
            th, tw = t.in_hw[0] * s, t.in_hw[1] * s
            ptrs.append(blk.data_ptr() + k * batch * channel * th * tw * blk.element_size())
        tab = torch.tensor(ptrs, dtype=torch.int64).to(x.device, non_blocking=True)
        geo = torch.tensor(tiling.blend_table(tiles, s), dtype=torch.int32).to(x.device, non_blocking=True)
        ny, nx = math.ceil(height / tile_size), math.ceil(width / tile_size)
        with torch.cuda.device(x.device):
            _lib.check(getattr(_lib.load(), fmt.blend)(torch.cuda.current_stream().cuda_stream, tab.data_ptr(), geo.data_ptr(), len(tiles), ny, nx,
                                                       tile_size * s, *fmt.native_bc(batch, channel), height * s, width * s, output.data_ptr()))
        return output

"""DISTS (Ding et al., "Image Quality Assessment: Unifying Structure and Texture Similarity"; `pyiqa.create_metric('dists')`) on the
MI355X path: the full-reference metric SR papers report beside LPIPS.

    DISTS(pretrained_model_path=..., backbone_model_path=None)(x, y) -> (B,) float64, lower is better

x, y: float32 (B,3,H,W) RGB in [0,1] on a GPU, H, W >= 8.  Everything runs in libfemasr_hip.so (csrc/dists.hip + the fp32 conv kernels with
a ReLU epilogue); there is no CPU path.  The definition is restated in float64 in tests/dists_ref.py.  No resize-to-256 preprocessing.

Weights.  No pyiqa / DISTS_pytorch source and no DISTS weight file is available to this project.  The checkpoint names below are written
from memory of those packages' module structure (`alpha`, `beta` of shape (1,1475,1,1); the backbone as `stageK.I.weight|bias` with I the
torchvision `features` index) and are NOT verified against a real file; the whole mapping is `_NAME_RULES`: correct it there if a
checkpoint's names differ.  torchvision's `features.I.*` and an LPIPS-VGG file's `net.sliceK.I.*` are accepted for the backbone;
`mean`, `std` and the `stageK.I.filter` buffers of the pool layers are ignored (they are constants of the method).
"""
import ctypes
import re
import warnings
from collections import OrderedDict

import torch
import torch.nn as nn

from . import _lib
from .lpips import _unwrap

METRIC_TYPES = ('dists',)

# (stage K, torchvision feature index I, Cin, Cout); every conv 3x3 stride 1 pad 1 + ReLU; an L2 pool in front of stages 2..5
_CONVS = ((1, 0, 3, 64), (1, 2, 64, 64),
          (2, 5, 64, 128), (2, 7, 128, 128),
          (3, 10, 128, 256), (3, 12, 256, 256), (3, 14, 256, 256),
          (4, 17, 256, 512), (4, 19, 512, 512), (4, 21, 512, 512),
          (5, 24, 512, 512), (5, 26, 512, 512), (5, 28, 512, 512))
MAP_CHANNELS = (3, 64, 128, 256, 512, 512)
N_CHANNELS = sum(MAP_CHANNELS)      # 1475
MIN_SIDE = 8
_STAGE_OF = {i: k for k, i, _, _ in _CONVS}


def _by_index(m):
    i = int(m[1])
    return None if i not in _STAGE_OF else f'stage{_STAGE_OF[i]}.{i}.{m[2]}'


# checkpoint name -> canonical name (None: not a DISTS weight, ignored).  One table: correct it here if a checkpoint's names differ.
_NAME_RULES = (
    (re.compile(r'(alpha|beta)'), lambda m: m[1]),
    (re.compile(r'stage\d\.(\d+)\.(weight|bias)'), _by_index),            # the DISTS module
    (re.compile(r'features\.(\d+)\.(weight|bias)'), _by_index),           # torchvision VGG16
    (re.compile(r'net\.slice\d\.(\d+)\.(weight|bias)'), _by_index),       # an LPIPS-VGG file's backbone
)


def expected_shapes():
    """Canonical key -> shape of every weight the metric needs."""
    out = OrderedDict()
    for k, i, cin, cout in _CONVS:
        out[f'stage{k}.{i}.weight'] = (cout, cin, 3, 3)
        out[f'stage{k}.{i}.bias'] = (cout,)
    out['alpha'] = (1, N_CHANNELS, 1, 1)
    out['beta'] = (1, N_CHANNELS, 1, 1)
    return out


def canonical_state_dict(*state_dicts):
    """Map one or more checkpoint state dicts (backbone and alpha / beta in one, or split) to the canonical keys and check every shape.
    Raises KeyError naming the missing keys, ValueError naming the mis-shaped ones."""
    want = expected_shapes()
    out = OrderedDict()
    for sd in state_dicts:
        for key, v in _unwrap(sd).items():
            for rx, fn in _NAME_RULES:
                m = rx.fullmatch(key)
                if m:
                    ck = fn(m)
                    if ck is not None and ck in want:
                        out[ck] = v.detach().to(torch.float32).cpu()
                    break
    missing = [k for k in want if k not in out]
    if missing:
        raise KeyError(f'DISTS weights: missing {missing} (accepted layouts: alpha, beta; stageK.I.* / features.I.* / net.sliceK.I.* '
                       'for the backbone)')
    bad = [f'{k}: {tuple(out[k].shape)} != {want[k]}' for k in want if tuple(out[k].shape) != want[k]]
    if bad:
        raise ValueError(f'DISTS weights: wrong shapes {bad}')
    return OrderedDict((k, out[k]) for k in want)


def load_dists_weights(pretrained_model_path, backbone_model_path=None):
    """Canonical state dict from one file holding backbone, alpha and beta, or an alpha / beta file plus a backbone file."""
    sds = [torch.load(pretrained_model_path, map_location='cpu', weights_only=True)]
    if backbone_model_path is not None:
        sds.insert(0, torch.load(backbone_model_path, map_location='cpu', weights_only=True))
    return canonical_state_dict(*sds)


def map_shapes(H, W):
    """[(h, w, C)] of the six maps at input (H, W): the input, then the five stage outputs (the pool halves with ceil)."""
    if H < MIN_SIDE or W < MIN_SIDE:
        raise ValueError(f'DISTS needs H, W >= {MIN_SIDE}, got {H}x{W}')
    out, y, x = [(H, W, 3)], H, W
    for k, c in enumerate(MAP_CHANNELS[1:]):
        if k:
            y, x = (y + 1) // 2, (x + 1) // 2
        out.append((y, x, c))
    return out


class _Holder(nn.Module):
    pass


class DISTS(nn.Module):
    """Parameter holder with the canonical state-dict names; forward runs femasr_dists_forward on the parameters' GPU."""

    def __init__(self, pretrained_model_path=None, backbone_model_path=None, state_dict=None):
        super().__init__()
        for k, i, cin, cout in _CONVS:
            if not hasattr(self, f'stage{k}'):
                self.add_module(f'stage{k}', _Holder())
            getattr(self, f'stage{k}').add_module(str(i), nn.Conv2d(cin, cout, 3, 1, 1))
        self.alpha = nn.Parameter(torch.full((1, N_CHANNELS, 1, 1), 0.1))
        self.beta = nn.Parameter(torch.full((1, N_CHANNELS, 1, 1), 0.1))
        for p in self.parameters():
            p.requires_grad_(False)
        if pretrained_model_path is not None:
            self.load_state_dict(load_dists_weights(pretrained_model_path, backbone_model_path))
        elif state_dict is not None:
            self.load_state_dict(canonical_state_dict(state_dict))
        elif backbone_model_path is not None:
            raise ValueError('DISTS: backbone_model_path needs pretrained_model_path (the file with alpha and beta)')
        else:       # a DISTS with torch's random init scores nothing meaningful: say so (load_state_dict may still follow)
            warnings.warn('DISTS() built without weights (no pretrained_model_path / state_dict): its parameters are random until '
                          'load_state_dict()', stacklevel=2)
        self.eval()
        self._handle = None
        self._handle_device = None
        self._stamp = None
        self._ws = None

    # ---- native handle: repacked copies of the weights, re-pushed when a parameter changed (version counter / storage)
    def _param_stamp(self):
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    def _native(self, device):
        if device.type != 'cuda':
            raise _lib.FemasrError('DISTS (MI355X build) runs on a GPU device only; move the module to cuda. There is no CPU fallback.')
        lib = _lib.load()
        dev_index = device.index if device.index is not None else torch.cuda.current_device()
        if self._handle is None or self._handle_device != dev_index:
            self._release()
            h = ctypes.c_void_p()
            _lib.check(lib.femasr_dists_create(dev_index, ctypes.byref(h)))
            self._handle, self._handle_device, self._stamp = h, dev_index, None
        stamp = self._param_stamp()
        if stamp != self._stamp:
            torch.cuda.synchronize(device)
            for key, t in self.state_dict().items():
                src = t.detach().to(device=device, dtype=torch.float32).contiguous()
                shape = (ctypes.c_int64 * src.dim())(*src.shape)
                _lib.check(lib.femasr_dists_set_weight(self._handle, key.encode(), _lib.ptr(src), shape, src.dim()))
            _lib.check(lib.femasr_dists_finalize_weights(self._handle))
            self._stamp = stamp
        return lib, self._handle

    def _release(self):
        if getattr(self, '_handle', None) is not None:
            _lib.load().femasr_dists_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def workspace_bytes(self, B, H, W):
        """Bytes femasr_dists_forward needs for B pairs at (H, W) (a caller-owned workspace: forward(..., workspace=))."""
        lib, h = self._native(self.alpha.device)
        nbytes = ctypes.c_size_t()
        _lib.check(lib.femasr_dists_workspace_bytes(h, B, H, W, ctypes.byref(nbytes)))
        return int(nbytes.value)

    def _workspace(self, nbytes, device):
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != device:
            self._ws = None
            self._ws = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        return self._ws

    @torch.no_grad()
    def forward(self, x, y, per_layer=False, workspace=None):
        """(B,3,H,W) pairs in [0,1] -> (B,) float64 (and the (B,6,2) sums of alpha S1 / beta S2 per map with per_layer=True).  Runs on the
        current stream.  workspace: a caller-owned uint8 tensor of at least workspace_bytes(B, H, W) bytes (default: the module's own)."""
        if x.shape != y.shape or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f'DISTS: expected two (B,3,H,W) tensors of one shape, got {tuple(x.shape)} and {tuple(y.shape)}')
        device = self.alpha.device
        if x.device != device or y.device != device:
            raise _lib.FemasrError(f'DISTS: inputs on {x.device} / {y.device}, module on {device} (no CPU fallback)')
        lib, h = self._native(device)
        B, _, H, W = x.shape
        x = x.detach().to(torch.float32).contiguous()
        y = y.detach().to(torch.float32).contiguous()
        out = torch.empty(B, dtype=torch.float64, device=device)
        terms = torch.empty((B, 6, 2), dtype=torch.float64, device=device)
        # pairs per call: the 2-image-per-pair feature tensors stay below 2^31 elements and at most 65535 pairs (a grid dimension); pairs
        # are independent and every sum is per pair, so the split does not change a bit
        step = max(1, min(65535, ((1 << 31) - 1) // (2 * max(H * W * 64, 1))))
        stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        for b0 in range(0, B, step):
            nb = min(step, B - b0)
            nbytes = ctypes.c_size_t()
            _lib.check(lib.femasr_dists_workspace_bytes(h, nb, H, W, ctypes.byref(nbytes)))
            if workspace is None:
                ws = self._workspace(nbytes.value, device)
            else:
                ws = workspace
                if ws.device != device or ws.dtype != torch.uint8 or ws.numel() < nbytes.value or ws.data_ptr() % 256:
                    raise ValueError(f'DISTS: workspace must be a 256-byte aligned uint8 tensor of >= {nbytes.value} bytes on {device}')
            _lib.check(lib.femasr_dists_forward(h, stream, _lib.ptr(x[b0:b0 + nb]), _lib.ptr(y[b0:b0 + nb]), nb, H, W, _lib.ptr(ws),
                                                nbytes.value, _lib.ptr(out[b0:b0 + nb]), _lib.ptr(terms[b0:b0 + nb])))
        return (out, terms) if per_layer else out


def create_metric(metric_type, device=None, pretrained_model_path=None, backbone_model_path=None, **ignore_kwargs):
    """pyiqa.create_metric('dists', pretrained_model_path=..., ...)."""
    if metric_type not in METRIC_TYPES:
        raise ValueError(f'unknown DISTS metric type {metric_type!r} (known: {sorted(METRIC_TYPES)})')
    if pretrained_model_path is None:
        raise ValueError("metric 'dists' needs pretrained_model_path (no network access: pass the local DISTS weight file)")
    m = DISTS(pretrained_model_path=pretrained_model_path, backbone_model_path=backbone_model_path)
    return m.to(device) if device is not None else m

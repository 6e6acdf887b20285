"""Inference surface of the reference's `FeMaSRModel` (basicsr/models/femasr_model.py) on the MI355X path.

What is mirrored (same names, argument meaning and behaviour):
  __init__(opt)            femasr_model.py:20-70   build_network(opt['network_g']); LQ stage: frozen HQ net from
                                                   path.pretrain_network_hq (also loaded non-strictly into net_g);
                                                   path.pretrain_network_g with path.strict_load
  load_network             base_model.py:291-323   {'params'|'params_ema'} key, 'module.' prefix stripping, and with
                                                   strict=False same-name/different-size tensors are skipped
  feed_data / test         femasr_model.py:135-138,217-227   (whole image below 8000x8000 pixels, else test_tile)
  validation               base_model.py:45-57 -> nondist_validation femasr_model.py:234-328: per image feed/test,
                                                   tensor2img, save under path.visualization/<dataset>/<name>_<suffix|opt name>.png,
                                                   metric averages
  extract_gt_indices       femasr_model.py:144-146  `net_hq(gt)` -> indices
What is NOT here: training (optimizers, losses, discriminator, schedulers), best-model bookkeeping, tensorboard.
Metrics: the reference evaluates them with `pyiqa` (not installed here): 'psnr' and 'ssim' follow the BasicSR
definitions (crop_border, test_y_channel on the BT.601 Y of the uint8-rounded image).  calculate_psnr / calculate_ssim below
(numpy / scipy, fp64) ARE those definitions; validation scores them on the GPU (femasr_amd.psnr_ssim, csrc/psnr_ssim.hip) on the
uint8 SR and GT images already on the device, within 1e-9 dB / 1e-12 of these functions.  'lpips' (AlexNet) and 'lpips-vgg'
(VGG16) are LPIPS v0.1 on the GPU (femasr_amd.lpips, csrc/lpips.hip) when their options carry `pretrained_model_path`
(pyiqa's keyword; optionally `backbone_model_path`): scored on (sr_u8 / 255, gt) as femasr_model.py:262 does, the uint8 SR
image never leaving the device.  'niqe' is the no-reference NIQE (BasicSR's calculate_niqe, restated below as calculate_niqe with its
pieces: _niqe_y, _convolve_nearest, imresize / imresize_tables, aggd_tables, niqe_features, niqe_score_from_features) when its options
carry `pretrained_model_path` (a local niqe_pris_params.npz): scored on sr_u8 on the GPU (femasr_amd.niqe, csrc/niqe.hip) for every image,
also of a dataset without ground truth; only its tail (36 numbers per block) runs on the host, in the definition's own function.  'dists'
is DISTS on the GPU (femasr_amd.dists, csrc/dists.hip) under the same keywords and on the same tensors as the LPIPS types.  Without
a weight / parameter file (none is ever downloaded) these types, like every other type (musiq, ...), are reported as skipped (None).
There is no CPU path: the module needs a GPU and the HIP library.
"""
import logging
import os
from collections import OrderedDict
from copy import deepcopy

import numpy as np
import torch

from .. import dists as dists_metric
from .. import imgproc
from .. import lpips as lpips_metric
from .. import niqe as niqe_metric
from .. import psnr_ssim
from ..archs import build_network
from . import MODEL_REGISTRY

logger = logging.getLogger('femasr_amd')


def tensor2img(tensor, rgb2bgr=False, min_max=(0, 1)):
    """img_util.py:38-94 for the (1,3,H,W) / (3,H,W) case: clamp, scale, round half to even, uint8 HWC.
    The reference returns BGR for cv2.imwrite; images are written with PIL here, so the default stays RGB."""
    t = tensor.detach().float().cpu()
    if t.dim() == 4:
        t = t.squeeze(0)
    t = (t.clamp(*min_max) - min_max[0]) / (min_max[1] - min_max[0])
    img = (t.numpy().transpose(1, 2, 0) * 255.0).round().astype(np.uint8)
    return img[:, :, ::-1].copy() if rgb2bgr else img


def _to_y(img_u8_rgb):
    """BT.601 luma of an RGB uint8 image, the `rgb2ycbcr(..., y_only=True)` of BasicSR, range [16, 235]."""
    x = img_u8_rgb.astype(np.float64) / 255.0
    return (x @ np.array([65.481, 128.553, 24.966])) + 16.0


def calculate_psnr(img, img2, crop_border=0, test_y_channel=False, **_):
    a, b = img.astype(np.float64), img2.astype(np.float64)
    if crop_border:
        a, b = a[crop_border:-crop_border, crop_border:-crop_border], b[crop_border:-crop_border, crop_border:-crop_border]
    if test_y_channel:
        a, b = _to_y(a.astype(np.uint8)), _to_y(b.astype(np.uint8))
    mse = np.mean((a - b) ** 2)
    return float('inf') if mse == 0 else float(10.0 * np.log10(255.0 * 255.0 / mse))


def _ssim_plane(a, b):
    from scipy.signal import convolve2d
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / (2 * 1.5 ** 2))
    g /= g.sum()
    win = np.outer(g, g)

    def f(x):
        return convolve2d(x, win, mode='valid')
    mu1, mu2 = f(a), f(b)
    s1, s2, s12 = f(a * a) - mu1 * mu1, f(b * b) - mu2 * mu2, f(a * b) - mu1 * mu2
    return float((((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))).mean())


def calculate_ssim(img, img2, crop_border=0, test_y_channel=False, **_):
    a, b = img.astype(np.float64), img2.astype(np.float64)
    if crop_border:
        a, b = a[crop_border:-crop_border, crop_border:-crop_border], b[crop_border:-crop_border, crop_border:-crop_border]
    if test_y_channel:
        return _ssim_plane(_to_y(a.astype(np.uint8)), _to_y(b.astype(np.uint8)))
    return float(np.mean([_ssim_plane(a[..., c], b[..., c]) for c in range(a.shape[2])]))


_METRICS = {'psnr': calculate_psnr, 'ssim': calculate_ssim}


# ---------------------------------------------------------------- imresize and NIQE: the definitions (numpy, fp64)
def _cubic(x):
    """matlab_functions.py:6-13."""
    ax = np.abs(x)
    ax2, ax3 = ax * ax, ax * ax * ax
    return (1.5 * ax3 - 2.5 * ax2 + 1) * (ax <= 1) + (-0.5 * ax3 + 2.5 * ax2 - 4 * ax + 2) * ((ax > 1) & (ax <= 2))


def imresize_tables(in_length, out_length, scale, antialiasing=True):
    """calculate_weights_indices (matlab_functions.py:16-82) in fp64: (weights (out_length, taps) float64, rows (out_length, taps) int32).
    The reference pads the image symmetrically; here the padding is folded into the indices: a 1-based index i < 1 reads 1 - i, i > n reads
    2n + 1 - i, and `rows` holds them 0-based.  Raises ValueError where a reflected index leaves the image (the reference raises there too).
    The column trimming is the reference's: the first (last) column goes when ANY of its weights is exactly zero."""
    import math
    if not (in_length >= 1 and out_length >= 1 and scale > 0):
        raise ValueError(f'imresize: length {in_length} -> {out_length} at scale {scale}')
    kernel_width = 4.0
    aa = scale < 1 and antialiasing
    if aa:
        kernel_width = kernel_width / scale
    x = np.arange(1, out_length + 1, dtype=np.float64)
    u = x / scale + 0.5 * (1 - 1 / scale)
    left = np.floor(u - kernel_width / 2)
    p = math.ceil(kernel_width) + 2
    ind = left[:, None] + np.arange(p, dtype=np.float64)[None, :]
    dist = u[:, None] - ind
    w = scale * _cubic(dist * scale) if aa else _cubic(dist)
    total = np.zeros(out_length)
    for k in range(p):                  # the row sums in ascending order
        total = total + w[:, k]
    w = w / total[:, None]
    zeros = (w == 0).sum(0)
    if zeros[0] != 0:
        ind, w = ind[:, 1:p - 1], w[:, 1:p - 1]
    if zeros[-1] != 0:
        ind, w = ind[:, :p - 2], w[:, :p - 2]
    i = ind.astype(np.int64)
    i = np.where(i < 1, 1 - i, i)
    i = np.where(i > in_length, 2 * in_length + 1 - i, i)
    if i.min() < 1 or i.max() > in_length:
        raise ValueError(f'imresize: a length of {in_length} is too short for scale {scale}'
                         f'{" with antialiasing" if aa else ""}: the symmetric padding would leave the image')
    return np.ascontiguousarray(w), np.ascontiguousarray(i - 1, dtype=np.int32)


def imresize(img, scale, antialiasing=True):
    """MATLAB-style bicubic imresize (matlab_functions.py:86-178) of (..., H, W) planes in fp64: the H pass, then the W pass; every output
    is one accumulator over its taps in ascending order from 0.0.  Output size ceil(n * scale)."""
    import math
    img = np.asarray(img, dtype=np.float64)
    h, w = img.shape[-2:]
    oh, ow = math.ceil(h * scale), math.ceil(w * scale)
    wh, ih = imresize_tables(h, oh, scale, antialiasing)
    ww, iw = imresize_tables(w, ow, scale, antialiasing)
    out1 = np.zeros(img.shape[:-2] + (oh, w))
    for k in range(wh.shape[1]):
        out1 = out1 + wh[:, k][:, None] * img[..., ih[:, k], :]
    out2 = np.zeros(img.shape[:-2] + (oh, ow))
    for k in range(ww.shape[1]):
        out2 = out2 + ww[:, k] * out1[..., :, iw[:, k]]
    return out2


def _niqe_y(img_u8_rgb):
    """The rounded BT.601 luma NIQE scores, as ONE fixed-order fp64 expression (no BLAS, unlike _to_y): on the 194 RGB triples whose exact Y
    is k + 0.5 one ulp decides the rounded pixel."""
    x = img_u8_rgb.astype(np.float64)
    return np.round(((65.481 * x[..., 0] + 128.553 * x[..., 1]) + 24.966 * x[..., 2]) / 255.0 + 16.0)


def _convolve_nearest(x, window):
    """scipy.ndimage.convolve(x, window, mode='nearest') for an odd square window, restated: the raster walk over the FLIPPED window, one
    accumulator from 0.0, no fma.  Equal to scipy bit for bit (tests/test_niqe_host.py); in flat regions x - mu is rounding noise whose sign
    decides which pixels count as negative, so the order is part of the definition."""
    k = window.shape[0]
    r = k // 2
    wf = window[::-1, ::-1]
    xp = np.pad(x, r, mode='edge')
    h, w = x.shape
    s = np.zeros((h, w))
    for a in range(k):
        for b in range(k):
            s = s + wf[a, b] * xp[a:a + h, b:b + w]
    return s


_AGGD_TABLES = None


def aggd_tables():
    """(r_gam, gamma(1/gam), gamma(2/gam), gamma(3/gam), gam), gam = arange(0.2, 10.001, 0.001) (9801 values): the grid of the AGGD shape
    search, shared by the definition and the GPU path (which has no gamma function).  math.gamma, not scipy.special.gamma."""
    global _AGGD_TABLES
    if _AGGD_TABLES is None:
        import math
        gam = np.arange(0.2, 10.001, 0.001)
        rec = np.reciprocal(gam)
        g1 = np.array([math.gamma(v) for v in rec])
        g2 = np.array([math.gamma(v) for v in rec * 2])
        g3 = np.array([math.gamma(v) for v in rec * 3])
        _AGGD_TABLES = (g2 * g2 / (g1 * g3), g1, g2, g3, gam)
    return _AGGD_TABLES


def _aggd(x):
    """Asymmetric generalised Gaussian fit of one map: (grid position, alpha, beta_l, beta_r, margin); margin is the gap between the best and
    the second-best |r_gam - rn| (NaN when rn is).  An empty side has mean NaN, and argmin of an all-NaN objective is 0: alpha 0.2, that side's beta NaN."""
    r_gam, g1, _, g3, gam = aggd_tables()
    x = x.ravel()
    with np.errstate(all='ignore'):
        neg, pos = x[x < 0], x[x > 0]
        l = np.sqrt(np.float64(np.sum(neg * neg)) / np.float64(neg.size))
        r = np.sqrt(np.float64(np.sum(pos * pos)) / np.float64(pos.size))
        g = l / r
        rhat = np.mean(np.abs(x)) ** 2 / np.mean(x * x)
        rn = rhat * (g * g * g + 1) * (g + 1) / ((g * g + 1) * (g * g + 1))
        d = r_gam - rn
        p = int(np.argmin(d * d))
        two = np.partition(np.abs(d), 1)[:2]
        k = np.sqrt(g1[p] / g3[p])
        return p, gam[p], l * k, r * k, float(two[1] - two[0])


def _niqe_block_feature(block):
    """18 features of one block at one scale, the 5 grid positions and the smallest margin."""
    _, g1, g2, _, _ = aggd_tables()
    p, alpha, bl, br, margin = _aggd(block)
    feat, poss, margins = [alpha, (bl + br) / 2], [p], [margin]
    for shift in ([0, 1], [1, 0], [1, 1], [1, -1]):
        p, alpha, bl, br, margin = _aggd(block * np.roll(block, shift, axis=(0, 1)))          # circular inside the block
        feat += [alpha, (br - bl) * (g2[p] / g1[p]), bl, br]
        poss.append(p)
        margins.append(margin)
    return feat, poss, margins


def niqe_features(y, window, details=None):
    """(features (n_blocks, 36), alpha grid positions (n_blocks, 10)) of a rounded luma plane.  Blocks of 96 x 96 (48 x 48 at the second
    scale) in the order `for iw: for ih`.  `details`, a dict, receives the planes y, z, y2, z2 and the alpha margins (n_blocks, 10)."""
    window = np.asarray(window, dtype=np.float64)
    nh, nw = y.shape[0] // 96, y.shape[1] // 96
    if nh < 1 or nw < 1:
        raise ValueError(f'niqe: a plane of {y.shape[0]}x{y.shape[1]} holds no 96x96 block')
    y = np.ascontiguousarray(y[:nh * 96, :nw * 96], dtype=np.float64)
    feats, poss, margins = [], [], []
    for scale in (1, 2):
        mu = _convolve_nearest(y, window)
        sigma = np.sqrt(np.abs(_convolve_nearest(y * y, window) - mu * mu))
        z = (y - mu) / (sigma + 1)
        if details is not None:
            details['y' if scale == 1 else 'y2'], details['z' if scale == 1 else 'z2'] = y, z
        n = 96 // scale
        rows = [_niqe_block_feature(z[ih * n:(ih + 1) * n, iw * n:(iw + 1) * n]) for iw in range(nw) for ih in range(nh)]
        feats.append(np.array([r[0] for r in rows]))
        poss.append(np.array([r[1] for r in rows]))
        margins.append(np.array([r[2] for r in rows]))
        if scale == 1:
            y = imresize(y / 255.0, 0.5, antialiasing=True) * 255.0        # not rounded
    if details is not None:
        details['margin'] = np.concatenate(margins, 1)
    return np.concatenate(feats, 1), np.concatenate(poss, 1).astype(np.int32)


def niqe_score_from_features(features, mu_pris, cov_pris):
    """NIQE's tail on the (n_blocks, 36) features, shared by the definition and the GPU path: nanmean, the covariance of the rows without
    NaN, pinv of the pooled covariance, the quadratic form.  Fewer than two rows without NaN leave the covariance undefined: NaN."""
    import warnings
    d = np.asarray(features, dtype=np.float64).reshape(-1, 36)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', category=RuntimeWarning)
        mu_d = np.nanmean(d, axis=0)
    dn = d[~np.isnan(d).any(axis=1)]
    if dn.shape[0] < 2:
        return float('nan')
    pooled = (np.asarray(cov_pris, dtype=np.float64).reshape(36, 36) + np.cov(dn, rowvar=False)) / 2
    diff = np.asarray(mu_pris, dtype=np.float64).reshape(36) - mu_d
    if not (np.isfinite(pooled).all() and np.isfinite(diff).all()):
        return float('nan')
    return float(np.sqrt(diff @ np.linalg.pinv(pooled) @ diff))


def calculate_niqe(img, crop_border, params, **_):
    """BasicSR's calculate_niqe(img, crop_border, input_order='HWC', convert_to='y') for a uint8 RGB image; params = (mu_pris_param,
    cov_pris_param, gaussian_window) as femasr_amd.niqe.load_pris_params returns them."""
    mu_pris, cov_pris, window = params
    y = _niqe_y(img)
    if crop_border:
        y = y[crop_border:-crop_border, crop_border:-crop_border]
    return niqe_score_from_features(niqe_features(y, window)[0], mu_pris, cov_pris)


@MODEL_REGISTRY.register()
class FeMaSRModel:
    def __init__(self, opt):
        self.opt = opt
        if opt.get('is_train', False):
            raise NotImplementedError('femasr_amd.models.FeMaSRModel is inference-only (is_train must be false)')
        if not torch.cuda.is_available():
            raise RuntimeError('FeMaSRModel needs a GPU: the hot path has no CPU implementation')
        self.device = torch.device('cuda', int(opt.get('local_rank', 0)))
        self.is_train = False
        path = opt.get('path', {}) or {}
        self.net_g = build_network(opt['network_g']).to(self.device).eval()

        self.LQ_stage = opt['network_g'].get('LQ_stage', False)
        self.net_hq = None
        if self.LQ_stage:
            load_path = path.get('pretrain_network_hq', None)
            if load_path is not None:       # the reference asserts it (needed for training); inference can do without
                hq_opt = deepcopy(opt['network_g'])
                hq_opt['LQ_stage'] = False
                self.net_hq = build_network(hq_opt).to(self.device).eval()
                self.load_network(self.net_hq, load_path, path.get('strict_load', True))
                self.load_network(self.net_g, load_path, False)
        load_path = path.get('pretrain_network_g', None)
        if load_path is not None:
            logger.info('Loading net_g from %s', load_path)
            self.load_network(self.net_g, load_path, path.get('strict_load', True))
        self.metric_results = {}

    # ---- base_model.py:258-323
    def load_network(self, net, load_path, strict=True, param_key='params'):
        if str(load_path).startswith('https://'):
            raise RuntimeError(f'no network in this environment: download {load_path} and pass the local file')
        load_net = torch.load(load_path, map_location='cpu')
        if param_key is not None:
            if param_key not in load_net and 'params' in load_net:
                param_key = 'params'
            load_net = load_net[param_key]
        load_net = OrderedDict((k[7:] if k.startswith('module.') else k, v) for k, v in load_net.items())
        crt = net.state_dict()
        missing, unexpected = sorted(set(crt) - set(load_net)), sorted(set(load_net) - set(crt))
        if missing or unexpected:
            logger.warning('Current net - loaded net: %s; loaded net - current net: %s', missing, unexpected)
        if not strict:
            for k in sorted(set(crt) & set(load_net)):
                if tuple(crt[k].shape) != tuple(load_net[k].shape):
                    logger.warning('Size different, ignore [%s]: crt_net %s; load_net %s', k, tuple(crt[k].shape),
                                   tuple(load_net[k].shape))
                    load_net[k + '.ignore'] = load_net.pop(k)
        return net.load_state_dict(load_net, strict=strict)

    def feed_data(self, data):
        self.lq = data['lq'].to(self.device)
        if 'gt' in data:
            self.gt = data['gt'].to(self.device)
        elif hasattr(self, 'gt'):
            del self.gt             # never score an image against the previous item's ground truth

    @torch.no_grad()
    def test(self):
        min_size = 8000 * 8000
        _, _, h, w = self.lq.shape
        # `val: tile_blend: true` (an extension key, absent = false): the tiled branch blends the tile overlaps (FeMaSRNet.test_tile)
        val = self.opt.get('val') or {}
        blend = bool(val.get('tile_blend', False))
        # `val: color_fix: true` (an extension key, absent = false): the opt-in wavelet colour fix on either branch; `val: color_fix_levels: N`
        # sets the network's `color_fix_levels` (absent: the network keeps its own, 5)
        kw = {'blend': True} if blend else {}
        fix = {'color_fix': True} if val.get('color_fix', False) else {}
        if fix and val.get('color_fix_levels') is not None:
            self.net_g.color_fix_levels = int(val['color_fix_levels'])
        # `val: self_ensemble: true` (an extension key, absent = false): the opt-in x8 geometric self-ensemble on either branch
        if val.get('self_ensemble', False):
            fix['self_ensemble'] = True
        if h * w < min_size:
            self.output = self.net_g.test(self.lq, **fix)
        else:
            self.output = self.net_g.test_tile(self.lq, **kw, **fix)

    @torch.no_grad()
    def extract_gt_indices(self, gt=None):
        """`self.gt_rec, _, _, gt_indices = self.net_hq(self.gt)` (femasr_model.py:145-146) as an inference service."""
        if self.net_hq is None:
            raise RuntimeError('no HQ network: set path.pretrain_network_hq in an LQ-stage option file')
        self.gt_rec, _, _, gt_indices = self.net_hq(self.gt if gt is None else gt.to(self.device))
        return gt_indices

    def validation(self, dataloader, current_iter, tb_logger, save_img=False, save_as_dir=None):
        return self.nondist_validation(dataloader, current_iter, tb_logger, save_img, save_as_dir)

    def nondist_validation(self, dataloader, current_iter, tb_logger, save_img, save_as_dir=None):
        dataset_name = dataloader.dataset.opt['name']
        val_opt = self.opt.get('val', {}) or {}
        metrics = val_opt.get('metrics') or {}
        self.metric_results = {name: 0.0 for name in metrics}
        gpu_metrics = {name: self._gpu_metric(name, m) for name, m in metrics.items()
                       if (m.get('type') in lpips_metric.METRIC_NETS or m.get('type') in dists_metric.METRIC_TYPES)
                       and m.get('pretrained_model_path')}
        # psnr / ssim on the device; the CPU functions in _METRICS are their definition
        pixel_metrics = {name: psnr_ssim.create_metric(m['type'], **{k: v for k, v in m.items() if k not in ('type', 'better')})
                         for name, m in metrics.items() if m.get('type') in _METRICS}
        # niqe needs no ground truth: scored on the device for every image, also of a dataset without `gt`
        noref_metrics = {name: niqe_metric.create_metric('niqe', **{k: v for k, v in m.items() if k not in ('type', 'better')})
                         for name, m in metrics.items() if m.get('type') == 'niqe' and m.get('pretrained_model_path')}
        skipped = sorted(name for name, m in metrics.items()
                         if m.get('type') not in _METRICS and name not in gpu_metrics and name not in noref_metrics)
        if skipped:
            logger.warning('metrics %s are skipped: lpips / lpips-vgg need `pretrained_model_path` (a local LPIPS weight file), dists needs '
                           '`pretrained_model_path` (a local DISTS weight file), niqe needs '
                           '`pretrained_model_path` (a local niqe_pris_params.npz), other pyiqa types are not implemented in this build',
                           skipped)
        # `val: io_threads: N` (extension key; absent: Image.save here, as ever): the saves go through a pngio.PngWriter - PNG row filters
        # on the GPU, N threads deflate and write behind the next forward; the same pixels in the files
        writer = None
        if save_img and val_opt.get('io_threads'):
            from .. import pngio
            writer = pngio.PngWriter(threads=min(int(val_opt['io_threads']), pngio.MAX_THREADS))
        try:
            n = self._validate_images(dataloader, dataset_name, val_opt, metrics, save_img, save_as_dir, writer, noref_metrics, pixel_metrics,
                                      gpu_metrics)
        finally:
            if writer is not None:
                writer.close()                              # every file is written before the metrics are logged
        for name in self.metric_results:
            self.metric_results[name] = self.metric_results[name] / max(n, 1) if name not in skipped else None
        if metrics:
            logger.info('Validation %s: %s', dataset_name, self.metric_results)
        return self.metric_results

    def _validate_images(self, dataloader, dataset_name, val_opt, metrics, save_img, save_as_dir, writer, noref_metrics, pixel_metrics, gpu_metrics):
        from PIL import Image
        n = 0
        for val_data in dataloader:
            img_name = os.path.splitext(os.path.basename(val_data['lq_path'][0]))[0]
            self.feed_data(val_data)
            self.test()
            # tensor2img (img_util.py:38-94) on the GPU: clamp / x255 / round-half-even in a HIP kernel; uint8 crosses PCIe only to be saved
            sr_u8 = imgproc.output_to_u8(self.output)
            if save_img:
                suffix = val_opt.get('suffix') or self.opt['name']
                save_img_path = os.path.join(self.opt['path']['visualization'], dataset_name, f'{img_name}_{suffix}.png')
                os.makedirs(os.path.dirname(save_img_path), exist_ok=True)
                if save_as_dir:
                    os.makedirs(save_as_dir, exist_ok=True)
                if writer is not None:
                    writer.submit(sr_u8, save_img_path)
                    if save_as_dir:
                        writer.submit(sr_u8, os.path.join(save_as_dir, f'{img_name}.png'))
                else:
                    sr_img = sr_u8.cpu().numpy()
                    Image.fromarray(sr_img, 'RGB').save(save_img_path)
                    if save_as_dir:
                        Image.fromarray(sr_img, 'RGB').save(os.path.join(save_as_dir, f'{img_name}.png'))
            for name, fn in noref_metrics.items():
                self.metric_results[name] += fn(sr_u8)
            if metrics and hasattr(self, 'gt'):
                gt_u8 = imgproc.output_to_u8(self.gt)
                for name, fn in pixel_metrics.items():
                    self.metric_results[name] += fn(sr_u8, gt_u8)
                if gpu_metrics:
                    # metric_data = [img2tensor(sr_img).unsqueeze(0) / 255, self.gt] (femasr_model.py:262), the /255 in a HIP kernel
                    sr = imgproc.u8_to_input(sr_u8)
                    for name, fn in gpu_metrics.items():
                        self.metric_results[name] += fn(sr, self.gt).item()
            del self.lq, self.output
            if hasattr(self, 'gt'):
                del self.gt
            n += 1
        return n

    def _gpu_metric(self, name, m):
        """The LPIPS or DISTS module of metric `name` (built once per model and option set)."""
        cache = self.__dict__.setdefault('_lpips_metrics', {})
        key = (name, m.get('type'), m.get('pretrained_model_path'), m.get('backbone_model_path'))
        if key not in cache:
            factory = dists_metric if m['type'] in dists_metric.METRIC_TYPES else lpips_metric
            cache[key] = factory.create_metric(m['type'], device=self.device, pretrained_model_path=m['pretrained_model_path'],
                                                    backbone_model_path=m.get('backbone_model_path'))
        return cache[key]

    def get_current_visuals(self):
        out = OrderedDict(lq=self.lq.detach().cpu(), result=self.output.detach().cpu())
        if hasattr(self, 'gt'):
            out['gt'] = self.gt.detach().cpu()
        return out

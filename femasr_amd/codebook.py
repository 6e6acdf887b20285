"""Codebook usage statistics of VQ index maps: what vis_codebook.py:20-83 of the reference does with `FeMaSRNet` as an encoder.

    idx = net.encode_indices(gt)                    # [(B,1,h,w) int64] - no decoder runs (FeMaSRNet.encode_indices)
    counts = usage(idx[0], n_e)                     # (n_e,) int64 on the indices' device
    perplexity(counts)                              # exp of the usage entropy: n_e when every code is used equally, 1 for one code
    maps = sample_index_maps(counts, 16, latent=8)  # vis_hrp's sampling, reproducible
    textures = net.decode_indices(torch.from_numpy(maps).cuda())

`usage` on a GPU tensor is one native call (csrc/codebook_stats.hip: per-block LDS counters, per-block partials, a fixed-order
reduction; exact); on a host tensor it is its definition in torch.bincount.  There is no other fallback: a GPU tensor without the
library raises.
"""
import ctypes

import numpy as np
import torch

from . import _lib


def _groups(indices, per_image):
    if not isinstance(indices, torch.Tensor):
        raise ValueError(f'usage: indices must be a torch tensor, got {type(indices).__name__}')
    if indices.dtype != torch.int64:
        raise ValueError(f'usage: indices must be int64 (what the network returns), got {indices.dtype}')
    if indices.numel() == 0 or (per_image and indices.dim() < 2):
        raise ValueError(f'usage: no tokens{" per image" if per_image else ""} in a tensor of shape {tuple(indices.shape)}')
    return indices.contiguous().reshape(indices.shape[0] if per_image else 1, -1)


def usage_host(idx, n_e):
    """The definition on a host (G, M) int64 tensor: (counts (G, n_e), invalid (G,)), int64.  An index outside [0, n_e) - compared as a
    64-bit integer - is counted in `invalid` and in no bin."""
    ok = (idx >= 0) & (idx < n_e)
    counts = torch.stack([torch.bincount(row[m], minlength=n_e) for row, m in zip(idx, ok)])
    return counts.to(torch.int64), (~ok).sum(dim=1).to(torch.int64)


def usage_counts(indices, n_e, per_image=False):
    """(counts, invalid) of `usage` without its range check: counts (n_e,) / (B, n_e) and invalid () / (B,), int64, on the indices' device."""
    n_e = int(n_e)
    if n_e < 1:
        raise ValueError(f'usage: n_e must be positive, got {n_e}')
    idx = _groups(indices, per_image)
    if idx.device.type == 'cuda':
        lib = _lib.load()
        g, m = idx.shape
        nbytes = ctypes.c_size_t()
        _lib.check(lib.femasr_index_histogram_workspace_bytes(g, m, n_e, ctypes.byref(nbytes)))
        with torch.cuda.device(idx.device):
            ws = torch.empty(max(int(nbytes.value), 4), dtype=torch.uint8, device=idx.device)
            counts = torch.empty((g, n_e), dtype=torch.int64, device=idx.device)
            invalid = torch.empty((g,), dtype=torch.int64, device=idx.device)
            stream = ctypes.c_void_p(torch.cuda.current_stream(idx.device).cuda_stream)
            _lib.check(lib.femasr_index_histogram(stream, _lib.ptr(idx), g, m, n_e, _lib.ptr(counts), _lib.ptr(invalid), _lib.ptr(ws), ws.numel()))
    else:
        counts, invalid = usage_host(idx, n_e)
    return (counts, invalid) if per_image else (counts[0], invalid[0])


def usage(indices, n_e, per_image=False):
    """How often each of the `n_e` codes occurs in an int64 index tensor of any shape: int64 (n_e,), or (B, n_e) - one row per entry of the
    first axis - with per_image=True, on the indices' device.  ValueError when an index lies outside [0, n_e) (checked on all 64 bits:
    2**32 + 5 is out of range, not code 5); that check reads one number back from the device."""
    counts, invalid = usage_counts(indices, n_e, per_image)
    bad = int(invalid.sum())
    if bad:
        raise ValueError(f'usage: {bad} of {indices.numel()} indices are outside [0, {int(n_e)})')
    return counts


def perplexity(counts):
    """exp(-sum p ln p) of the empirical code distribution p = counts / counts.sum(), in float64, with 0 ln 0 = 0: the effective number of
    codes in use.  (n_e,) -> float; (B, n_e) -> float64 array (B,).  All-zero counts give 1.0 (no token, no surprise)."""
    c = np.asarray(counts.detach().cpu() if isinstance(counts, torch.Tensor) else counts, dtype=np.float64)
    if c.ndim not in (1, 2) or c.shape[-1] < 1 or (c < 0).any():
        raise ValueError(f'perplexity: counts must be non-negative, (n_e,) or (B, n_e); got shape {c.shape}')
    tot = c.sum(axis=-1, keepdims=True)
    p = np.divide(c, tot, out=np.zeros_like(c), where=tot > 0)
    h = -(p * np.log(np.where(p > 0, p, 1.0))).sum(axis=-1)
    out = np.exp(h)
    return float(out) if c.ndim == 1 else out


def sample_index_maps(counts, n, latent=8, seed=0):
    """`n` index maps (n, 1, latent, latent), int64 numpy, drawn code by code from the empirical distribution counts / counts.sum() with
    numpy.random.default_rng(seed).choice: vis_codebook.py's vis_hrp sampling (np.random.choice over the class histogram), reproducible.
    Only codes with a non-zero count can appear."""
    c = np.asarray(counts.detach().cpu() if isinstance(counts, torch.Tensor) else counts, dtype=np.float64).reshape(-1)
    if c.size < 1 or (c < 0).any() or not c.sum() > 0:
        raise ValueError('sample_index_maps: counts must be non-negative with at least one token')
    if int(n) < 1 or int(latent) < 1:
        raise ValueError(f'sample_index_maps: n and latent must be positive, got {n}, {latent}')
    rng = np.random.default_rng(seed)
    return rng.choice(c.size, size=(int(n), 1, int(latent), int(latent)), p=c / c.sum()).astype(np.int64)

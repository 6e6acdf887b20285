"""DISTS restated from the published method (Ding et al., "Image Quality Assessment: Unifying Structure and Texture Similarity", as
packaged by DISTS_pytorch and pyiqa), in float64, by two routes that share only the backbone's convs:

  route 'torch'   the L2 pool as a grouped F.conv2d of f^2, the statistics with torch's mean
  route 'numpy'   the pool and the five moments as explicit numpy loops over the window taps / the pixels

plus the float32 restatement of the L2-pool kernel's arithmetic (l2pool_f32) and the statistics of given maps (score_from_maps, in the
two-pass form of the definition or the single-pass form of the kernel).  Maps are NCHW here unless a name says nhwc.
"""
import numpy as np
import torch
import torch.nn.functional as F

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
STAGES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))      # torchvision `features` indices of the convs of stage 1..5
CHANNELS = (3, 64, 128, 256, 512, 512)
C1 = C2 = 1e-6
HANN = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], np.float64) / 16.0     # a (x) a / sum with a = hanning(5)[1:-1] = (0.5, 1, 0.5)


def l2pool_torch(f):
    c = f.shape[1]
    g = torch.from_numpy(HANN).to(f.dtype)[None, None].repeat(c, 1, 1, 1)
    return torch.sqrt(F.conv2d(f * f, g, stride=2, padding=1, groups=c) + 1e-12)


def l2pool_numpy(f):
    """The same by a loop over the nine taps of every output pixel (zero padding: taps outside the map add nothing)."""
    a = f.numpy().astype(np.float64)
    b, c, h, w = a.shape
    hp, wp = (h + 1) // 2, (w + 1) // 2
    out = np.zeros((b, c, hp, wp), np.float64)
    for oy in range(hp):
        for ox in range(wp):
            for ky in range(3):
                for kx in range(3):
                    iy, ix = 2 * oy - 1 + ky, 2 * ox - 1 + kx
                    if 0 <= iy < h and 0 <= ix < w:
                        out[:, :, oy, ox] += HANN[ky, kx] * a[:, :, iy, ix] ** 2
    return torch.from_numpy(np.sqrt(out + 1e-12)).to(f.dtype)


def features(sd, x, dtype=torch.float64, pool=l2pool_torch):
    """The six maps of x ((B,3,H,W) array in [0,1]): the raw input, then the five stage outputs.  sd: canonical state dict (arrays)."""
    x = torch.as_tensor(np.asarray(x)).to(dtype)
    h = (x - torch.tensor(MEAN, dtype=dtype).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=dtype).view(1, 3, 1, 1)
    maps = [x]
    for k, idx in enumerate(STAGES):
        if k:
            h = pool(h)
        for i in idx:
            wt = torch.as_tensor(np.asarray(sd[f'stage{k + 1}.{i}.weight'])).to(dtype)
            bs = torch.as_tensor(np.asarray(sd[f'stage{k + 1}.{i}.bias'])).to(dtype)
            h = F.relu(F.conv2d(h, wt, bs, stride=1, padding=1))
        maps.append(h)
    return maps


def moments_torch(fx, fy):
    """(mx, my, vx, vy, cov), each (B,C) float64: the definition's two-pass form."""
    fx, fy = fx.to(torch.float64), fy.to(torch.float64)
    mx, my = fx.mean((2, 3)), fy.mean((2, 3))
    vx = ((fx - mx[:, :, None, None]) ** 2).mean((2, 3))
    vy = ((fy - my[:, :, None, None]) ** 2).mean((2, 3))
    cov = (fx * fy).mean((2, 3)) - mx * my
    return [t.numpy() for t in (mx, my, vx, vy, cov)]


def moments_numpy(fx, fy):
    """The same by a loop over the pixels."""
    ax, ay = np.asarray(fx, np.float64), np.asarray(fy, np.float64)
    b, c, h, w = ax.shape
    n = h * w
    mx, my, xy = np.zeros((b, c)), np.zeros((b, c)), np.zeros((b, c))
    for iy in range(h):
        for ix in range(w):
            mx += ax[:, :, iy, ix]
            my += ay[:, :, iy, ix]
            xy += ax[:, :, iy, ix] * ay[:, :, iy, ix]
    mx, my = mx / n, my / n
    vx, vy = np.zeros((b, c)), np.zeros((b, c))
    for iy in range(h):
        for ix in range(w):
            vx += (ax[:, :, iy, ix] - mx) ** 2
            vy += (ay[:, :, iy, ix] - my) ** 2
    return [mx, my, vx / n, vy / n, xy / n - mx * my]


def moments_single_pass(fx, fy):
    """v = E[x^2] - m^2, the form the kernel's five sums give."""
    ax, ay = np.asarray(fx, np.float64), np.asarray(fy, np.float64)
    mx, my = ax.mean((2, 3)), ay.mean((2, 3))
    return [mx, my, (ax * ax).mean((2, 3)) - mx * mx, (ay * ay).mean((2, 3)) - my * my, (ax * ay).mean((2, 3)) - mx * my]


def score_from_maps(maps_x, maps_y, alpha, beta, moments=moments_torch):
    """(score (B,), terms (B,6,2)) float64 from the six maps of either image.  terms[:, k] = (sum_c alpha S1, sum_c beta S2) of map k."""
    alpha, beta = np.asarray(alpha, np.float64).reshape(-1), np.asarray(beta, np.float64).reshape(-1)
    w = alpha.sum() + beta.sum()
    b = maps_x[0].shape[0]
    terms = np.zeros((b, 6, 2))
    off = 0
    for k, (fx, fy) in enumerate(zip(maps_x, maps_y)):
        c = fx.shape[1]
        mx, my, vx, vy, cov = moments(fx, fy)
        s1 = (2 * mx * my + C1) / (mx ** 2 + my ** 2 + C1)
        s2 = (2 * cov + C2) / (vx + vy + C2)
        terms[:, k, 0] = (alpha[off:off + c] * s1).sum(1)
        terms[:, k, 1] = (beta[off:off + c] * s2).sum(1)
        off += c
    return 1.0 - terms.sum((1, 2)) / w, terms


def dists(sd, x, y, dtype=torch.float64, route='torch'):
    """score (B,), terms (B,6,2).  dtype float32: features by stock torch in float32, statistics in float64."""
    pool, mom = (l2pool_torch, moments_torch) if route == 'torch' else (l2pool_numpy, moments_numpy)
    return score_from_maps(features(sd, x, dtype, pool), features(sd, y, dtype, pool), sd['alpha'], sd['beta'], mom)


# ---------------------------------------------------------------- float32 restatements of the kernels' arithmetic
def normalise_f32(x_nchw):
    """(v - mean) / std in float32 (IEEE subtract and divide), NCHW -> NHWC."""
    x = np.asarray(x_nchw, np.float32).transpose(0, 2, 3, 1)
    return ((x - np.array(MEAN, np.float32)) / np.array(STD, np.float32)).astype(np.float32)


def l2pool_f32(f_nhwc):
    """q = f * f rounded; acc = 0, then acc = fmaf(g[ky][kx], q, acc) for ky, kx ascending with the padded taps skipped; sqrtf(acc + 1e-12f).
    g is a power of two, so g * q is exact and a float64 sum of two float32 values rounded to float32 is the fmaf's single rounding."""
    f = np.asarray(f_nhwc, np.float32)
    b, h, w, c = f.shape
    hp, wp = (h + 1) // 2, (w + 1) // 2
    with np.errstate(over='ignore', invalid='ignore'):
        q = (f * f).astype(np.float32)
        acc = np.zeros((b, hp, wp, c), np.float32)
        for ky in range(3):
            oy = [o for o in range(hp) if 0 <= 2 * o - 1 + ky < h]
            for kx in range(3):
                ox = [o for o in range(wp) if 0 <= 2 * o - 1 + kx < w]
                if not oy or not ox:
                    continue
                iy, ix = [2 * o - 1 + ky for o in oy], [2 * o - 1 + kx for o in ox]
                tap = q[:, iy][:, :, ix].astype(np.float64) * HANN[ky, kx]
                sel = np.ix_(range(b), oy, ox, range(c))
                acc[sel] = (tap + acc[sel].astype(np.float64)).astype(np.float32)
        return np.sqrt((acc + np.float32(1e-12)).astype(np.float32)).astype(np.float32)

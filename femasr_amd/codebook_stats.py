#!/usr/bin/env python
"""Counterpart of the reference's vis_codebook.py: which codes of the codebook a set of images uses, per class, and what they look like.

    python -m femasr_amd.codebook_stats -i <dir> (-w <weights.pth> | --synthetic-seed N) [--lq-stage -s {2,4}] [--max-per-class N]
                                        [--samples K --latent L --seed S] [--reconstruct] -o <out>

<dir> holds images, or one sub-folder of images per class (the script's OutdoorSceneTrain layout).  Every image goes through the network
as an ENCODER only (FeMaSRNet.encode_indices: no decoder runs); the index maps are counted on the GPU (femasr_amd.codebook.usage).  Written:

    <out>/usage.npz             classes, images (classes,), n_e (codebooks,) and per codebook k: counts_k (classes, n_e) int64, tokens_k,
                                codes_used_k (classes,) int64, perplexity_k (classes,) float64
    <out>/usage.csv             class, codebook, n_e, images, tokens, codes_used, perplexity - one line per class and codebook
    <out>/textures/<class>.png  a grid (16 per row) of decode_indices on K maps of L x L codes drawn from the class histogram of the first
                                codebook (vis_hrp: np.random.choice over counts / sum(counts); here numpy.random.default_rng(S + class
                                number)), min-max normalised over the grid like torchvision's save_image(normalize=True)
    <out>/rec/<class>/<name>.png   with --reconstruct: the network's reconstruction of every image (reconstruct_ost)

What differs from the script: the network is the HQ net by default, as there, or an LQ net with --lq-stage; weights are never downloaded;
images are taken in sorted order (no shuffle), --max-per-class of them; an HQ net has no mirror pad, so an image is cropped at the bottom
and right to a multiple of 2**max_depth (logged once); PNG instead of JPEG; and there is no plotting dependency - the seaborn histogram
PDFs are left out, usage.npz holds the numbers they would show.
"""
import argparse
import csv
import os

import numpy as np
import torch

from . import codebook

IMG_EXT = ('.png', '.jpg', '.jpeg', '.bmp', '.tif', '.tiff', '.webp')


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('-i', '--input', type=str, required=True, help='folder of images, or of one sub-folder of images per class')
    ap.add_argument('-w', '--weight', type=str, default=None, help='path for model weights')
    ap.add_argument('--synthetic-seed', type=int, default=None, help='use deterministic synthetic weights (no checkpoint)')
    ap.add_argument('--lq-stage', action='store_true', help='the LQ (super-resolution) net of scale -s; default: the HQ net, as vis_codebook.py')
    ap.add_argument('-s', '--out_scale', type=int, default=4, choices=[2, 4], help='scale of the --lq-stage net')
    ap.add_argument('--max-per-class', type=int, default=None, metavar='N', help='at most N images per class (sorted order)')
    ap.add_argument('--samples', type=int, default=32, metavar='K', help='texture samples per class (vis_hrp: 32)')
    ap.add_argument('--latent', type=int, default=8, metavar='L', help='side of a sampled index map (vis_hrp: 8)')
    ap.add_argument('--seed', type=int, default=0, metavar='S', help='seed of the sampling')
    ap.add_argument('--reconstruct', action='store_true', help="also write the network's reconstruction of every image")
    ap.add_argument('-o', '--output', type=str, default='results/codebook_stats', help='Output folder')
    return ap


def _images(folder):
    return sorted(os.path.join(folder, f) for f in os.listdir(folder)
                  if not f.startswith('.') and f.lower().endswith(IMG_EXT) and os.path.isfile(os.path.join(folder, f)))


def list_classes(input_dir, max_per_class=None):
    """[(class name, [image paths])]: one class per sub-folder that holds images, in sorted order; a folder without such sub-folders is
    one class under its own name."""
    subs = sorted(d for d in os.listdir(input_dir) if not d.startswith('.') and os.path.isdir(os.path.join(input_dir, d)))
    classes = [(d, _images(os.path.join(input_dir, d))) for d in subs]
    classes = [(d, p) for d, p in classes if p]
    if not classes:
        classes = [(os.path.basename(os.path.normpath(input_dir)) or 'images', _images(input_dir))]
    if max_per_class is not None:
        classes = [(d, p[:max(0, int(max_per_class))]) for d, p in classes]
    if not any(p for _, p in classes):
        raise SystemExit(f'no images in {input_dir}')
    return classes


def _read(path, device):
    from PIL import Image
    with Image.open(path) as im:
        a = np.array(im.convert('RGB'))
    return torch.from_numpy(a).to(device).permute(2, 0, 1).unsqueeze(0).to(torch.float32) / 255.0


def _write_png(path, chw):
    """float (3,H,W) in [0,1] -> PNG, rounded as tensor2img does (x255, half to even)."""
    from PIL import Image
    u8 = (chw.detach().clamp(0, 1) * 255.0).round().to(torch.uint8).permute(1, 2, 0).cpu().numpy()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.ascontiguousarray(u8), 'RGB').save(path)


def class_usage(net, classes, read=_read, device='cuda', log=print, rec_dir=None):
    """Index maps of every image through `net.encode_indices`, counted per class.  Returns {'classes', 'images', 'n_e', 'counts': [per
    codebook (classes, n_e) int64 numpy]}.  HQ nets: `forward`'s geometry on the image cropped to a multiple of 2**max_depth; LQ nets:
    `test()`'s mirror pad.  `rec_dir`: also write the reconstructions (`forward` / `test`)."""
    lq = bool(net.LQ_stage)
    mult = 1 if lq else 2 ** int(net.max_depth)
    n_e = [int(cb[1]) for cb in net._cb]
    counts = [np.zeros((len(classes), n), np.int64) for n in n_e]
    images = np.zeros(len(classes), np.int64)
    told = False
    for ci, (name, paths) in enumerate(classes):
        for path in paths:
            x = read(path, device)
            h, w = x.shape[2] // mult * mult, x.shape[3] // mult * mult
            if h < 1 or w < 1:
                log(f'{path}: {x.shape[2]}x{x.shape[3]} is smaller than {mult}x{mult}: left out')
                continue
            if (h, w) != tuple(x.shape[2:]):
                if not told:
                    log(f'HQ net: images are cropped at the bottom and right to a multiple of {mult} (first: {path}, '
                        f'{x.shape[2]}x{x.shape[3]} -> {h}x{w})')
                    told = True
                x = x[:, :, :h, :w].contiguous()
            idx = net.encode_indices(x, pad=lq)
            for k, m in enumerate(idx):
                counts[k][ci] += codebook.usage(m, n_e[k]).cpu().numpy()
            images[ci] += 1
            if rec_dir is not None:
                rec = net.test(x) if lq else net(x)[0]
                _write_png(os.path.join(rec_dir, name, os.path.splitext(os.path.basename(path))[0] + '.png'), rec[0])
    return {'classes': [c for c, _ in classes], 'images': images, 'n_e': n_e, 'counts': counts}


def write_usage(out_dir, stats):
    """usage.npz and usage.csv (module docstring) from class_usage's result; returns the dict that went into the .npz."""
    os.makedirs(out_dir, exist_ok=True)
    names = stats['classes']
    z = {'classes': np.array(names, dtype=np.str_), 'images': np.asarray(stats['images'], np.int64), 'n_e': np.asarray(stats['n_e'], np.int64)}
    rows = []
    for k, c in enumerate(stats['counts']):
        c = np.asarray(c, np.int64)
        z[f'counts_{k}'] = c
        z[f'tokens_{k}'] = c.sum(axis=1)
        z[f'codes_used_{k}'] = (c > 0).sum(axis=1).astype(np.int64)
        z[f'perplexity_{k}'] = np.asarray(codebook.perplexity(c), np.float64).reshape(len(names))
        for ci, name in enumerate(names):
            rows.append([name, k, int(z['n_e'][k]), int(z['images'][ci]), int(z[f'tokens_{k}'][ci]), int(z[f'codes_used_{k}'][ci]),
                         f'{z[f"perplexity_{k}"][ci]:.6f}'])
    np.savez(os.path.join(out_dir, 'usage.npz'), **z)
    with open(os.path.join(out_dir, 'usage.csv'), 'w', newline='') as f:
        wr = csv.writer(f)
        wr.writerow(['class', 'codebook', 'n_e', 'images', 'tokens', 'codes_used', 'perplexity'])
        wr.writerows(rows)
    return z


def texture_grid(imgs, nrow=16, padding=2):
    """(n,3,h,w) float -> (3,H,W) in [0,1]: min-max normalised over the whole batch, tiled `nrow` per row with `padding` black pixels
    between and around the tiles - torchvision's save_image(normalize=True, nrow=16)."""
    lo, hi = float(imgs.min()), float(imgs.max())
    imgs = (imgs.clamp(lo, hi) - lo) / max(hi - lo, 1e-5)
    n, c, h, w = imgs.shape
    cols = min(nrow, n)
    rows = (n + cols - 1) // cols
    grid = imgs.new_zeros((c, rows * (h + padding) + padding, cols * (w + padding) + padding))
    for i in range(n):
        y, x = padding + (i // cols) * (h + padding), padding + (i % cols) * (w + padding)
        grid[:, y:y + h, x:x + w] = imgs[i]
    return grid


def write_textures(net, out_dir, stats, samples=32, latent=8, seed=0, device='cuda', log=print):
    """textures/<class>.png from the class histograms of the first codebook; a class without tokens is left out."""
    for ci, name in enumerate(stats['classes']):
        c = stats['counts'][0][ci]
        if c.sum() == 0:
            log(f'{name}: no tokens, no textures')
            continue
        maps = codebook.sample_index_maps(c, samples, latent, seed + ci)
        imgs = net.decode_indices(torch.from_numpy(maps).to(device))
        _write_png(os.path.join(out_dir, 'textures', name + '.png'), texture_grid(imgs.to(torch.float32)))


def main(argv=None):
    from femasr_amd import synth
    from femasr_amd.archs.femasr_arch import FeMaSRNet
    from femasr_amd.inference import load_weights

    args = build_parser().parse_args(argv)
    if args.samples < 1 or args.latent < 1:
        raise SystemExit(f'--samples and --latent must be positive, got {args.samples} and {args.latent}')
    if not torch.cuda.is_available():
        raise SystemExit('femasr_amd.codebook_stats needs a GPU (there is no CPU fallback)')
    dev = torch.device('cuda', torch.cuda.current_device())
    classes = list_classes(args.input, args.max_per_class)
    model = FeMaSRNet(codebook_params=[[32, 1024, 512]], LQ_stage=args.lq_stage, scale_factor=args.out_scale)
    if args.weight is not None:
        load_weights(model, args.weight)
    elif args.synthetic_seed is not None:
        w = synth.fill_state_dict(model.state_dict(), args.synthetic_seed, 'trained')
        model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    else:
        raise SystemExit('no network here: pass -w <weights.pth> or --synthetic-seed N')
    model = model.to(dev).eval()
    stats = class_usage(model, classes, device=dev, rec_dir=os.path.join(args.output, 'rec') if args.reconstruct else None)
    z = write_usage(args.output, stats)
    write_textures(model, args.output, stats, args.samples, args.latent, args.seed, dev)
    for ci, name in enumerate(stats['classes']):
        print(f'{name:20} images {int(z["images"][ci]):5d}  tokens {int(z["tokens_0"][ci]):9d}  codes used {int(z["codes_used_0"][ci]):5d} '
              f'of {int(z["n_e"][0])}  perplexity {z["perplexity_0"][ci]:.2f}')
    print(f'wrote {os.path.join(args.output, "usage.npz")}, usage.csv and textures/ for {len(stats["classes"])} class(es)')


if __name__ == '__main__':
    main()

#!/usr/bin/env python
"""DISTS of every restored image against its ground truth (the counterpart of lpips_folder.py for pyiqa's 'dists').

    python -m femasr_amd.dists_folder -r <restored_dir> -g <gt_dir> -w <dists weights> [--backbone <file>] [--suffix S]

Pairs files by name: for every file <base><ext> of the GT folder (sorted) the restored image is <base><suffix><ext>.  The PNGs are read
with PIL; the uint8 -> [0,1] conversion and the metric run on the GPU (femasr_amd.dists).  There is no network here to fetch weights:
-w names a local DISTS file (alpha and beta, optionally with the backbone), --backbone an optional separate VGG16 file (torchvision
`features.*`, DISTS `stageK.*` or lpips `net.slice*` names).
"""
import argparse
import glob
import os

import numpy as np
import torch


def pair_files(restored, gt, suffix=''):
    """[(base name, gt path, restored path)] for every file of the GT folder, sorted."""
    out = []
    for gt_path in sorted(glob.glob(os.path.join(gt, '*'))):
        basename, ext = os.path.splitext(os.path.basename(gt_path))
        out.append((basename, gt_path, os.path.join(restored, basename + suffix + ext)))
    return out


def score_folders(restored, gt, weights, backbone=None, suffix='', device='cuda', out=print):
    pairs = pair_files(restored, gt, suffix)
    if not pairs:
        raise SystemExit(f'no images in {gt}')
    from PIL import Image

    from femasr_amd import imgproc
    from femasr_amd.dists import DISTS
    metric = DISTS(pretrained_model_path=weights, backbone_model_path=backbone).to(device)
    vals = []
    for i, (basename, gt_path, res_path) in enumerate(pairs):
        imgs = []
        for p in (gt_path, res_path):
            u8 = np.ascontiguousarray(np.asarray(Image.open(p).convert('RGB'), dtype=np.uint8))
            imgs.append(imgproc.u8_to_input(torch.from_numpy(u8).to(device)))
        val = metric(imgs[1], imgs[0]).item()
        out(f'{i + 1:3d}: {basename:25}. \tDISTS: {val:.6f}.')
        vals.append(val)
    avg = sum(vals) / len(vals)
    out(f'Average: DISTS: {avg:.6f}')
    return vals, avg


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('-r', '--restored', required=True, help='folder of restored images')
    ap.add_argument('-g', '--gt', required=True, help='folder of ground-truth images')
    ap.add_argument('-w', '--weights', required=True, help='DISTS weight file (alpha, beta, optionally with the backbone)')
    ap.add_argument('--backbone', default=None, help='separate VGG16 backbone weight file')
    ap.add_argument('--suffix', default='', help='restored name = GT base name + suffix + extension')
    a = ap.parse_args(argv)
    score_folders(a.restored, a.gt, a.weights, a.backbone, a.suffix)


if __name__ == '__main__':
    main()

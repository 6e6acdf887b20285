#!/usr/bin/env python
"""Counterpart of the reference's scripts/metrics/calculate_lpips.py: LPIPS of every restored image against its ground truth.

    python -m femasr_amd.lpips_folder -r <restored_dir> -g <gt_dir> -w <lpips weights> [--net vgg|alex] [--backbone <file>] [--suffix S]

Pairs files by name: for every file <base><ext> of the GT folder (sorted) the restored image is <base><suffix><ext>.  The PNGs are read
with PIL; the uint8 -> [0,1] conversion and the metric run on the GPU (femasr_amd.lpips).  The default net is VGG16, as in that script.
There is no network here to fetch weights: -w names a local LPIPS file (heads, or heads and backbone), --backbone an optional separate
backbone file (torchvision `features.*` or lpips `net.slice*` names).
"""
import argparse
import glob
import os

import numpy as np
import torch


def score_folders(restored, gt, weights, net='vgg', backbone=None, suffix='', device='cuda', out=print):
    from PIL import Image

    from femasr_amd import imgproc
    from femasr_amd.lpips import LPIPS
    metric = LPIPS(net, pretrained_model_path=weights, backbone_model_path=backbone).to(device)
    vals = []
    for i, gt_path in enumerate(sorted(glob.glob(os.path.join(gt, '*')))):
        basename, ext = os.path.splitext(os.path.basename(gt_path))
        res_path = os.path.join(restored, basename + suffix + ext)
        imgs = []
        for p in (gt_path, res_path):
            u8 = np.ascontiguousarray(np.asarray(Image.open(p).convert('RGB'), dtype=np.uint8))
            imgs.append(imgproc.u8_to_input(torch.from_numpy(u8).to(device)))
        val = metric(imgs[1], imgs[0]).item()        # loss_fn_vgg(img_restored, img_gt)
        out(f'{i + 1:3d}: {basename:25}. \tLPIPS: {val:.6f}.')
        vals.append(val)
    if not vals:
        raise SystemExit(f'no images in {gt}')
    avg = sum(vals) / len(vals)
    out(f'Average: LPIPS: {avg:.6f}')
    return vals, avg


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('-r', '--restored', required=True, help='folder of restored images')
    ap.add_argument('-g', '--gt', required=True, help='folder of ground-truth images')
    ap.add_argument('-w', '--weights', required=True, help='LPIPS weight file (linK heads, optionally with the backbone)')
    ap.add_argument('--net', default='vgg', choices=('vgg', 'alex'))
    ap.add_argument('--backbone', default=None, help='separate backbone weight file')
    ap.add_argument('--suffix', default='', help='restored name = GT base name + suffix + extension')
    a = ap.parse_args(argv)
    score_folders(a.restored, a.gt, a.weights, a.net, a.backbone, a.suffix)


if __name__ == '__main__':
    main()

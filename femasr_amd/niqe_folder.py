#!/usr/bin/env python
"""Counterpart of the reference's scripts/metrics/calculate_niqe.py: the NIQE of every image in a folder (no ground truth needed).

    python -m femasr_amd.niqe_folder --input <dir> --params <niqe_pris_params.npz> [--crop_border N]

Listing and the printed lines are the script's: the folder is listed recursively and sorted, as `scandir(dir, recursive=True,
full_path=True)` does (files whose names start with '.' are left out), one line per image and the average.  What differs: --params names
the parameter file (BasicSR reads its own copy; none ships here and none is downloaded), images are read with PIL and converted to RGB,
and the arithmetic is calculate_niqe of femasr_amd.models.femasr_model computed on the GPU (femasr_amd.niqe), one image per call since
sizes differ.
"""
import argparse
import os

from .psnr_ssim_folder import scandir


def list_images(input_dir):
    """[(basename, path)] in the script's order."""
    return [(os.path.splitext(os.path.basename(p))[0], p) for p in sorted(scandir(input_dir))]


def score_folder(input_dir, params_path, crop_border=0, device='cuda', out=print):
    from femasr_amd.niqe import load_pris_params, niqe
    from femasr_amd.psnr_ssim_folder import _read_u8
    images = list_images(input_dir)
    if not images:
        raise SystemExit(f'no images in {input_dir}')
    params = load_pris_params(params_path)
    niqe_all = []
    for i, (basename, path) in enumerate(images):
        score = niqe(_read_u8(path, device), params, crop_border).item()
        out(f'{i + 1:3d}: {basename:25}. \tNIQE: {score:.6f}')
        niqe_all.append(score)
    out(input_dir)
    out(f'Average: NIQE: {sum(niqe_all) / len(niqe_all):.6f}')
    return niqe_all


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--input', type=str, default='datasets/val_set14/Set14', help='Input path')
    ap.add_argument('--crop_border', type=int, default=0, help='Crop border for each side')
    ap.add_argument('--params', type=str, required=True, help='NIQE parameter file (.npz: mu_pris_param, cov_pris_param, gaussian_window)')
    a = ap.parse_args(argv)
    score_folder(a.input, a.params, a.crop_border)


if __name__ == '__main__':
    main()

#!/usr/bin/env python
"""Counterpart of the reference's scripts/metrics/calculate_psnr_ssim.py: PSNR and SSIM of every restored image against its ground truth.

    python -m femasr_amd.psnr_ssim_folder --gt <gt_dir> --restored <restored_dir> [--crop_border N] [--suffix S] [--test_y_channel]

Listing, pairing and the printed lines are the script's.  Both folders are listed recursively and sorted, as `scandir(dir, recursive=True,
full_path=True)` does (files whose names start with '.' are left out).  With an empty --suffix the i-th restored file pairs with the i-th GT
file; with a suffix the restored image of a GT file <base><ext> (in any subfolder) is <restored>/<base><suffix><ext>.

What differs from the script: images are read with PIL and converted to RGB, and the arithmetic is the validation's - calculate_psnr /
calculate_ssim of femasr_amd.models.femasr_model, in fp64 on the uint8 values (Y = the fp64 BT.601 luma, not rounded) - computed on the GPU
(femasr_amd.psnr_ssim).  The script scores float32 copies instead (cv2's BGR image / 255. then * 255, its float32 bgr2ycbcr for the Y
channel), so its values can differ in the last printed digits.  --correct_mean_var is refused: it rewrites the restored image in float32
before scoring, which needs a float input path this tool does not have.
"""
import argparse
import os


def scandir(dir_path):
    """Files under dir_path, recursively, as full paths (basicsr.utils.scandir(..., recursive=True, full_path=True)): names starting with
    '.' are skipped, directories are entered."""
    for entry in os.scandir(dir_path):
        if entry.is_file():
            if not entry.name.startswith('.'):
                yield entry.path
        elif entry.is_dir():
            yield from scandir(entry.path)


def list_pairs(gt, restored, suffix=''):
    """[(basename, gt path, restored path)] in the script's order and pairing."""
    gt_files = sorted(scandir(gt))
    res_files = sorted(scandir(restored)) if suffix == '' else None
    if res_files is not None and len(res_files) < len(gt_files):
        raise SystemExit(f'{restored} holds {len(res_files)} files, {gt} {len(gt_files)}: with an empty --suffix they pair by index')
    pairs = []
    for i, gt_path in enumerate(gt_files):
        basename, ext = os.path.splitext(os.path.basename(gt_path))
        res_path = res_files[i] if suffix == '' else os.path.join(restored, basename + suffix + ext)
        pairs.append((basename, gt_path, res_path))
    return pairs


def _read_u8(path, device):
    import numpy as np
    import torch
    from PIL import Image
    return torch.from_numpy(np.array(Image.open(path).convert('RGB'), dtype=np.uint8)).to(device)


def score_folders(gt, restored, crop_border=0, suffix='', test_y_channel=False, device='cuda', out=print):
    from femasr_amd.psnr_ssim import psnr_ssim
    pairs = list_pairs(gt, restored, suffix)
    if not pairs:
        raise SystemExit(f'no images in {gt}')
    out('Testing Y channel.' if test_y_channel else 'Testing RGB channels.')
    psnr_all, ssim_all = [], []
    for i, (basename, gt_path, res_path) in enumerate(pairs):
        img_gt, img_restored = _read_u8(gt_path, device), _read_u8(res_path, device)
        if img_gt.shape != img_restored.shape:
            raise SystemExit(f'{gt_path} is {tuple(img_gt.shape)}, {res_path} is {tuple(img_restored.shape)}: the sizes must match')
        r = psnr_ssim(img_gt, img_restored, crop_border, test_y_channel)
        psnr, ssim = r.psnr.item(), r.ssim.item()
        out(f'{i + 1:3d}: {basename:25}. \tPSNR: {psnr:.6f} dB, \tSSIM: {ssim:.6f}')
        psnr_all.append(psnr)
        ssim_all.append(ssim)
    out(gt)
    out(restored)
    out(f'Average: PSNR: {sum(psnr_all) / len(psnr_all):.6f} dB, SSIM: {sum(ssim_all) / len(ssim_all):.6f}')
    return psnr_all, ssim_all


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--gt', type=str, default='datasets/val_set14/Set14', help='Path to gt (Ground-Truth)')
    ap.add_argument('--restored', type=str, default='results/Set14', help='Path to restored images')
    ap.add_argument('--crop_border', type=int, default=0, help='Crop border for each side')
    ap.add_argument('--suffix', type=str, default='', help='Suffix for restored images')
    ap.add_argument('--test_y_channel', action='store_true',
                    help='If True, test Y channel (In MatLab YCbCr format). If False, test RGB channels.')
    ap.add_argument('--correct_mean_var', action='store_true', help='not supported here (refused)')
    a = ap.parse_args(argv)
    if a.correct_mean_var:
        ap.error('--correct_mean_var is not supported: it rewrites the restored image in float32 before scoring, and this tool scores the '
                 'uint8 images (use the reference script for it)')
    score_folders(a.gt, a.restored, a.crop_border, a.suffix, a.test_y_channel)


if __name__ == '__main__':
    main()

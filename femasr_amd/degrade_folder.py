"""LQ folder from a GT folder on the GPU - the counterpart of the reference's generate_dataset.py (femasr_amd/degrade.py).

    python -m femasr_amd.degrade_folder -i GT_DIR -o LQ_DIR -s {2,4} [--mode bsrgan|bicubic] [--seed 123]
                                        [--recipes out.json | --recipes-in in.json] [--io-threads N] [--device cuda:0]

Sorted recursive listing as data.make_dataset does; every file is written under the same relative path below LQ_DIR.  A file's recipe is
degrade.sample_recipe(seed, relative path, h, w, scale, mode): it does not depend on the other files.  --recipes records every file's recipe
({relative path: recipe}), --recipes-in replays such a file: --seed is not used then, and a listed image without a recipe, or a recipe whose
scale or mode is not the one given with -s / --mode, ends the run before anything is written.  PNG output goes through pngio.PngWriter when
--io-threads is above 0 (the GPU row filters and the threaded deflate), through Pillow otherwise.  Other extensions always go through
Pillow's Image.save under the same name: a .jpg ground truth gives a .jpg LQ file, that is Pillow's default-quality JPEG coding ON TOP of the
synthesized degradation - keep ground truth as PNG (as the reference's datasets are) where the LQ pixels must be exactly degrade_u8's."""
import argparse
import json
import os
import sys

import numpy as np


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog='python -m femasr_amd.degrade_folder', description='Synthesize LQ images from a folder of GT images on the GPU.')
    p.add_argument('-i', '--input', required=True, help='folder of ground-truth images (searched recursively)')
    p.add_argument('-o', '--output', required=True, help='folder for the LQ images (the same relative paths)')
    p.add_argument('-s', '--scale', required=True, type=int, choices=(2, 4))
    p.add_argument('--mode', default='bsrgan', choices=('bsrgan', 'bicubic'))
    p.add_argument('--seed', type=int, default=123)
    p.add_argument('--recipes', default=None, help='write {relative path: recipe} of every file to this JSON file')
    p.add_argument('--recipes-in', default=None, help='replay the recipes of this JSON file instead of sampling')
    p.add_argument('--io-threads', type=int, default=0, help='above 0: PNG files through the fast writer with this many threads')
    p.add_argument('--device', default='cuda')
    args = p.parse_args(argv)
    if args.io_threads < 0:
        p.error('--io-threads must be 0 or more')
    return args


def main(argv=None):
    args = parse_args(argv)
    if not os.path.isdir(args.input):
        raise SystemExit(f'degrade_folder: {args.input} is not a directory')
    if os.path.abspath(args.input) == os.path.abspath(args.output):
        raise SystemExit('degrade_folder: the output folder must differ from the input folder')
    if args.recipes and args.recipes_in:
        raise SystemExit('degrade_folder: give --recipes or --recipes-in, not both')
    from .data import make_dataset
    paths = make_dataset(args.input)
    if not paths:
        raise SystemExit(f'degrade_folder: no images under {args.input}')
    replay = None
    if args.recipes_in:
        with open(args.recipes_in) as f:
            replay = json.load(f)
        for path in paths:
            rel = os.path.relpath(path, args.input)
            if rel not in replay:
                raise SystemExit(f'degrade_folder: {args.recipes_in} has no recipe for {rel}')
            for key, want in (('sf', args.scale), ('mode', args.mode)):
                if replay[rel].get(key) != want:
                    raise SystemExit(f"degrade_folder: the recipe of {rel} in {args.recipes_in} has {'scale' if key == 'sf' else 'mode'} "
                                     f"{replay[rel].get(key)!r}, the arguments ask for {want!r}")
    import torch
    from PIL import Image
    from . import degrade, pngio
    device = torch.device(args.device)
    writer = pngio.PngWriter(threads=args.io_threads) if args.io_threads > 0 else None
    used = {}
    try:
        for path in paths:
            rel = os.path.relpath(path, args.input)
            img = np.array(Image.open(path).convert('RGB'), dtype=np.uint8)
            if replay is not None:
                rec = degrade.Recipe.from_json(replay[rel])
            else:
                rec = degrade.sample_recipe(args.seed, rel, img.shape[0], img.shape[1], args.scale, args.mode)
            used[rel] = rec
            lq = degrade.degrade_u8(torch.from_numpy(img).to(device), rec)
            dst = os.path.join(args.output, rel)
            os.makedirs(os.path.dirname(dst) or '.', exist_ok=True)
            if writer is not None and dst.lower().endswith('.png'):
                writer.submit(lq, dst)
            else:
                Image.fromarray(lq.cpu().numpy(), 'RGB').save(dst)
    finally:
        if writer is not None:
            writer.close()
    if args.recipes:
        with open(args.recipes, 'w') as f:
            json.dump(used, f, sort_keys=True, indent=1)
    print(f'degrade_folder: {len(paths)} images, scale {args.scale}, mode {args.mode} -> {args.output}')
    return 0


if __name__ == '__main__':
    sys.exit(main())

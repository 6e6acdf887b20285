#!/usr/bin/env python
"""CLI counterpart of the reference's `inference_femasr.py` (lines 19-69) on the MI355X path.

Same flags (-i -w -o -s --suffix --max_size), same per-image policy (sorted glob; whole-image `test()` when
h*w < max_size**2, else `test_tile()`), same output naming.  Differences, all forced by the environment:
  * images are read/written with PIL (cv2 is not installed); channel order is handled explicitly, PNG is exact;
  * weights are never downloaded (no network): pass -w, or --synthetic-seed N for the deterministic generator;
  * pre/post-processing runs on the GPU (femasr_amd.imgproc) — uint8 crosses PCIe, not fp32;
  * with torchrun (WORLD_SIZE > 1) large images are tile-sharded over the ranks (femasr_amd.distributed).
"""
import argparse
import glob
import os

import numpy as np
import torch


def load_weights(model, path):
    """`torch.load(path)['params']` with strict=False like inference_femasr.py:40; `module.` prefixes stripped
    like basicsr/models/base_model.py:258-323."""
    sd = torch.load(path, map_location='cpu')
    for key in ('params', 'params_ema', 'state_dict'):
        if isinstance(sd, dict) and key in sd and isinstance(sd[key], dict):
            sd = sd[key]
            break
    sd = {(k[7:] if k.startswith('module.') else k): v for k, v in sd.items()}
    return model.load_state_dict(sd, strict=False)


def _final_scale(text):
    """--final-scale: the flag's text as an exact fraction ('3', '1.5', '1.1', '3/2')."""
    from fractions import Fraction
    try:
        f = Fraction(text)
    except (ValueError, ZeroDivisionError):
        raise argparse.ArgumentTypeError(f'expected a number such as 3, 1.5 or 3/2, got {text!r}') from None
    if f <= 0:
        raise argparse.ArgumentTypeError(f'expected a positive number, got {text!r}')
    return f


def _final_size(text):
    """--final-size: 'WxH' -> (W, H)."""
    import re
    m = re.fullmatch(r'([1-9][0-9]*)[xX]([1-9][0-9]*)', text.strip())
    if not m:
        raise argparse.ArgumentTypeError(f'expected WIDTHxHEIGHT in pixels such as 3840x2160, got {text!r}')
    return int(m.group(1)), int(m.group(2))


class _Half(argparse.Action):
    """--half: both half-precision modes at once (a later --linear-math / --decoder-math still overrides its side)."""

    def __call__(self, parser, namespace, values, option_string=None):
        namespace.linear_math = 'fp16'
        namespace.decoder_math = 'fp16'


def build_parser():
    ap = argparse.ArgumentParser(description='FeMaSR inference on MI355X')
    ap.add_argument('-i', '--input', type=str, default='inputs', help='Input image or folder')
    ap.add_argument('-w', '--weight', type=str, default=None, help='path for model weights')
    ap.add_argument('-o', '--output', type=str, default='results', help='Output folder')
    ap.add_argument('-s', '--out_scale', type=int, default=4, help='The final upsampling scale of the image')
    ap.add_argument('--suffix', type=str, default='', help='Suffix of the restored image')
    ap.add_argument('--max_size', type=int, default=600, help='Max image size for whole image inference, otherwise use tiled_test')
    ap.add_argument('--synthetic-seed', type=int, default=None, help='use deterministic synthetic weights (no checkpoint)')
    ap.add_argument('--tile_size', type=int, default=240)
    ap.add_argument('--tile_pad', type=int, default=16)
    ap.add_argument('--streams', type=int, default=3, help='sub-batch streams inside one batched forward of the tiled branch (3 measured fastest on MI355X)')
    ap.add_argument('--decoder-math', choices=['fp32', 'fp32_strict', 'fp32_direct', 'bf16x3', 'fp16'], default='fp32',
                    help="arithmetic of the convs behind the codebook lookup (FeMaSRNet.decoder_math); 'fp32_strict' is bit-identical to the CPU oracle; 'fp16' is the fast half-precision mode (same VQ indices, image ~5e-4 of its range off)")
    ap.add_argument('--linear-math', choices=['bf16_split', 'fp32', 'fp16'], default='bf16_split',
                    help="arithmetic of the layers in front of the codebook lookup (FeMaSRNet.linear_math); 'fp16' runs the Swin linears and the "
                         'stride-1 3x3 convs there in one fp16 pass: faster, but VQ indices may differ from the other modes (a nearly tied token can '
                         'flip and change the image locally by up to ~0.1 of its range)')
    ap.add_argument('--half', action=_Half, nargs=0, help='shorthand for --linear-math fp16 --decoder-math fp16: the whole network half-precision grade')
    ap.add_argument('--blend', action='store_true',
                    help='tiled branch: blend the overlapping tile halos instead of discarding them (no seams between tiles; NOT the '
                         "reference's arithmetic, off by default; needs 2 * tile_pad <= tile_size)")
    ap.add_argument('--color-fix', action='store_true',
                    help='wavelet colour fix of the result: detail from the network, everything coarser than ~2^N pixels from the bicubically '
                         "upsampled input (removes per-tile tone offsets and colour drift; NOT the reference's arithmetic, off by default)")
    ap.add_argument('--color-fix-levels', type=int, default=5, metavar='N', help='levels of --color-fix (1..12, default 5)')
    ap.add_argument('--self-ensemble', action='store_true',
                    help='x8 geometric self-ensemble: the network runs on the eight flips / transposes of the image (of every tile on the tiled '
                         "branch) and the eight results' bytes are averaged, at eight times the compute (NOT the reference's arithmetic, off by default)")
    ap.add_argument('--io-threads', type=int, default=0, metavar='N',
                    help='0 (default): decode, forward, Image.save one after the other, as ever.  N >= 1 (at most 16): the row filters of '
                         'PNG run on the GPU, N threads deflate and write behind the forward (femasr_amd.pngio: the same pixels, not the '
                         'same file bytes), one more thread decodes up to two inputs ahead')
    ap.add_argument('--png-level', type=int, default=6, metavar='0..9', help="deflate level of --io-threads N >= 1 (default 6, PIL's)")
    ap.add_argument('--jpeg-quality', type=int, default=None, metavar='1..100',
                    help="quality of the outputs named .jpg / .jpeg (default: unset - Image.save's own defaults, quality 75 with 4:2:0 chroma, "
                         'as ever).  With --io-threads N >= 1 such outputs take the fast JPEG path: colour, DCT and quantisation in one '
                         'launch on the GPU, Huffman coding in restart intervals on the N threads (femasr_amd.jpegio: a baseline JPEG of '
                         "its own definition, not libjpeg's bytes); with --io-threads 0 they go through Image.save(quality=, subsampling=)")
    ap.add_argument('--jpeg-subsampling', choices=['420', '444'], default=None,
                    help='chroma subsampling of --jpeg-quality (default 420; 444 keeps full-resolution chroma); refused without --jpeg-quality')
    ap.add_argument('--keep-format', action='store_true',
                    help="the output has the input's channels: a gray image (modes L, 1) comes back gray, gray + alpha (LA) and RGBA (also a "
                         'palette image with transparency) keep their alpha channel (femasr_amd.channels; off by default: every input is '
                         'converted to RGB and written as RGB)')
    ap.add_argument('--alpha', choices=['bicubic', 'network'], default='bicubic',
                    help="with --keep-format, how the alpha channel is upscaled: 'bicubic' (MATLAB bicubic, clipped and rounded) or 'network' "
                         '(the alpha plane takes the same forward as the colour, without the colour fix)')
    final = ap.add_mutually_exclusive_group()
    final.add_argument('--final-scale', type=_final_scale, default=None, metavar='F',
                       help="size of the written image as a multiple of the INPUT's size: 3, 1.5, 3/2, 1 (ceil of size times F, exact "
                            "arithmetic).  -s/--out_scale stays the NETWORK's factor (2 or 4, the weights decide); its result is resampled "
                            'once on the GPU, MATLAB bicubic with antialiasing, to the final size (femasr_amd.resample; each axis within '
                            "1/8 .. 8 of the network's result).  Off by default: the network's result is written as it is")
    final.add_argument('--final-size', type=_final_size, default=None, metavar='WxH',
                       help='the same with an exact size in pixels for every image, e.g. 3840x2160; the aspect ratio may change')
    return ap


def check_jpeg_flags(args):
    """--jpeg-quality / --jpeg-subsampling: a bad value ends the run before anything loads; args.jpeg_subsampling becomes '420' by default."""
    if args.jpeg_quality is None:
        if args.jpeg_subsampling is not None:
            raise SystemExit('--jpeg-subsampling needs --jpeg-quality')
        return
    if not 1 <= args.jpeg_quality <= 100:
        raise SystemExit(f'--jpeg-quality must be in 1..100, got {args.jpeg_quality}')
    if args.jpeg_subsampling is None:
        args.jpeg_subsampling = '420'


def _is_jpeg_name(name):
    return name.lower().endswith(('.jpg', '.jpeg'))


def _decode(path, keep_format=False):
    """uint8 (H,W,3) RGB.  keep_format: the file's own channels instead - (H,W) for modes L and 1, (H,W,2) for LA, (H,W,4) for RGBA and for
    a palette image with transparency; a palette image without, and every other mode (RGB, I;16, CMYK, ...): RGB as ever."""
    from PIL import Image
    im = Image.open(path)
    if keep_format:
        if im.mode in ('L', '1'):
            return np.array(im.convert('L'))
        if im.mode in ('LA', 'RGBA'):
            return np.array(im)
        if im.mode == 'P' and 'transparency' in im.info:
            return np.array(im.convert('RGBA'))
    return np.array(im.convert('RGB'))                                    # cv2.imread + BGR2RGB == RGB


def _decoded(paths, ahead, keep_format=False):
    """(path, image array) in order.  ahead = 0: decoded when asked for; else one thread decodes at most `ahead` images ahead."""
    if not ahead:
        for path in paths:
            yield path, _decode(path, keep_format)
        return
    import queue
    import threading
    q, stop = queue.Queue(maxsize=ahead), threading.Event()

    def put(item):
        while not stop.is_set():
            try:
                return q.put(item, timeout=0.1)
            except queue.Full:
                pass

    def reader():
        try:
            for path in paths:
                if stop.is_set():
                    return
                put((path, _decode(path, keep_format), None))
            put(None)
        except BaseException as e:
            put((None, None, e))

    th = threading.Thread(target=reader, name='decode-ahead', daemon=True)
    th.start()
    try:
        while True:
            item = q.get()
            if item is None:
                return
            if item[2] is not None:
                raise item[2]
            yield item[0], item[1]
    finally:
        stop.set()
        th.join()


def main(argv=None):
    from PIL import Image
    from femasr_amd import distributed as fd
    from femasr_amd import imgproc, synth
    from femasr_amd.archs.femasr_arch import FeMaSRNet

    args = build_parser().parse_args(argv)
    check_jpeg_flags(args)

    if not torch.cuda.is_available():
        raise SystemExit('femasr_amd.inference needs a GPU (there is no CPU fallback)')
    rank, world, local = fd.init_from_env()
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)

    model = FeMaSRNet(codebook_params=[[32, 1024, 512]], LQ_stage=True, scale_factor=args.out_scale)
    if args.weight is not None:
        load_weights(model, args.weight)
    elif args.synthetic_seed is not None:
        w = synth.fill_state_dict(model.state_dict(), args.synthetic_seed, 'trained')
        model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    else:
        raise SystemExit('no network here: pass -w <weights.pth> (FeMaSR_SRX4/SRX2_model_g.pth) or --synthetic-seed N')
    model.decoder_math = args.decoder_math
    model.linear_math = args.linear_math
    if args.io_threads < 0 or not 0 <= args.png_level <= 9:
        raise SystemExit(f'--io-threads must be >= 0 and --png-level in 0..9, got {args.io_threads} and {args.png_level}')
    if not 1 <= args.color_fix_levels <= 12:
        raise SystemExit(f'--color-fix-levels must be in 1..12, got {args.color_fix_levels}')
    model.color_fix_levels = args.color_fix_levels
    fix = {'color_fix': True} if args.color_fix else {}
    if args.self_ensemble:
        fix['self_ensemble'] = True
    model.num_streams = args.streams          # tiled images run as batched test() calls: sub-batches on internal streams (bit-identical for any split)
    model = model.to(dev).eval()

    if rank == 0:
        os.makedirs(args.output, exist_ok=True)
    paths = [args.input] if os.path.isfile(args.input) else sorted(glob.glob(os.path.join(args.input, '*')))
    writer = None
    if args.io_threads >= 1 and rank == 0:
        from femasr_amd import pngio
        writer = pngio.PngWriter(threads=min(args.io_threads, pngio.MAX_THREADS), level=args.png_level,
                                 **({} if args.jpeg_quality is None else {'jpeg_quality': args.jpeg_quality, 'jpeg_subsampling': args.jpeg_subsampling}))
    try:
        _run(args, model, paths, dev, rank, world, fix, writer, fd, Image)
    finally:
        if writer is not None:
            writer.close()
    if world > 1:
        torch.distributed.barrier()


def _run(args, model, paths, dev, rank, world, fix, writer, fd, Image):
    from femasr_amd import channels

    def forward(xu8, fix):
        """uint8 (H,W,3) -> uint8 (sH,sW,3); None on a rank that does not hold the result."""
        h, w = xu8.shape[:2]
        if h * w < args.max_size ** 2:
            # whole image: ONE native call, uint8 in -> uint8 out (decode fused into the pad kernel, tensor2img into the crop kernel)
            return model.test_u8(xu8, **fix) if rank == 0 else None
        # tiled: uint8 tiles in, uint8 tiles out - crops, the all-gather over xGMI and the paste move one byte per value, no fp32 image
        # or canvas is ever held (FeMaSRNet.test_tile_u8); with several ranks only rank 0 pastes
        if world > 1:
            return fd.test_tile_parallel(model, xu8, args.tile_size, args.tile_pad, root_only=True, blend=args.blend, **fix)
        return model.test_tile_u8(xu8, args.tile_size, args.tile_pad, blend=args.blend, **fix)

    plain = {k: v for k, v in fix.items() if k != 'color_fix'}              # the alpha plane's forward: everything but the colour fix
    resample = None
    if args.final_scale is not None or args.final_size is not None:
        from femasr_amd import resample                                     # (--final-scale / --final-size: imported only with them)
    for path, img in _decoded(paths, 2 if args.io_threads >= 1 else 0, args.keep_format):
        img_name = os.path.basename(path)
        xu8 = torch.from_numpy(img).to(dev)
        final = None                                                        # (out_h, out_w) where it is not the network's own size
        if resample is not None:
            h, w = img.shape[:2]
            final = resample.target_size(h, w, args.out_scale, args.final_scale, args.final_size)
            if final == (args.out_scale * h, args.out_scale * w):
                final = None
            else:
                try:                                                        # refused before the forward runs
                    resample.prepare(args.out_scale * h, args.out_scale * w, final[0], final[1], dev)
                except (resample.ResampleRatio, resample.ResampleTooSmall) as e:
                    raise SystemExit(f"{path}: the network's {args.out_scale * w}x{args.out_scale * h} result cannot be resampled to "
                                     f'{final[1]}x{final[0]} ({e})')
        if args.keep_format:
            # the input's channels (femasr_amd.channels): split -> the same forward -> merge; an RGB image is forward(xu8) itself
            try:
                u8 = channels.upscale_u8(xu8, lambda x: forward(x, fix), args.out_scale, alpha=args.alpha, run_alpha=lambda x: forward(x, plain))
            except channels.AlphaTooSmall as e:
                raise SystemExit(f'{path}: {img.shape[0]}x{img.shape[1]} is too small for the bicubic upscale of its alpha channel ({e}): '
                                 'pass --alpha network')
        else:
            u8 = forward(xu8, fix)
        if final is not None and u8 is not None:
            # once, on the final bytes of the rank that holds them: behind blend, colour fix, self-ensemble and the alpha merge
            u8 = resample.resample_u8(u8, final[0], final[1])
        if writer is not None:
            writer.submit(u8, os.path.join(args.output, img_name))
        elif rank == 0:
            # (--jpeg-quality without a writer: PIL's encoder at the same settings; its subsampling 0 is 4:4:4, 2 is 4:2:0)
            how = ({'quality': args.jpeg_quality, 'subsampling': 0 if args.jpeg_subsampling == '444' else 2}
                   if args.jpeg_quality is not None and _is_jpeg_name(img_name) else {})
            Image.fromarray(u8.cpu().numpy(), channels.MODES[u8.shape[2] if u8.dim() == 3 else 1]).save(os.path.join(args.output, img_name), **how)


if __name__ == '__main__':
    main()

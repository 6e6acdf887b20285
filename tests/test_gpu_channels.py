"""-m gpu: gray / gray + alpha / RGBA through inference on the device (csrc/channels.hip, the pixel-size template of csrc/png_filter.hip,
femasr_amd/channels.py).

Integer work and one fp64 sum in the definition's order: everything is compared BIT FOR BIT with the numpy definitions (held to Pillow in
test_channels_host.py); no tolerance appears in this module.  The C entries run on the guard arenas of tests/guard_arena.py - every operand
at its exact size between poison, once per poison: no byte outside the outputs may change and the outputs may not depend on the poison."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import guard_arena as GA
import gpu_utils as G
from femasr_amd import _lib, channels as CH, inference, pngio, synth
from femasr_amd.models.femasr_model import imresize, imresize_tables
from helpers import synth_weights

pytestmark = pytest.mark.gpu

# (H, W) of the input.  2 is the smallest length imresize_tables accepts at s = 2 and 4 (asserted below); (5,7), (9,33), (64,3): odd, H != W,
# rows that start off a dword at s = 2; (2,515): 1030 / 2060 output pixels per row, i.e. two and three blocks of 1024 in a row
SHAPES = [(2, 2), (5, 7), (9, 33), (64, 3), (2, 515)]
SCALES = (2, 4)


def _same(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = np.argwhere(got != ref)
    assert bad.size == 0, f'{what}: {len(bad)} of {got.size} bytes differ, the first at {bad[0].tolist()}'


def _raw(what, inputs, outs, call):
    """One library call on exact-size regions under both poisons: inputs {name: array}, outs {name: shape} (uint8); call(lib, ops)."""
    lib = _lib.load()

    def go():
        ops = G.Operands(what)
        for n, a in inputs.items():
            ops.inp(n, a)
        for n, shp in outs.items():
            ops.out(n, int(np.prod(shp)))
        ops.build()
        _lib.check(call(lib, ops))
        ops.check()
        return {n: ops.get(n, torch.uint8, shp).cpu().numpy() for n, shp in outs.items()}
    return GA.run_twice(go, what)


def _alpha(kind, shape, seed):
    if kind == 'random':
        return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
    if kind == 'board':                                    # 0 / 255 checkerboard: the bicubic overshoots, the clip decides the byte
        return ((np.add.outer(np.arange(shape[0]), np.arange(shape[1])) & 1) * 255).astype(np.uint8)
    return np.full(shape, 255, np.uint8)


def _tables(h, w, s):
    wh, ih = imresize_tables(h, h * s, s)
    ww, iw = imresize_tables(w, w * s, s)
    return dict(wh=wh, ih=ih, ww=ww, iw=iw), wh.shape[1], ww.shape[1]


def test_smallest_shape_is_the_tables_smallest():
    for s in SCALES:
        with pytest.raises(ValueError):
            imresize_tables(1, s, s)
        imresize_tables(2, 2 * s, s)


# ------------------------------------------------------------------------------------------------ the C entries on guard arenas
@pytest.mark.parametrize('hw', SHAPES, ids=lambda v: f'{v[0]}x{v[1]}')
def test_split_and_gray_entries(cuda_device, hw):
    H, W = hw
    rng = np.random.default_rng(H * 1000 + W)
    for C in (1, 2, 4):
        img = rng.integers(0, 256, (2, H, W, C), dtype=np.uint8)
        outs = {'rgb': (2, H, W, 3)}
        if C != 1:
            outs['alpha'] = (2, H, W)
        got = _raw(f'channels_split_u8 C={C}', {'img': img}, outs,
                   lambda lib, o: lib.femasr_channels_split_u8(None, o.p('img'), 2, H, W, C, o.p('rgb'), o.p('alpha')))
        for b in range(2):
            rgb, a = CH.split_ref(img[b])
            _same(got['rgb'][b], rgb, f'split C={C} rgb')
            if C != 1:
                _same(got['alpha'][b], a, f'split C={C} alpha')
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    got = _raw('channels_merge_u8 gray', {'rgb': rgb}, {'o': (H, W)},
               lambda lib, o: lib.femasr_channels_merge_u8(None, o.p('rgb'), None, None, H, W, 1, 1, None, None, 0, None, None, 0, o.p('o')))
    _same(got['o'], CH.gray_ref(rgb), 'gray')


@pytest.mark.parametrize('s', SCALES)
@pytest.mark.parametrize('hw', SHAPES, ids=lambda v: f'{v[0]}x{v[1]}')
def test_merge_entry(cuda_device, hw, s):
    H, W = hw
    sH, sW = s * H, s * W
    rng = np.random.default_rng(H * 1000 + W + s)
    rgb = rng.integers(0, 256, (sH, sW, 3), dtype=np.uint8)
    tabs, ph, pw = _tables(H, W, s)
    for kind in ('random', 'board', 'const'):
        a = _alpha(kind, (H, W), 7)
        a_sr = CH.alpha_up_ref(a, s)
        if kind == 'board':
            assert imresize(a.astype(np.float64), s).min() < -1 and a_sr.min() == 0          # the clip decides bytes of this case
        if kind == 'const':
            assert (a_sr == 255).all()
        got = _raw(f'channels_merge_u8 alpha only s={s} {kind}', dict(a=a, **tabs), {'o': (sH, sW)},
                   lambda lib, o: lib.femasr_channels_merge_u8(None, None, o.p('a'), None, H, W, s, 1, o.p('wh'), o.p('ih'), ph, o.p('ww'), o.p('iw'),
                                                               pw, o.p('o')))
        _same(got['o'], a_sr, f'alpha_bicubic {kind}')
        for ch in (2, 4):
            got = _raw(f'channels_merge_u8 bicubic s={s} ch={ch} {kind}', dict(rgb=rgb, a=a, **tabs), {'o': (sH, sW, ch)},
                       lambda lib, o: lib.femasr_channels_merge_u8(None, o.p('rgb'), o.p('a'), None, H, W, s, ch, o.p('wh'), o.p('ih'), ph,
                                                                   o.p('ww'), o.p('iw'), pw, o.p('o')))
            _same(got['o'], CH.merge_ref(rgb, a_sr, ch), f'merge bicubic ch={ch} {kind}')
    net_a = rng.integers(0, 256, (sH, sW, 3), dtype=np.uint8)                              # what a network makes of (a, a, a): any RGB image
    for ch in (2, 4):
        got = _raw(f'channels_merge_u8 network s={s} ch={ch}', dict(rgb=rgb, n=net_a), {'o': (sH, sW, ch)},
                   lambda lib, o: lib.femasr_channels_merge_u8(None, o.p('rgb'), None, o.p('n'), H, W, s, ch, None, None, 0, None, None, 0, o.p('o')))
        _same(got['o'], CH.merge_ref(rgb, CH.gray_ref(net_a), ch), f'merge network ch={ch}')


# ------------------------------------------------------------------------------------------------ the Python wrappers
def test_wrappers(cuda_device):
    rng = np.random.default_rng(3)
    dev = cuda_device
    for H, W in ((5, 7), (9, 33)):
        for C in (1, 2, 4):
            img = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
            view = torch.from_numpy(np.ascontiguousarray(img.transpose(1, 0, 2))).to(dev).transpose(0, 1)      # not contiguous
            assert not view.is_contiguous()
            rgb, a = CH.split_u8(view)
            rr, ar = CH.split_ref(img)
            _same(rgb.cpu().numpy(), rr, 'split_u8')
            assert (a is None) == (ar is None)
            if a is not None:
                _same(a.cpu().numpy(), ar, 'split_u8 alpha')
        gray = rng.integers(0, 256, (H, W), dtype=np.uint8)
        _same(CH.split_u8(torch.from_numpy(gray).to(dev))[0].cpu().numpy(), CH.split_ref(gray)[0], 'split_u8 (H,W)')
        batch = rng.integers(0, 256, (2, H, W, 4), dtype=np.uint8)
        rgb, a = CH.split_u8(torch.from_numpy(batch).to(dev))
        _same(rgb.cpu().numpy(), batch[..., :3], 'split_u8 batch')
        _same(a.cpu().numpy(), batch[..., 3], 'split_u8 batch alpha')
        # a buffer that starts one byte off a dword: the byte-wise paths of the kernels
        odd = torch.from_numpy(rng.integers(0, 256, 1 + H * W * 4, dtype=np.uint8)).to(dev)[1:].view(H, W, 4)
        rgb, a = CH.split_u8(odd)
        _same(rgb.cpu().numpy(), odd.cpu().numpy()[..., :3], 'split_u8 off a dword')
        _same(a.cpu().numpy(), odd.cpu().numpy()[..., 3], 'split_u8 off a dword, alpha')
        for s in SCALES:
            sr = rng.integers(0, 256, (s * W, s * H, 3), dtype=np.uint8)
            srv = torch.from_numpy(sr).to(dev).transpose(0, 1)                             # (sH,sW,3), not contiguous
            srn = np.ascontiguousarray(sr.transpose(1, 0, 2))
            _same(CH.gray_u8(srv).cpu().numpy(), CH.gray_ref(srn), 'gray_u8')
            al = rng.integers(0, 256, (W, H), dtype=np.uint8)
            alv, aln = torch.from_numpy(al).to(dev).t(), np.ascontiguousarray(al.T)
            up = CH.alpha_up_ref(aln, s)
            _same(CH.alpha_bicubic_u8(alv, s).cpu().numpy(), up, 'alpha_bicubic_u8')
            na = rng.integers(0, 256, (s * H, s * W, 3), dtype=np.uint8)
            for ch in (2, 4):
                _same(CH.merge_u8(srv, alv, ch, s).cpu().numpy(), CH.merge_ref(srn, up, ch), f'merge_u8 bicubic {ch}')
                _same(CH.merge_u8(srv, torch.from_numpy(na).to(dev), ch).cpu().numpy(), CH.merge_ref(srn, CH.gray_ref(na), ch), f'merge_u8 network {ch}')
            _same(CH.merge_u8(srv, None, 1).cpu().numpy(), CH.gray_ref(srn), 'merge_u8 gray')
            assert CH.merge_u8(srv, None, 3) is srv
            out = torch.empty((s * H, s * W, 4), dtype=torch.uint8, device=dev)
            assert CH.merge_u8(srv, alv, 4, s, out=out).data_ptr() == out.data_ptr()
    x = torch.zeros((4, 4, 3), dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.FemasrError):
        CH.gray_u8(x.cpu())
    with pytest.raises(_lib.FemasrError):
        CH.split_u8(x.cpu()[..., :2])
    for bad in (lambda: CH.gray_u8(x.float()), lambda: CH.gray_u8(x[..., :2]), lambda: CH.split_u8(x), lambda: CH.split_u8(x[:0, :, :1]),
                lambda: CH.merge_u8(x, None, 4), lambda: CH.merge_u8(x, x[..., 0], 1), lambda: CH.merge_u8(x, x[:2, :2, 0], 4, 4),
                lambda: CH.merge_u8(x, x[..., 0], 4, 2), lambda: CH.alpha_bicubic_u8(x[:1, :, 0], 2), lambda: CH.alpha_bicubic_u8(x[..., 0], 0),
                lambda: CH.merge_u8(x, x[..., 0], 4, 1, out=x)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        CH.gray_u8(np.zeros((4, 4, 3), np.uint8))


# ------------------------------------------------------------------------------------------------ PNG filters for 1, 2 and 4 bytes per pixel
def _smooth(shape, seed):
    steps = np.random.default_rng(seed).integers(-3, 4, shape)
    return np.clip(128 + np.cumsum(steps, axis=-2) + np.cumsum(steps, axis=-3), 0, 255).astype(np.uint8)      # image-like: the filters compete


@pytest.mark.parametrize('C', [1, 2, 4])
def test_filter_entry(cuda_device, C):
    """Both sides of the one-wave limit (C W = 3072 bytes and one pixel more), small odd sizes, and B = 2 with H = 2: the first row of the
    second image has no row above."""
    for B, H, W in ((1, 3, 3072 // C), (1, 3, 3072 // C + 1), (2, 2, 5), (1, 7, 17), (2, 2, 3072 // C + 1)):
        img = _smooth((B, H, W, C), 10 * C + W % 7)
        for f in (5, 4):
            got = _raw(f'png_filter_u8 C={C} {B}x{H}x{W} f={f}', {'img': img}, {'o': (B, H, 1 + C * W)},
                       lambda lib, o: lib.femasr_png_filter_u8(None, o.p('img'), B, H, W, C, f, o.p('o')))['o']
            for b in range(B):
                x = img[b, ..., 0] if C == 1 else img[b]
                _same(got[b], pngio.filter_image(x, 'adaptive' if f == 5 else f), f'C={C} {B}x{H}x{W} filter {f} image {b}')


def test_filter_past_the_resident_row_and_rgb_unchanged(cuda_device):
    """C = 4, W = 6145: one pixel past PF_BLOCK_ROW = 24576 bytes, the row goes through LDS in two segments.  And the RGB entry, now the
    C = 3 instantiation: its bytes are those of filter_rows, through either entry."""
    img = _smooth((1, 3, 6145, 4), 2)
    for f in (5, 4):
        got = _raw(f'png_filter_u8 segments f={f}', {'img': img}, {'o': (1, 3, 1 + 4 * 6145)},
                   lambda lib, o: lib.femasr_png_filter_u8(None, o.p('img'), 1, 3, 6145, 4, f, o.p('o')))['o']
        _same(got[0], pngio.filter_image(img[0], 'adaptive' if f == 5 else f), f'segments, filter {f}')
    for H, W in ((7, 17), (3, 1025)):
        rgb = _smooth((H, W, 3), 3)
        t = torch.from_numpy(rgb).to(cuda_device)
        for f in ('adaptive', 'paeth', 'sub'):
            want = pngio.filter_rows(rgb, f)
            _same(pngio.filter_rows_gpu(t, f).cpu().numpy(), want, f'filter_rows_gpu {f}')
            _same(pngio.filter_image_gpu(t, f).cpu().numpy(), want, f'filter_image_gpu C=3 {f}')
    for C in (1, 2, 4):                                    # the wrapper: (H,W), (H,W,C), a batch, a view, out=
        x = _smooth((2, 9, 21, C), C)
        t = torch.from_numpy(x).to(cuda_device)
        got = pngio.filter_image_gpu(t).cpu().numpy()
        for b in range(2):
            _same(got[b], pngio.filter_image(x[b, ..., 0] if C == 1 else x[b]), f'filter_image_gpu batch C={C}')
        view = torch.from_numpy(np.ascontiguousarray(x[0].transpose(1, 0, 2))).to(cuda_device).transpose(0, 1)
        _same(pngio.filter_image_gpu(view, 'paeth').cpu().numpy(), pngio.filter_image(x[0], 'paeth'), f'filter_image_gpu view C={C}')
    g = torch.from_numpy(x[0, ..., 0].copy()).to(cuda_device)
    out = torch.empty((9, 22), dtype=torch.uint8, device=cuda_device)
    assert pngio.filter_image_gpu(g, out=out).data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), pngio.filter_image(x[0, ..., 0]))
    for bad in (g.cpu(), g.float(), g[:0], torch.zeros(2, 2, 5, dtype=torch.uint8, device=cuda_device)):
        with pytest.raises(ValueError):
            pngio.filter_image_gpu(bad)


# ------------------------------------------------------------------------------------------------ the driver
_NETS = {}


def _net(cn, dev):
    if cn not in _NETS:
        _NETS[cn] = G.build_net(cn, synth_weights(cn, 5, 'trained'), dev, decoder_math='fp32')
    return _NETS[cn]


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize('cn,s,hw', [('x4', 4, (24, 20)), ('x2', 2, (40, 36))])
def test_upscale_u8(cuda_device, cn, s, hw):
    net, dev = _net(cn, cuda_device), cuda_device
    H, W = hw
    rgba = np.random.default_rng(s).integers(0, 256, (H, W, 4), dtype=np.uint8)
    rgba[..., 3] = _alpha('board', (H, W), 0)
    rgba[: H // 2, :, 3] = np.random.default_rng(s + 1).integers(0, 256, (H // 2, W), dtype=np.uint8)
    la = np.ascontiguousarray(rgba[..., 2:])
    tile = H // 2
    whole = lambda x: net.test_u8(x)
    runs = {'whole': whole, 'tiles': lambda x: net.test_tile_u8(x, tile, 2), 'blend': lambda x: net.test_tile_u8(x, tile, 2, blend=True)}
    stack = lambda p: torch.from_numpy(np.repeat(p[..., None], 3, axis=2)).to(dev)
    assert H >= 2 * tile and W > tile                      # at least 2 x 2 tiles
    for name, run in runs.items():
        col = _np(run(torch.from_numpy(np.ascontiguousarray(rgba[..., :3])).to(dev)))
        assert col.shape == (s * H, s * W, 3)
        gra = CH.gray_ref(_np(run(stack(la[..., 0]))))
        a_net = CH.gray_ref(_np(run(stack(rgba[..., 3]))))
        a_bic = CH.alpha_up_ref(rgba[..., 3], s)
        for mode, a_sr in (('bicubic', a_bic), ('network', a_net)):
            out = _np(CH.upscale_u8(torch.from_numpy(rgba).to(dev), run, s, alpha=mode))
            assert out.shape == (s * H, s * W, 4)
            _same(out[..., :3], col, f'{name} {mode}: colour')
            _same(out[..., 3], a_sr, f'{name} {mode}: alpha')
            out = _np(CH.upscale_u8(torch.from_numpy(la).to(dev), run, s, alpha=mode))
            _same(out, np.stack([gra, a_sr], axis=2), f'{name} {mode}: gray + alpha')
        _same(_np(CH.upscale_u8(torch.from_numpy(la[..., 0].copy()).to(dev), run, s)), gra, f'{name}: gray')
    # the driver is its definition with the same `run`
    host_run = lambda a: _np(whole(torch.from_numpy(np.ascontiguousarray(a)).to(dev)))
    for mode in CH.ALPHA_MODES:
        _same(_np(CH.upscale_u8(torch.from_numpy(rgba).to(dev), whole, s, alpha=mode)), CH.upscale_ref(rgba, host_run, s, mode), f'upscale_ref {mode}')
    # the alpha pass may take another forward (the CLI: no colour fix); a 3-channel image is run(img) itself
    calls = []
    other = lambda x: calls.append('alpha') or whole(x)
    out = _np(CH.upscale_u8(torch.from_numpy(rgba).to(dev), lambda x: calls.append('colour') or net.test_u8(x, color_fix=True), s, alpha='network',
                            run_alpha=other))
    assert sorted(calls) == ['alpha', 'colour']
    _same(out[..., 3], CH.gray_ref(_np(whole(stack(rgba[..., 3])))), 'alpha pass without the colour fix')
    _same(out[..., :3], _np(net.test_u8(torch.from_numpy(np.ascontiguousarray(rgba[..., :3])).to(dev), color_fix=True)), 'colour pass with it')
    x3 = torch.from_numpy(np.ascontiguousarray(rgba[..., :3])).to(dev)
    seen = []

    def once(x):
        seen.append(x)
        return whole(x)
    res = CH.upscale_u8(x3, once, s)
    assert len(seen) == 1 and seen[0] is x3 and np.array_equal(_np(res), _np(whole(x3)))
    assert CH.upscale_u8(x3, lambda x: None, s) is None and CH.upscale_u8(torch.from_numpy(rgba).to(dev), lambda x: None, s) is None
    with pytest.raises(ValueError):
        CH.upscale_u8(torch.from_numpy(rgba).to(dev), whole, s + 1)
    with pytest.raises(ValueError):
        CH.upscale_u8(torch.from_numpy(rgba).to(dev), whole, s, alpha='nearest')


# ------------------------------------------------------------------------------------------------ the command line
SEED = 3
_CLI = {}


def _cli_net(dev):
    """The network inference.main builds for --synthetic-seed SEED."""
    if 'net' not in _CLI:
        from femasr_amd.archs.femasr_arch import FeMaSRNet
        model = FeMaSRNet(codebook_params=[[32, 1024, 512]], LQ_stage=True, scale_factor=4)
        w = synth.fill_state_dict(model.state_dict(), SEED, 'trained')
        model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
        _CLI['net'] = model.to(dev).eval()
    return _CLI['net']


def _cli_inputs(folder):
    rng = np.random.default_rng(12)
    rgba = rng.integers(0, 256, (12, 16, 4), dtype=np.uint8)
    rgba[:, ::2, 3] = 0
    imgs = {'a_rgba.png': rgba, 'b_la.png': rng.integers(0, 256, (9, 13, 2), dtype=np.uint8), 'c_l.png': rng.integers(0, 256, (8, 11), dtype=np.uint8)}
    folder.mkdir()
    for name, a in imgs.items():
        Image.fromarray(a, CH.MODES[1 if a.ndim == 2 else a.shape[2]]).save(str(folder / name))
    return imgs


@pytest.mark.parametrize('alpha', CH.ALPHA_MODES)
@pytest.mark.parametrize('threads', [0, 2])
def test_cli_keep_format(cuda_device, tmp_path, threads, alpha):
    imgs = _cli_inputs(tmp_path / 'in')
    out = tmp_path / 'out'
    inference.main(['-i', str(tmp_path / 'in'), '-o', str(out), '--synthetic-seed', str(SEED), '--keep-format', '--alpha', alpha,
                    '--io-threads', str(threads)])
    net = _cli_net(cuda_device)
    assert sorted(p.name for p in out.iterdir()) == sorted(imgs)
    for name, a in imgs.items():
        want = _np(CH.upscale_u8(torch.from_numpy(a).to(cuda_device), net.test_u8, 4, alpha=alpha))
        with Image.open(str(out / name)) as im:
            assert im.mode == CH.MODES[1 if a.ndim == 2 else a.shape[2]] and im.size == (4 * a.shape[1], 4 * a.shape[0]), (name, im.mode, im.size)
            _same(np.array(im), want, name)
    assert not np.array_equal(np.array(Image.open(str(out / 'a_rgba.png')))[..., 3], 255)      # the alpha channel is the image's, not opaque


def test_cli_without_the_flag_writes_rgb_as_ever(cuda_device, tmp_path):
    imgs = _cli_inputs(tmp_path / 'in')
    out = tmp_path / 'out'
    inference.main(['-i', str(tmp_path / 'in'), '-o', str(out), '--synthetic-seed', str(SEED)])
    net = _cli_net(cuda_device)
    for name in imgs:
        rgb = np.array(Image.open(str(tmp_path / 'in' / name)).convert('RGB'))
        buf = io.BytesIO()
        Image.fromarray(_np(net.test_u8(torch.from_numpy(rgb).to(cuda_device))), 'RGB').save(buf, 'PNG')
        assert (out / name).read_bytes() == buf.getvalue(), name


def test_cli_names_the_other_alpha_mode_for_a_tiny_image(cuda_device, tmp_path):
    """A 1-pixel-high RGBA image has no bicubic tables: the message says what to pass instead.  (The network's own size limit is another
    matter: the forward is never reached.)"""
    (tmp_path / 'in').mkdir()
    Image.fromarray(np.full((1, 16, 4), 200, np.uint8), 'RGBA').save(str(tmp_path / 'in' / 'thin.png'))
    with pytest.raises(SystemExit) as e:
        inference.main(['-i', str(tmp_path / 'in'), '-o', str(tmp_path / 'out'), '--synthetic-seed', str(SEED), '--keep-format'])
    assert '--alpha network' in str(e.value)

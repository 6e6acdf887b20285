"""-m gpu: the final resample of the output image on the device (csrc/resample.hip, femasr_amd/resample.py).

Bytes in, one fp64 sum per output in the definition's order, bytes out: everything is compared BIT FOR BIT with resample.resample_ref (held
to femasr_model.imresize in test_resample_host.py); no tolerance appears in this module.  The C entry runs on the guard arenas of
tests/guard_arena.py - every operand at its exact size between poison, once per poison: no byte outside the output may change and the
output may not depend on the poison."""
import numpy as np
import pytest
import torch
from PIL import Image

from femasr_amd import _lib, channels as CH, inference, resample as RS, synth
from resample_utils import resample_entry, step_image, tie_image

pytestmark = pytest.mark.gpu

# (H, W) -> (out_h, out_w).  Down / up on both axes; one axis down and the other up, both ways (7x40 -> 11x10, 40x7 -> 10x11); the height
# kept in a three-column image beside 1/4 in H (64x3 -> 16x3: identity tables in W); the two extreme ratios, at the smallest
# lengths imresize_tables takes for them (24 -> 3: 32 taps, every source pixel tapped by every output; 3 -> 24); the smallest image with a
# true tie; odd sizes whose rows start off a dword for C = 1, 2, 3
CASES = [((13, 17), (10, 13)), ((9, 11), (14, 16)), ((12, 20), (9, 15)), ((7, 40), (11, 10)), ((40, 7), (10, 11)), ((64, 3), (16, 3)),
         ((24, 24), (3, 3)), ((3, 3), (24, 24)), ((2, 2), (3, 3)), ((33, 65), (25, 49))]


def _same(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = np.argwhere(got != ref)
    assert bad.size == 0, f'{what}: {len(bad)} of {got.size} bytes differ, the first at {bad[0].tolist()}: {got[tuple(bad[0])]} for {ref[tuple(bad[0])]}'


def _np(t):
    return t.cpu().numpy()


def _image(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ the C entry on guard arenas
@pytest.mark.parametrize('C', [1, 2, 3, 4])
@pytest.mark.parametrize('case', CASES, ids=lambda v: f'{v[0][0]}x{v[0][1]}to{v[1][0]}x{v[1][1]}')
def test_entry(cuda_device, case, C):
    (H, W), (oh, ow) = case
    if (H, W) == (2, 2):
        img = tie_image()[..., [c % 2 for c in range(C)]]                            # the tie of test_resample_host.py in every channel
        assert RS.resample_values(img, 3, 3)[1, 1, 0] == 151.5
    else:
        img = _image((H, W, C), 100 * H + W + C)
    _same(resample_entry(img, oh, ow), RS.resample_ref(img, oh, ow), f'{case} C={C}')


@pytest.mark.parametrize('ratio', [(3, 4), (3, 2)], ids=['down', 'up'])
def test_tile_edges(cuda_device, ratio):
    """Output rows of one pixel less than a tile, a tile, one pixel more, and two tiles and a pixel (three blocks per row); two output rows."""
    num, den = ratio
    assert _lib.load().femasr_resample_tile() == RS.TILE
    for ow in (RS.TILE - 1, RS.TILE, RS.TILE + 1, 2 * RS.TILE + 1):
        W = -(-ow * den // num)
        img = _image((3, W, 3), ow)
        _same(resample_entry(img, 2, ow), RS.resample_ref(img, 2, ow), f'{W} -> {ow}')
    img = _image((3, 2 * RS.TILE + 7, 4), 5)                                         # C = 4 through the dword store, past a tile
    _same(resample_entry(img, 2, 2 * RS.TILE + 1), RS.resample_ref(img, 2, 2 * RS.TILE + 1), 'C=4')


def test_identity_flat_and_step(cuda_device):
    img = _image((13, 17, 3), 1)
    _same(resample_entry(img, 13, 17), img, 'identity')
    for v in (0, 1, 127, 128, 254, 255):
        flat = np.full((11, 13, 1), v, np.uint8)
        for oh, ow in ((8, 10), (17, 20), (3, 4)):
            _same(resample_entry(flat, oh, ow), np.full((oh, ow, 1), v, np.uint8), f'flat {v} -> {oh}x{ow}')
    step = step_image()
    vals = RS.resample_values(step, 24, 24)
    assert vals.min() < -15 and vals.max() > 270                                     # both clips decide bytes of this case
    got = resample_entry(step[..., None], 24, 24)[..., 0]
    _same(got, RS.resample_ref(step, 24, 24), 'step')
    assert got.min() == 0 and got.max() == 255


def test_foreign_tables_stay_inside_the_image(cuda_device):
    """The C entry takes the caller's tables.  Ones imresize_tables would never make: every output column taps the first AND the last source
    column, so the columns a tile taps (600) exceed the window the host staged for it (532: the H pass of the rest comes straight from
    memory), and some indices lie outside the image on both axes (the kernel clamps them to it).  The sums are the definition's loops over
    these tables with the clamped indices."""
    H, W, oh, ow, C = 9, 600, 5, 8, 3
    img = _image((H, W, C), 8)
    rng = np.random.default_rng(9)
    wh, ww = rng.uniform(-0.2, 0.6, (oh, 3)), rng.uniform(-0.2, 0.6, (ow, 4))
    wh, ww = wh / wh.sum(1, keepdims=True), ww / ww.sum(1, keepdims=True)               # rows sum to 1: the values stay near the byte range
    ih = rng.integers(-4, H + 4, (oh, 3)).astype(np.int32)
    iw = rng.integers(0, W, (ow, 4)).astype(np.int32)
    iw[:, 0], iw[:, 3] = 0, W - 1
    iw[2, 1], iw[5, 2] = -7, W + 1000
    assert ih.min() < 0 and ih.max() >= H
    x = img.astype(np.float64)
    h1 = np.zeros((oh, W, C))
    for k in range(3):
        h1 = h1 + wh[:, k][:, None, None] * x[np.clip(ih[:, k], 0, H - 1)]
    v = np.zeros((oh, ow, C))
    for k in range(4):
        v = v + ww[:, k][None, :, None] * h1[:, np.clip(iw[:, k], 0, W - 1)]
    want = np.rint(np.clip(v, 0, 255)).astype(np.uint8)
    assert len(np.unique(want)) > 32                                                    # not a saturated image
    _same(resample_entry(img, oh, ow, tables=(wh, ih, ww, iw)), want, 'foreign tables')


# ------------------------------------------------------------------------------------------------ the Python wrapper
def test_wrapper(cuda_device):
    dev = cuda_device
    for (H, W), (oh, ow), C in (((13, 17), (10, 23), 3), ((40, 7), (10, 11), 4), ((9, 300), (9, 2 * RS.TILE + 3), 2)):
        img = _image((H, W, C), H + W)
        x = torch.from_numpy(img).to(dev)
        got = RS.resample_u8(x, oh, ow)
        assert got.shape == (oh, ow, C) and got.dtype == torch.uint8 and got.device == x.device
        _same(_np(got), RS.resample_ref(img, oh, ow), f'resample_u8 {H}x{W}x{C}')
        out = torch.empty((oh, ow, C), dtype=torch.uint8, device=dev)
        assert RS.resample_u8(x, oh, ow, out=out).data_ptr() == out.data_ptr()
        _same(_np(out), _np(got), 'out=')
    gray = _image((12, 20), 4)
    got = RS.resample_u8(torch.from_numpy(gray).to(dev), 9, 31)
    assert got.dim() == 2
    _same(_np(got), RS.resample_ref(gray, 9, 31), '(H,W)')
    _same(_np(RS.resample_u8(torch.from_numpy(gray[..., None].copy()).to(dev), 9, 31)), RS.resample_ref(gray, 9, 31)[..., None], '(H,W,1)')
    # a buffer that starts one byte off a dword: byte stores for C = 4, unaligned window loads
    odd = torch.from_numpy(_image(1 + 9 * 11 * 4, 6)).to(dev)[1:].view(9, 11, 4)
    odd_out = torch.empty(1 + 14 * 16 * 4, dtype=torch.uint8, device=dev)[1:].view(14, 16, 4)
    _same(_np(RS.resample_u8(odd, 14, 16, out=odd_out)), RS.resample_ref(_np(odd), 14, 16), 'off a dword')
    x = torch.zeros((16, 16, 3), dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.FemasrError):
        RS.resample_u8(x.cpu(), 8, 8)
    with pytest.raises(RS.ResampleRatio) as e:
        RS.resample_u8(x, 16, 129)
    assert '1/8 .. 8' in str(e.value)
    with pytest.raises(RS.ResampleRatio):
        RS.resample_u8(x, 1, 16)
    with pytest.raises(RS.ResampleTooSmall):
        RS.resample_u8(x[:1].contiguous(), 1, 16)                                    # a 1-pixel axis has no tables, even at equal size
    for bad in (lambda: RS.resample_u8(x.float(), 8, 8), lambda: RS.resample_u8(torch.zeros((16, 16, 5), dtype=torch.uint8, device=dev), 8, 8),
                lambda: RS.resample_u8(x.transpose(0, 1), 8, 8), lambda: RS.resample_u8(x[:, :, :2], 8, 8), lambda: RS.resample_u8(x[0, 0], 8, 8),
                lambda: RS.resample_u8(x, 0, 8), lambda: RS.resample_u8(x, 8.0, 8), lambda: RS.resample_u8(x, 8, 8, out=x),
                lambda: RS.resample_u8(x, 8, 8, out=torch.empty((8, 8, 3), dtype=torch.uint8))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        RS.resample_u8(np.zeros((16, 16, 3), np.uint8), 8, 8)


def test_graph_capture(cuda_device):
    """One capture of a call, two replays on new input bytes: each equals the eager result (a launch that escaped the capture, or a host
    read of the image, would show the first input's result)."""
    dev = cuda_device
    imgs = [torch.from_numpy(_image((37, 530, 3), s)).to(dev) for s in (1, 2, 3)]
    eager = [RS.resample_u8(x, 28, 398).clone() for x in imgs]                       # (also makes the device tables: a capture copies nothing)
    assert not torch.equal(eager[1], eager[2])
    _same(_np(eager[2]), RS.resample_ref(_np(imgs[2]), 28, 398), 'eager')
    static_in, static_out = imgs[0].clone(), torch.zeros_like(eager[0])
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        RS.resample_u8(static_in, 28, 398, out=static_out)
    for x, want in zip(imgs[1:], eager[1:]):
        static_in.copy_(x)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(static_out, want)


def test_past_2_to_31_input_bytes(cuda_device):
    """23200 x 23200 x 4 = 2.15e9 input bytes -> 17400 x 17400 x 4: offsets of the source window pass 2^31.  Eight output rows, the first and
    the last among them, against the definition's sums evaluated on the source rows those rows tap."""
    dev = cuda_device
    if torch.cuda.mem_get_info(dev)[0] < 6 << 30:
        pytest.skip('less than 6 GiB of device memory free')
    n, o, C = 23200, 17400, 4
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    x = torch.empty((n, n, C), dtype=torch.uint8, device=dev)
    for y0 in range(0, n, 2900):                                                     # (in slabs: no generator needs 2^31 values in one call)
        x[y0:y0 + 2900] = torch.randint(0, 256, (2900, n, C), dtype=torch.uint8, device=dev, generator=g)
    assert x.numel() > 1 << 31
    out = RS.resample_u8(x, o, o)
    wh, ih = RS._tables(n, o)
    ww, iw = RS._tables(n, o)
    rows = [0, o - 1] + sorted(np.random.default_rng(12).choice(np.arange(1, o - 1), 6, replace=False).tolist())
    assert ih[o - 1].max() == n - 1 and (ih[o - 1].astype(np.int64).max() * n + n) * C > 1 << 31
    for Y in rows:
        src = _np(x[torch.from_numpy(ih[Y].astype(np.int64)).to(dev)]).astype(np.float64)      # (taps, n, C): the rows output row Y taps
        h1 = np.zeros((n, C))
        for k in range(wh.shape[1]):
            h1 = h1 + wh[Y, k] * src[k]
        v = np.zeros((o, C))
        for k in range(ww.shape[1]):
            v = v + ww[:, k][:, None] * h1[iw[:, k]]
        _same(_np(out[Y]), np.rint(np.clip(v, 0, 255)).astype(np.uint8), f'row {Y}')
    del x, out
    torch.cuda.empty_cache()


def test_row_restatement_is_the_definition():
    """The per-row sums of test_past_2_to_31_input_bytes are resample_ref's, on an image small enough to run it whole."""
    img = _image((29, 31, 4), 2)
    wh, ih = RS._tables(29, 22)
    ww, iw = RS._tables(31, 23)
    ref = RS.resample_ref(img, 22, 23)
    for Y in (0, 9, 21):
        src = img[ih[Y]].astype(np.float64)
        h1 = np.zeros((31, 4))
        for k in range(wh.shape[1]):
            h1 = h1 + wh[Y, k] * src[k]
        v = np.zeros((23, 4))
        for k in range(ww.shape[1]):
            v = v + ww[:, k][:, None] * h1[iw[:, k]]
        _same(np.rint(np.clip(v, 0, 255)).astype(np.uint8), ref[Y], f'row {Y}')


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
    rng = np.random.default_rng(21)
    rgba = rng.integers(0, 256, (20, 24, 4), dtype=np.uint8)
    rgba[:, ::2, 3] = 0
    imgs = {'a_rgb.png': rng.integers(0, 256, (24, 20, 3), dtype=np.uint8), 'b_rgba.png': rgba}
    folder.mkdir()
    for name, a in imgs.items():
        Image.fromarray(a, CH.MODES[a.shape[2]]).save(str(folder / name))
    return imgs


def _run_cli(tmp_path, out, threads, *flags):
    inference.main(['-i', str(tmp_path / 'in'), '-o', str(tmp_path / out), '--synthetic-seed', str(SEED), '--io-threads', str(threads)] + list(flags))
    return {p.name: np.array(Image.open(str(p))) for p in (tmp_path / out).iterdir()}


@pytest.mark.parametrize('flags,size', [(('--final-scale', '3'), None), (('--final-size', '50x70'), (70, 50))], ids=['scale3', 'size50x70'])
@pytest.mark.parametrize('threads', [0, 2])
def test_cli_rgb(cuda_device, tmp_path, threads, flags, size):
    imgs = _cli_inputs(tmp_path / 'in')
    got = _run_cli(tmp_path, 'out', threads, *flags)
    net = _cli_net(cuda_device)
    assert sorted(got) == sorted(imgs)
    for name, a in imgs.items():
        rgb = np.array(Image.open(str(tmp_path / 'in' / name)).convert('RGB'))
        oh, ow = size or (3 * a.shape[0], 3 * a.shape[1])
        assert size or (oh, ow) == {'a_rgb.png': (72, 60), 'b_rgba.png': (60, 72)}[name]
        want = RS.resample_ref(_np(net.test_u8(torch.from_numpy(rgb).to(cuda_device))), oh, ow)
        _same(got[name], want, f'{name} {flags}')


@pytest.mark.parametrize('threads', [0, 2])
def test_cli_keep_format(cuda_device, tmp_path, threads):
    imgs = _cli_inputs(tmp_path / 'in')
    got = _run_cli(tmp_path, 'out', threads, '--keep-format', '--final-scale', '3')
    net = _cli_net(cuda_device)
    for name, a in imgs.items():
        sr = _np(CH.upscale_u8(torch.from_numpy(a).to(cuda_device), net.test_u8, 4))
        assert sr.shape == (4 * a.shape[0], 4 * a.shape[1], a.shape[2])
        assert got[name].shape == (3 * a.shape[0], 3 * a.shape[1], a.shape[2])        # the RGBA file keeps its 4 channels
        _same(got[name], RS.resample_ref(sr, 3 * a.shape[0], 3 * a.shape[1]), f'{name} --keep-format')
    assert not (got['b_rgba.png'][..., 3] == 255).all()


@pytest.mark.parametrize('threads', [0, 2])
def test_cli_final_scale_of_the_network_is_no_resample(cuda_device, tmp_path, threads):
    _cli_inputs(tmp_path / 'in')
    plain = _run_cli(tmp_path, 'plain', threads)
    same = _run_cli(tmp_path, 'same', threads, '--final-scale', '4')
    assert sorted(plain) == sorted(same)
    for name in plain:
        _same(same[name], plain[name], name)
        if threads == 0:                                                             # (the banded deflate of --io-threads N is the same pixels only)
            assert (tmp_path / 'same' / name).read_bytes() == (tmp_path / 'plain' / name).read_bytes()


def test_cli_names_the_ratio_limit(cuda_device, tmp_path):
    """2400 -> 10 columns is far below 1/8: refused by name before the forward runs."""
    (tmp_path / 'in').mkdir()
    Image.fromarray(_image((8, 600, 3), 1), 'RGB').save(str(tmp_path / 'in' / 'wide.png'))
    with pytest.raises(SystemExit) as e:
        inference.main(['-i', str(tmp_path / 'in'), '-o', str(tmp_path / 'out'), '--synthetic-seed', str(SEED), '--final-size', '10x10'])
    assert 'wide.png' in str(e.value) and '1/8 .. 8' in str(e.value)
    assert not list((tmp_path / 'out').iterdir())

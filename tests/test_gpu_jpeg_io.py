"""-m gpu: fast JPEG output on the device (csrc/jpeg_dct.hip, femasr_amd/jpegio.py).

The kernel is integer work: everything here is compared BIT FOR BIT with the numpy definition `jpegio.coefficients_ref` (held to a float64 DCT
and to Pillow's decoder in test_jpeg_io_host.py), files byte for byte with `jpegio.encode_ref`; no tolerance appears in this module."""
import ctypes
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import guard_arena as GA
import gpu_utils as G
from femasr_amd import _lib, jpegio, pngio

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (H, W): below one MCU; exactly one 8x8 / 16x16 MCU; odd sizes whose padding differs between 8 and 16; several MCU rows and (130x70) sizes that
# are no multiple of either MCU; 64x259: more than the 256 pixel columns of one block - two strips, the second of one (8x8) / one (16x16) MCU
SHAPES = [(1, 1), (8, 8), (15, 17), (16, 16), (17, 33), (130, 70), (64, 259)]
QUALITIES = (1, 50, 90, 100)
CONTENTS = ('noise', 'zeros', 'ones', 'checker1', 'checker8', 'red')


def _content(kind, h, w, channels, seed):
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == 'noise':
        g = np.random.RandomState(seed).randint(0, 256, (h, w, channels)).astype(np.uint8)
        return g[..., 0] if channels == 1 else g
    if kind == 'red':                                        # (gray: its red channel, a flat 255, is 'ones'; a ramp instead)
        if channels == 1:
            return ((yy * 7 + xx * 3) & 255).astype(np.uint8)
        out = np.zeros((h, w, 3), np.uint8)
        out[..., 0] = 255
        return out
    g = {'zeros': np.zeros((h, w), np.uint8), 'ones': np.full((h, w), 255, np.uint8), 'checker1': (((yy + xx) & 1) * 255).astype(np.uint8),
         'checker8': (((yy // 8 + xx // 8) & 1) * 255).astype(np.uint8)}[kind]
    return g if channels == 1 else np.ascontiguousarray(np.repeat(g[..., None], 3, axis=2))


def _coefficients_entry(img, quality, subsampling):
    """femasr_jpeg_coefficients_u8 on a guard arena under both poisons: the image, the tables and the planes are regions of their exact size;
    no byte outside the planes may change and the planes may not depend on the poison."""
    H, W, C = jpegio.check_shape(img.shape)
    shapes = jpegio.geometry(H, W, C, subsampling)[2]
    tabs = jpegio.kernel_tables(quality)
    what = f'jpeg_coefficients_u8 {H}x{W}x{C} q{quality} {subsampling}'

    def go():
        ops = G.Operands(what).inp('img', img).inp('qy', tabs[0])
        if C == 3:
            ops.inp('qc', tabs[1])
        for i, (hb, wb) in enumerate(shapes):
            ops.out(f'out{i}', hb * wb * 128)
        ops.build()
        _lib.check(_lib.load().femasr_jpeg_coefficients_u8(ops.p('img'), H, W, C, 0 if C == 1 else int(subsampling), ops.p('qy'), ops.p('qc'),
                                                           ops.p('out0'), ops.p('out1'), ops.p('out2'), None))
        ops.check()
        return [ops.get(f'out{i}', torch.int16, (hb, wb, 64)).cpu().numpy() for i, (hb, wb) in enumerate(shapes)]
    return GA.run_twice(go, what)


@pytest.mark.parametrize('hw', SHAPES, ids=lambda v: f'{v[0]}x{v[1]}')
def test_kernel_equals_definition(cuda_device, hw):
    h, w = hw
    for ci, kind in enumerate(CONTENTS):
        for channels, subs in ((1, ('444',)), (3, ('444', '420'))):
            img = _content(kind, h, w, channels, 10 * ci + channels)
            for ss in subs:
                for q in QUALITIES:
                    want = jpegio.coefficients_ref(img, q, ss)
                    got = _coefficients_entry(img, q, ss)
                    assert len(got) == len(want) == channels
                    for k, (a, b) in enumerate(zip(got, want)):
                        bad = np.argwhere(a != b)
                        assert a.shape == b.shape and bad.size == 0, \
                            f'{kind} C={channels} {ss} q{q}, component {k}: {len(bad)} coefficients differ, first at (by, bx, k) {bad[0].tolist()}'


def test_python_entry_and_refusals(cuda_device):
    rng = np.random.RandomState(2)
    img = rng.randint(0, 256, (37, 53, 3)).astype(np.uint8)
    t = torch.from_numpy(img).to(cuda_device)
    for ss in ('444', '420', 420):
        got = jpegio.coefficients_gpu(t, 75, ss)
        want = jpegio.coefficients_ref(img, 75, ss)
        assert all(g.dtype == torch.int16 and g.is_cuda and np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want)) and len(got) == 3
    # an image that starts 3 bytes off any alignment, and a view that is not contiguous
    raw = torch.zeros(img.size + 64, dtype=torch.uint8, device=cuda_device)
    raw[3:3 + img.size] = t.reshape(-1)
    off = raw[3:3 + img.size].view(37, 53, 3)
    assert off.data_ptr() % 4 == 3
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(jpegio.coefficients_gpu(off, 75, '420'), jpegio.coefficients_ref(img, 75, '420')))
    view = torch.from_numpy(np.ascontiguousarray(img.transpose(1, 0, 2))).to(cuda_device).transpose(0, 1)
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(jpegio.coefficients_gpu(view, 75, '444'), jpegio.coefficients_ref(img, 75, '444')))
    gray = jpegio.coefficients_gpu(t[..., 1], 50)
    assert len(gray) == 1 and np.array_equal(gray[0].cpu().numpy(), jpegio.coefficients_ref(img[..., 1], 50)[0])
    flat, views = jpegio.coefficients_flat_gpu(t, 75, '420')
    assert flat.numel() == sum(v.numel() for v in views) and views[0].data_ptr() == flat.data_ptr()
    for bad in (t.cpu(), t.float(), t[..., :2], t[:0], torch.zeros(8, 8, 4, dtype=torch.uint8, device=cuda_device),
                torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device=cuda_device), torch.zeros(1, 65536, dtype=torch.uint8, device=cuda_device)):
        with pytest.raises(ValueError):
            jpegio.coefficients_gpu(bad, 75)
    for q, ss in ((0, '420'), (101, '420'), (75, '422')):
        with pytest.raises(ValueError):
            jpegio.coefficients_gpu(t, q, ss)
    # the C entry's refusals leave the planes untouched
    lib = _lib.load()
    out = torch.full((3, 5 * 7 * 64 + 64), 0x5A5A, dtype=torch.int16, device=cuda_device)
    tab = jpegio.device_tables(75, cuda_device)
    s = torch.cuda.current_stream(cuda_device).cuda_stream
    p = lambda x: ctypes.c_void_p(x.data_ptr())      # noqa: E731
    base = dict(img=p(t), H=37, W=53, C=3, sub=444, qy=p(tab[0]), qc=p(tab[1]), y=p(out[0]), cb=p(out[1]), cr=p(out[2]))
    for kw in (dict(img=None), dict(H=0), dict(W=-1), dict(H=65536), dict(C=2), dict(C=4), dict(sub=422), dict(sub=0), dict(qy=None), dict(qc=None),
               dict(y=None), dict(cr=None), dict(C=1, sub=0), dict(y=ctypes.c_void_p(out[0].data_ptr() + 2))):
        a = dict(base, **kw)
        rc = lib.femasr_jpeg_coefficients_u8(a['img'], a['H'], a['W'], a['C'], a['sub'], a['qy'], a['qc'], a['y'], a['cb'], a['cr'], s)
        assert rc == -1 and lib.femasr_last_error(), kw
    torch.cuda.synchronize(cuda_device)
    assert bool((out == 0x5A5A).all())


def test_entropy_entry_on_a_guard_arena():
    """The host coder with its operands in a (host) guard arena: planes of their exact size, the output buffer of EXACTLY the scan's size."""
    rng = np.random.RandomState(4)
    for img, ss in ((rng.randint(0, 256, (40, 24)).astype(np.uint8), '444'), (rng.randint(0, 256, (17, 33, 3)).astype(np.uint8), '444'),
                    (rng.randint(0, 256, (17, 33, 3)).astype(np.uint8), '420')):
        comps = jpegio.coefficients_ref(img, 100, ss)
        want = jpegio.entropy_ref(comps, ss)
        my, mx = comps[-1].shape[:2]
        code = 0 if len(comps) == 1 else int(ss)
        assert len(want) <= _lib.load().femasr_jpeg_entropy_bound(mx, len(comps), code, my)

        def go():
            ops = G.Operands(f'jpeg_entropy_rows {img.shape} {ss}', device='cpu')
            for i, c in enumerate(comps):
                ops.inp(f'c{i}', c)
            ops.out('scan', len(want)).build()
            n = _lib.load().femasr_jpeg_entropy_rows(ops.p('c0'), ops.p('c1'), ops.p('c2'), len(comps), code, my, mx, 0, my, ops.p('scan'), len(want))
            ops.check()
            assert n == len(want)
            return ops.get('scan', torch.uint8).numpy().tobytes()
        assert GA.run_twice(go, 'jpeg_entropy_rows') == want


def test_offsets_past_2_31_elements(cuda_device):
    """Gray 46400 x 46400: the plane has 5800^2 * 64 = 2.15e9 coefficients (4.3 GB), the image 2.15 GB; noise made on the device.  The first and
    last two MCU rows and 64 seeded blocks are compared with the definition on the crops they depend on."""
    n = 46400
    nb = n // 8
    assert nb * nb * 64 > 1 << 31
    free = torch.cuda.mem_get_info(cuda_device)[0]
    need = n * n + nb * nb * 128 + (2 << 30)               # image, plane, and the generator's chunk with some slack
    if free < need:
        pytest.skip(f'{free >> 20} MiB of device memory free, the 46400 x 46400 case needs {need >> 20} MiB')
    img = torch.empty((n, n), dtype=torch.uint8, device=cuda_device)
    g = torch.Generator(device=cuda_device)
    g.manual_seed(23)
    flat = img.view(-1)
    step = 1 << 28
    for lo in range(0, flat.numel(), step):
        part = flat[lo:lo + step]
        part.copy_(torch.randint(0, 256, (part.numel(),), dtype=torch.uint8, device=cuda_device, generator=g))
    plane, = jpegio.coefficients_gpu(img, 90)
    assert plane.shape == (nb, nb, 64) and plane.numel() > 1 << 31
    for rows in (slice(0, 2), slice(nb - 2, nb)):
        crop = img[8 * (rows.start):8 * rows.stop].cpu().numpy()
        assert np.array_equal(plane[rows].cpu().numpy(), jpegio.coefficients_ref(crop, 90)[0]), rows
    rng = np.random.RandomState(29)
    picks = [(int(rng.randint(0, nb)), int(rng.randint(0, nb))) for _ in range(62)] + [(nb - 1, nb - 1), ((1 << 31) // 64 // nb + 1, 7)]
    crops = np.stack([img[8 * by:8 * by + 8, 8 * bx:8 * bx + 8].cpu().numpy() for by, bx in picks])
    got = np.stack([plane[by, bx].cpu().numpy() for by, bx in picks])
    want = jpegio.coefficients_ref(np.ascontiguousarray(crops.reshape(64 * 8, 8)), 90)[0][:, 0]
    assert any((by * nb + bx) * 64 > 1 << 31 for by, bx in picks) and np.array_equal(got, want)


@pytest.mark.parametrize('case', [((17, 33, 3), '420'), ((64, 259, 3), '444'), ((40, 24), '444')], ids=lambda v: f'{"x".join(map(str, v[0]))}_{v[1]}')
def test_graph_replay_and_side_stream(cuda_device, case):
    """Captured with torch.cuda.graph and replayed on a second input: a launch that escaped the capture ran once, on the first input, and shows
    here.  Then on a side stream behind a queue of matmuls (the probabilistic check of test_gpu_graph_streams.py)."""
    from test_gpu_graph_streams import _side_stream_check
    shape, ss = case
    rng = np.random.RandomState(3)
    a, b = (torch.from_numpy(rng.randint(0, 256, shape).astype(np.uint8)).to(cuda_device) for _ in range(2))
    ea, eb = jpegio.coefficients_flat_gpu(a, 90, ss)[0], jpegio.coefficients_flat_gpu(b, 90, ss)[0]      # (also warms the table cache)
    assert not torch.equal(ea, eb)
    want = np.concatenate([c.reshape(-1) for c in jpegio.coefficients_ref(b.cpu().numpy(), 90, ss)])
    assert np.array_equal(eb.cpu().numpy(), want)
    static_in = a.clone()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(cuda_device)
    side.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            static_out = jpegio.coefficients_flat_gpu(static_in, 90, ss)[0]
    torch.cuda.current_stream(cuda_device).wait_stream(side)
    graph.replay()
    assert torch.equal(static_out, ea)
    static_in.copy_(b)
    graph.replay()
    assert torch.equal(static_out, eb), 'replay on new input'
    _side_stream_check(lambda t: jpegio.coefficients_flat_gpu(t, 90, ss)[0], [b], cuda_device, 'coefficients_gpu')


def test_writer_writes_encode_ref(cuda_device, tmp_path):
    rng = np.random.RandomState(12)
    rgb, gray = rng.randint(0, 256, (17, 33, 3)).astype(np.uint8), rng.randint(0, 256, (40, 24)).astype(np.uint8)
    mid = rng.randint(0, 256, (9, 13, 3)).astype(np.uint8)
    with pngio.PngWriter(threads=2, jpeg_quality=90) as w:
        assert (w.jpeg_quality, w.jpeg_subsampling) == (90, '420')
        w.submit(torch.from_numpy(rgb).to(cuda_device), tmp_path / 'a.jpg')
        w.submit(torch.from_numpy(mid).to(cuda_device), tmp_path / 'm.png')
        w.submit(torch.from_numpy(gray).to(cuda_device), tmp_path / 'b.JPEG')
        w.submit(torch.from_numpy(mid).to(cuda_device), tmp_path / 'n.bmp')
    assert (tmp_path / 'a.jpg').read_bytes() == jpegio.encode_ref(rgb, 90, '420')
    assert (tmp_path / 'b.JPEG').read_bytes() == jpegio.encode_ref(gray, 90, '420')
    assert (tmp_path / 'm.png').read_bytes() == pngio.encode_png(pngio.filter_rows(mid), 13, 9)      # unchanged from today
    assert np.array_equal(np.array(Image.open(str(tmp_path / 'n.bmp'))), mid)
    with pngio.PngWriter(threads=2, jpeg_quality=35, jpeg_subsampling='444') as w:
        w.submit(torch.from_numpy(rgb).to(cuda_device), tmp_path / 'c.jpeg')
    assert (tmp_path / 'c.jpeg').read_bytes() == jpegio.encode_ref(rgb, 35, '444')
    with Image.open(str(tmp_path / 'c.jpeg')) as im:
        assert im.format == 'JPEG' and im.size == (33, 17) and im.mode == 'RGB'
    # without the quality the same path is Image.save's, byte for byte
    with pngio.PngWriter(threads=2) as w:
        w.submit(torch.from_numpy(rgb).to(cuda_device), tmp_path / 'd.jpg')
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, 'JPEG')
    assert (tmp_path / 'd.jpg').read_bytes() == buf.getvalue()
    # a worker's exception comes back on close()
    w = pngio.PngWriter(threads=2, jpeg_quality=90)
    w.submit(torch.from_numpy(rgb).to(cuda_device), tmp_path / 'no_such_dir' / 'e.jpg')
    with pytest.raises(FileNotFoundError):
        w.close()
    with pytest.raises(ValueError):
        with pngio.PngWriter(threads=1, jpeg_quality=90) as w:
            w.submit(torch.from_numpy(rgb).to(cuda_device).float(), tmp_path / 'f.jpg')


def test_cli_jpeg_flags(cuda_device, tmp_path):
    """The CLI over two .jpg inputs and a .png, in fresh processes: with the flags every JPEG is encode_ref of the network's bytes and the PNG is
    the one a run without them writes; without --jpeg-quality the .jpg outputs are Image.save's bytes, as on the parent commit."""
    from femasr_amd import synth
    from femasr_amd.archs.femasr_arch import FeMaSRNet
    rng = np.random.RandomState(8)
    src = tmp_path / 'in'
    src.mkdir()
    Image.fromarray(rng.randint(0, 256, (24, 32, 3)).astype(np.uint8), 'RGB').save(str(src / 'small.jpg'), quality=95)
    Image.fromarray(rng.randint(0, 256, (36, 28, 3)).astype(np.uint8), 'RGB').save(str(src / 'tall.jpg'), quality=95)
    Image.fromarray(rng.randint(0, 256, (20, 28, 3)).astype(np.uint8), 'RGB').save(str(src / 'im.png'))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    runs = {'fast': ['--io-threads', '2', '--jpeg-quality', '90', '--jpeg-subsampling', '444'], 'plain': ['--io-threads', '2']}
    for tag, flags in runs.items():
        p = subprocess.run([sys.executable, '-m', 'femasr_amd.inference', '-i', str(src), '-o', str(tmp_path / tag), '--synthetic-seed', '3'] + flags,
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
    names = sorted(os.listdir(str(src)))
    assert sorted(os.listdir(str(tmp_path / 'fast'))) == names == sorted(os.listdir(str(tmp_path / 'plain')))
    model = FeMaSRNet(codebook_params=[[32, 1024, 512]], LQ_stage=True, scale_factor=4)
    weights = synth.fill_state_dict(model.state_dict(), 3, 'trained')
    model.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()}, strict=False)
    model.decoder_math, model.linear_math = 'fp32', 'bf16_split'          # the CLI's defaults
    model = model.to(cuda_device).eval()
    for name in ('small.jpg', 'tall.jpg'):
        x = np.array(Image.open(str(src / name)).convert('RGB'))
        u8 = model.test_u8(torch.from_numpy(x).to(cuda_device)).cpu().numpy()
        assert u8.shape == (4 * x.shape[0], 4 * x.shape[1], 3)
        assert (tmp_path / 'fast' / name).read_bytes() == jpegio.encode_ref(u8, 90, '444'), name
        buf = io.BytesIO()
        Image.fromarray(u8, 'RGB').save(buf, 'JPEG')
        assert (tmp_path / 'plain' / name).read_bytes() == buf.getvalue(), f'{name}: without --jpeg-quality the file is no longer Image.save\'s'
    assert (tmp_path / 'fast' / 'im.png').read_bytes() == (tmp_path / 'plain' / 'im.png').read_bytes()

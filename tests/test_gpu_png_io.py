"""-m gpu: fast PNG output on the device (csrc/png_filter.hip, femasr_amd/pngio.py).

The kernel is integer work: everything here is compared BIT FOR BIT with the numpy definition `pngio.filter_rows` (held to a byte-by-byte
restatement and to PIL's decoder in test_png_io_host.py); no tolerance appears in this module."""
import ctypes
import io
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

from femasr_amd import _lib, pngio
from helpers import synth_weights

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
# (H, W).  Row pitches 3W / 3W + 1: (17, 5) 15 / 16 and (19, 7) 21 / 22 - every input and output residue mod 16 occurs; 3W = 1023, 1026, 4098;
# W = 1024 is the widest row one wave takes (png_filter.hip PF_WAVE_ROW = 3072 bytes), W = 8192 the widest row resident in a block's LDS
# (PF_BLOCK_ROW = 24576 bytes), each with its neighbours; (2, 21846): a row over 64 KiB, streamed in three segments
SHAPES = [(1, 1), (1, 7), (2, 1), (7, 5), (17, 5), (19, 7), (3, 341), (3, 342), (5, 1366), (3, 1023), (3, 1024), (3, 1025), (3, 8191), (3, 8192),
          (3, 8193), (2, 21846)]
CONTENTS = ('random', 'flat', 'only0_255', 'only127_128')


def _content(kind, shape, seed):
    rng = np.random.RandomState(seed)
    if kind == 'random':
        return rng.randint(0, 256, shape).astype(np.uint8)
    if kind == 'flat':
        return np.full(shape, 93, np.uint8)
    if kind == 'only0_255':
        return (rng.randint(0, 2, shape) * 255).astype(np.uint8)
    if kind == 'only127_128':
        return (127 + rng.randint(0, 2, shape)).astype(np.uint8)
    steps = rng.randint(-2, 3, shape)                      # 'smooth': what an image looks like - the five filters really compete
    return np.clip(128 + np.cumsum(steps, axis=-2) + np.cumsum(steps[..., ::-1, :, :], axis=-3), 0, 255).astype(np.uint8)


def _guarded(nbytes, shift, dev, fill=0x5A):
    """A uint8 buffer of nbytes with GUARD sentinel bytes either side, its start `shift` bytes off 16-byte alignment."""
    buf = torch.full((GUARD + 16 + nbytes + GUARD,), fill, dtype=torch.uint8, device=dev)
    off = GUARD + (shift - buf.data_ptr() - GUARD) % 16
    assert (buf.data_ptr() + off) % 16 == shift % 16
    return buf, off


def _raw_call(stream, img_ptr, B, H, W, filter, out_ptr):
    return _lib.load().femasr_png_filter_rgb8(stream, ctypes.c_void_p(img_ptr), B, H, W, filter, ctypes.c_void_p(out_ptr))


def _run_guarded(imgs, filter, dev, in_shift=0, out_shift=0):
    """The kernel on (B,H,W,3) numpy images at the given misalignments, into a guarded buffer; returns (B,H,1+3W) and checks the sentinels."""
    B, H, W = imgs.shape[:3]
    n_in, n_out = imgs.size, B * H * (1 + 3 * W)
    src, so = _guarded(n_in, in_shift, dev, 0xC3)
    src[so:so + n_in].copy_(torch.from_numpy(imgs.reshape(-1)))
    dst, do = _guarded(n_out, out_shift, dev)
    _lib.check(_raw_call(torch.cuda.current_stream(dev).cuda_stream, src.data_ptr() + so, B, H, W, filter, dst.data_ptr() + do))
    host = dst.cpu().numpy()
    assert (host[:do] == 0x5A).all() and (host[do + n_out:] == 0x5A).all(), 'bytes outside the output were written'
    return host[do:do + n_out].reshape(B, H, 1 + 3 * W)


@pytest.mark.parametrize('hw', SHAPES, ids=lambda v: f'{v[0]}x{v[1]}')
def test_kernel_equals_definition(cuda_device, hw):
    """Filters 0..4 and adaptive on four kinds of content plus an image-like one; the input and the output each start at a different
    misalignment per case, and the 64 bytes either side of the output stay untouched."""
    H, W = hw
    for ci, kind in enumerate(CONTENTS + ('smooth',)):
        img = _content(kind, (H, W, 3), 100 + ci)
        want = {f: pngio.filter_rows(img, 'adaptive' if f == 5 else f) for f in range(6)}
        if kind == 'flat' and H > 1 and W > 1:
            assert want[5][:, 0].tolist() == [1] + [2] * (H - 1)
        for f in range(6):
            got = _run_guarded(img[None], f, cuda_device, in_shift=(3 * ci + f) % 16, out_shift=(5 * ci + 2 * f + 1) % 16)[0]
            bad = np.argwhere(got != want[f])
            assert bad.size == 0, f'{kind}, filter {f}: {len(bad)} bytes differ, first at (row, byte) {bad[0].tolist()}'


def test_python_entry(cuda_device):
    img = _content('smooth', (37, 53, 3), 1)
    t = torch.from_numpy(img).to(cuda_device)
    for f, name in ((5, 'adaptive'), (4, 'paeth'), (0, 0)):
        got = pngio.filter_rows_gpu(t, name)
        assert got.shape == (37, 160) and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), pngio.filter_rows(img, name))
    view = torch.from_numpy(np.ascontiguousarray(img.transpose(1, 0, 2))).to(cuda_device).transpose(0, 1)      # not contiguous
    assert np.array_equal(pngio.filter_rows_gpu(view).cpu().numpy(), pngio.filter_rows(img))
    out = torch.empty((37, 160), dtype=torch.uint8, device=cuda_device)
    assert pngio.filter_rows_gpu(t, out=out).data_ptr() == out.data_ptr()
    for bad in (t.cpu(), t.float(), t[..., :2], t[:0], torch.zeros(2, 2, 2, 2, 3, dtype=torch.uint8, device=cuda_device)):
        with pytest.raises(ValueError):
            pngio.filter_rows_gpu(bad)
    with pytest.raises(ValueError):
        pngio.filter_rows_gpu(t, out=out[:, :-1])
    with pytest.raises(ValueError):
        pngio.filter_rows_gpu(t, 7)


@pytest.mark.parametrize('hw', [(7, 5), (19, 7), (5, 1366)], ids=lambda v: f'{v[0]}x{v[1]}')
def test_batch(cuda_device, hw):
    """Row 0 of every image has no row above it; image 1 of a batch of three equals its own launch."""
    imgs = _content('smooth', (3,) + hw + (3,), 9)
    for f in (5, 2, 4):
        got = _run_guarded(imgs, f, cuda_device, in_shift=7, out_shift=11)
        alone = _run_guarded(imgs[1:2], f, cuda_device, in_shift=2, out_shift=5)
        assert np.array_equal(got[1], alone[0])
        for b in range(3):
            assert np.array_equal(got[b], pngio.filter_rows(imgs[b], 'adaptive' if f == 5 else f)), (f, b)
    t = torch.from_numpy(imgs).to(cuda_device)
    assert np.array_equal(pngio.filter_rows_gpu(t).cpu().numpy(), np.stack([pngio.filter_rows(i) for i in imgs]))


def test_refusals_leave_the_output_untouched(cuda_device):
    H, W = 6, 9
    src = torch.zeros(H * W * 3, dtype=torch.uint8, device=cuda_device)
    dst = torch.full((H * (1 + 3 * W) + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=cuda_device)
    sp, dp, lib = src.data_ptr(), dst.data_ptr() + GUARD, _lib.load()
    s = torch.cuda.current_stream(cuda_device).cuda_stream
    cases = [dict(img=0), dict(out=0), dict(B=0), dict(B=-1), dict(H=0), dict(H=-2), dict(W=0), dict(W=-9), dict(filter=-1), dict(filter=6),
             dict(W=(1 << 22) + 1), dict(B=1 << 16, H=1 << 15)]
    for kw in cases:
        a = dict(dict(img=sp, B=1, H=H, W=W, filter=5, out=dp), **kw)
        rc = lib.femasr_png_filter_rgb8(s, ctypes.c_void_p(a['img']) if a['img'] else None, a['B'], a['H'], a['W'], a['filter'],
                                        ctypes.c_void_p(a['out']) if a['out'] else None)
        assert rc == -1 and lib.femasr_last_error(), kw
    torch.cuda.synchronize(cuda_device)
    assert bool((dst == 0x5A).all())
    _lib.check(_raw_call(s, sp, 1, H, W, 5, dp))           # the same arguments without a fault are accepted
    assert np.array_equal(dst[GUARD:-GUARD].cpu().numpy().reshape(H, -1), pngio.filter_rows(np.zeros((H, W, 3), np.uint8)))


def test_offsets_past_4_gib(cuda_device):
    """(H, W) = (66000, 21846): 4.33 GB each way, filled on the device; rows on either side of output bytes 2^31 and 2^32, the first two and
    the last are compared (the definition of row y needs rows y - 1 and y only)."""
    H, W = 66000, 21846
    n, pitch = 3 * W, 3 * W + 1
    assert H * n > 1 << 32 and H * pitch > 1 << 32
    img = torch.empty((H, W, 3), dtype=torch.uint8, device=cuda_device)
    flat = img.view(-1)
    g = torch.Generator(device=cuda_device)
    g.manual_seed(17)
    step = 1 << 30
    for lo in range(0, flat.numel(), step):                # noise of +-8 around a slow ramp: the filters compete, and differ from row to row
        part = flat[lo:lo + step]
        part.copy_(torch.randint(120, 137, (part.numel(),), dtype=torch.uint8, device=cuda_device, generator=g))
    img[1::3] //= 2
    out = torch.full((H * pitch + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=cuda_device)
    rows_out = out[GUARD:GUARD + H * pitch].view(H, pitch)
    ys = sorted({0, 1, H - 1} | {y for b in (1 << 31, 1 << 32) for y in range(b // pitch - 2, b // pitch + 3)})
    assert all(any(y * pitch <= b < (y + 1) * pitch for y in ys) for b in (1 << 31, 1 << 32)) and len(ys) == 13
    for f in (5, 4):
        pngio.filter_rows_gpu(img, 'adaptive' if f == 5 else f, out=rows_out)
        kinds = set()
        for y in ys:
            two = img[max(y - 1, 0):y + 1].cpu().numpy()
            want = pngio.filter_rows(two, 'adaptive' if f == 5 else f)[-1] if y else pngio.filter_rows(two[:1], 'adaptive' if f == 5 else f)[0]
            got = rows_out[y].cpu().numpy()
            assert np.array_equal(got, want), f'filter {f}, row {y}: {int((got != want).sum())} bytes differ'
            kinds.add(int(got[0]))
        assert f == 4 or len(kinds) >= 2, kinds
        assert bool((out[:GUARD] == 0x5A).all()) and bool((out[-GUARD:] == 0x5A).all())


@pytest.mark.parametrize('hw', [(19, 7), (6, 1500), (3, 8193)], ids=lambda v: f'{v[0]}x{v[1]}')
def test_graph_replay_and_side_stream(cuda_device, hw):
    """Captured with torch.cuda.graph and replayed on a second input: a launch that escaped the capture ran once, on the first input, and
    shows here.  Then on a side stream behind a queue of matmuls (the probabilistic check of test_gpu_graph_streams.py)."""
    from test_gpu_graph_streams import _side_stream_check
    a = torch.from_numpy(_content('smooth', hw + (3,), 3)).to(cuda_device)
    b = torch.from_numpy(_content('smooth', hw + (3,), 4)).to(cuda_device)
    ea, eb = pngio.filter_rows_gpu(a), pngio.filter_rows_gpu(b)
    assert not torch.equal(ea, eb)
    assert np.array_equal(eb.cpu().numpy(), pngio.filter_rows(b.cpu().numpy()))
    static_in, static_out = a.clone(), torch.zeros_like(ea)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(cuda_device)
    side.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            pngio.filter_rows_gpu(static_in, out=static_out)
    torch.cuda.current_stream(cuda_device).wait_stream(side)
    graph.replay()
    assert torch.equal(static_out, ea)
    static_in.copy_(b)
    graph.replay()
    assert torch.equal(static_out, eb), 'replay on new input'
    _side_stream_check(lambda t: pngio.filter_rows_gpu(t), [b], cuda_device, 'filter_rows_gpu')


def _idat(data):
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, out = 8, b''
    while pos < len(data):
        n, kind = struct.unpack('>I4s', data[pos:pos + 8])
        assert struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(data[pos + 4:pos + 8 + n])
        if kind == b'IDAT':
            out += data[pos + 8:pos + 8 + n]
        pos += 12 + n
    return out


def test_writer_on_network_outputs(cuda_device, tmp_path):
    """Five inputs of two sizes through test_u8 and a PngWriter: the files decode to the tensors, their IDAT payload inflates to
    `filter_rows` of them; a .jpg-named path goes through PIL as ever."""
    import gpu_utils as G
    net = G.build_net('x4', synth_weights('x4', 5, 'trained'), cuda_device, decoder_math='fp32')
    rng = np.random.RandomState(21)
    xs = [torch.from_numpy(rng.randint(0, 256, (24, 40, 3) if i % 2 else (33, 17, 3)).astype(np.uint8)).to(cuda_device) for i in range(5)]
    outs = []
    with pngio.PngWriter(threads=4, depth=2) as w:
        for i, x in enumerate(xs):
            u8 = net.test_u8(x)
            outs.append(u8.cpu().numpy())
            w.submit(u8, tmp_path / f'{i}.png')
            del u8                                         # the writer keeps what it needs
        w.submit(net.test_u8(xs[0]), tmp_path / 'five.jpg')
    for i, want in enumerate(outs):
        data = (tmp_path / f'{i}.png').read_bytes()
        assert want.shape == (xs[i].shape[0] * 4, xs[i].shape[1] * 4, 3)
        assert np.array_equal(np.array(Image.open(io.BytesIO(data)).convert('RGB')), want), i
        assert zlib.decompress(_idat(data)) == pngio.filter_rows(want).tobytes(), i
        assert data == pngio.encode_png(pngio.filter_rows(want), want.shape[1], want.shape[0])
    with Image.open(str(tmp_path / 'five.jpg')) as im:
        assert im.format == 'JPEG' and im.size == (outs[0].shape[1], outs[0].shape[0])
    buf = io.BytesIO()
    Image.fromarray(outs[0], 'RGB').save(buf, 'JPEG')
    assert (tmp_path / 'five.jpg').read_bytes() == buf.getvalue()
    with pytest.raises(ValueError):
        with pngio.PngWriter(threads=1) as w:
            w.submit(xs[0].float(), tmp_path / 'bad.png')


def test_cli_io_threads(cuda_device, tmp_path):
    """The CLI over five small PNGs and one .jpg-named input, --io-threads 0 and 4, each in a fresh process: the same names, the same pixels
    in the PNG-named outputs; the --io-threads 0 files are byte for byte what Image.save writes."""
    rng = np.random.RandomState(8)
    src = tmp_path / 'in'
    src.mkdir()
    for i in range(5):
        Image.fromarray(rng.randint(0, 256, (20 + 4 * (i % 2), 28, 3)).astype(np.uint8), 'RGB').save(str(src / f'im{i}.png'))
    Image.fromarray(rng.randint(0, 256, (24, 20, 3)).astype(np.uint8), 'RGB').save(str(src / 'photo.jpg'))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    for n in (0, 4):
        p = subprocess.run([sys.executable, '-m', 'femasr_amd.inference', '-i', str(src), '-o', str(tmp_path / f'out{n}'), '--synthetic-seed', '3',
                            '--io-threads', str(n)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
    names = sorted(os.listdir(str(src)))
    assert sorted(os.listdir(str(tmp_path / 'out0'))) == names == sorted(os.listdir(str(tmp_path / 'out4')))
    for name in names:
        f0, f4 = tmp_path / 'out0' / name, tmp_path / 'out4' / name
        a0, a4 = np.array(Image.open(str(f0)).convert('RGB')), np.array(Image.open(str(f4)).convert('RGB'))
        with Image.open(str(src / name)) as im:
            assert a0.shape == a4.shape == (im.height * 4, im.width * 4, 3)
        if not name.endswith('.png'):
            with Image.open(str(f4)) as im:
                assert im.format == 'JPEG'
            continue
        assert np.array_equal(a0, a4), name
        buf = io.BytesIO()
        Image.fromarray(a0, 'RGB').save(buf, 'PNG')
        assert f0.read_bytes() == buf.getvalue(), f'{name}: --io-threads 0 is no longer the Image.save path'
        assert zlib.decompress(_idat(f4.read_bytes())) == pngio.filter_rows(a0).tobytes()


def test_validation_io_threads(cuda_device, tmp_path):
    """`val: io_threads: 2`: validation saves the same pixels (both files: save_img_path and save_as_dir) as without the key."""
    from femasr_amd.data import build_dataloader, build_dataset
    from femasr_amd.models import build_model
    rng = np.random.RandomState(4)
    lq = tmp_path / 'lq'
    lq.mkdir()
    for name, hw in (('a.png', (24, 40)), ('b.png', (33, 17)), ('c.png', (24, 40))):
        Image.fromarray(rng.randint(0, 256, hw + (3,)).astype(np.uint8), 'RGB').save(str(lq / name))
    ckpt = tmp_path / 'net_g.pth'
    torch.save({'params': {k: torch.from_numpy(v) for k, v in synth_weights('x4', 11, 'trained').items()}}, str(ckpt))
    saved = {}
    for tag, extra in (('plain', {}), ('threads', {'io_threads': 2})):
        root = tmp_path / tag
        opt = dict(name='pipe', model_type='FeMaSRModel', scale=4, root_path=str(root), is_train=False,
                   datasets=dict(val=dict(name='tiny', type='SingleImageDataset', dataroot_lq=str(lq), io_backend=dict(type='disk'))),
                   network_g=dict(type='FeMaSRNet', gt_resolution=256, norm_type='gn', act_type='silu', scale_factor=4,
                                  codebook_params=[[32, 1024, 512]], LQ_stage=True),
                   path=dict(pretrain_network_g=str(ckpt), strict_load=False, visualization=str(root / 'vis')),
                   val=dict(save_img=True, suffix='sr', **extra))
        model = build_model(opt)
        ds = dict(opt['datasets']['val'], phase='val', scale=4)
        loader = build_dataloader(build_dataset(ds), ds)
        model.validation(loader, 0, None, save_img=True, save_as_dir=str(root / 'flat'))
        files = {}
        for d in (root / 'vis' / 'tiny', root / 'flat'):
            for f in sorted(os.listdir(str(d))):
                files[f'{d.name}/{f}'] = d / f
        assert len(files) == 6
        saved[tag] = files
    assert sorted(saved['plain']) == sorted(saved['threads'])
    for key, f in saved['plain'].items():
        a, b = np.array(Image.open(str(f)).convert('RGB')), np.array(Image.open(str(saved['threads'][key])).convert('RGB'))
        assert a.ndim == 3 and np.array_equal(a, b), key
        assert zlib.decompress(_idat(saved['threads'][key].read_bytes())) == pngio.filter_rows(a).tobytes()      # (written by the writer)

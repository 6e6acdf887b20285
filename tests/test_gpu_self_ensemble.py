"""-m gpu: the x8 geometric self-ensemble (femasr_amd.ensemble -> femasr_dihedral_expand / _merge and their _u8 forms; FeMaSRNet.test*(...,
self_ensemble=True)).

The checker is the numpy restatement tests/ensemble_ref.py (index formulas; tests/test_self_ensemble_host.py holds it against flips and
transposes, float64 and np.rint): the kernels must reproduce it BIT FOR BIT.  The shapes bracket the kernels' 64x64 LDS tile (63, 64, 65, and
a 32x32 one: 31, 33) from one element through several tiles with ragged edges.  Expand inputs are index-valued, so a misplaced element
shows; merge inputs spread over 2^-6 .. 2^6 in magnitude, so a wrong summation order shows (the host test has the control).  The network
cases compare `self_ensemble=True` with the restatement applied to eight SEPARATE batch-1 calls on torch-transformed inputs."""
import ctypes

import numpy as np
import pytest
import torch

import ensemble_ref as R
from femasr_amd import _lib, synth, tiling
from femasr_amd import colorfix as CF
from femasr_amd import ensemble as E
from helpers import synth_weights

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(t, want):
    return t.dtype == torch.from_numpy(want).dtype and tuple(t.shape) == want.shape and np.array_equal(_bits(t), want.view(np.uint32) if want.dtype == np.float32 else want)


# --------------------------------------------------------------------------------------------------------------- 1. kernels, bit for bit
@pytest.mark.parametrize('h,w', R.SHAPES)
def test_kernels_equal_the_restatement_bitwise(cuda_device, h, w):
    for b in (1, 3):
        for c in (1, 3):
            x = R.index_f32(b, c, h, w)
            s, t = E.expand(_dev(x))
            rs, rt = R.expand(x)
            assert _same(s, rs) and _same(t, rt), ('expand', b, c)
            ys, yt = R.results_f32(b, c, h, w, seed=h * 131 + w + b + c)
            assert _same(E.merge(_dev(ys), _dev(yt)), R.merge(ys, yt)), ('merge', b, c)
        xu = R.pattern_u8(b, h, w)
        s, t = E.expand(_dev(xu))
        rs, rt = R.expand(xu)
        assert _same(s, rs) and _same(t, rt), ('expand_u8', b)
        us, ut = R.results_u8(b, h, w, seed=h * 131 + w + b)
        assert _same(E.merge(_dev(us), _dev(ut)), R.merge(us, ut)), ('merge_u8', b)


@pytest.mark.parametrize('h,w', [(65, 127), (64, 64)])
def test_round_trip(cuda_device, h, w):
    """merge(expand(x)) == x bit for bit: fp32 integer-valued below 2^20 (the eight-term sum is exact), uint8 any bytes (S = 8 x)."""
    g = torch.Generator().manual_seed(h)
    x = torch.randint(0, 1 << 20, (3, 3, h, w), generator=g).float().cuda()
    xu = torch.randint(0, 256, (3, h, w, 3), generator=g, dtype=torch.uint8).cuda()
    for a in (x, xu):
        s, t = E.expand(a)
        assert torch.equal(E.merge(s, t), a)
        if h == w:                                  # the single 8 B buffer: transposed = straight + 4 B C H W
            both = E.as_batch(s, t)
            assert both is not None and both.data_ptr() == s.data_ptr() and t.data_ptr() == s.data_ptr() + s.numel() * s.element_size()
            assert torch.equal(both[:4], s) and torch.equal(both[4:], t)
            assert torch.equal(E.merge(both[:4], both[4:]), a)
            for k in range(8):
                assert torch.equal(both[k], E.forward_variant(a, k))
        else:
            assert E.as_batch(s, t) is None


def test_forms_and_refusals(cuda_device):
    h, w = 33, 70
    x, xu = R.index_f32(2, 3, h, w), R.pattern_u8(2, h, w)
    ys, yt = R.results_f32(2, 3, h, w, 3)
    us, ut = R.results_u8(2, h, w, 4)
    dx, dxu, dys, dyt, dus, dut = (_dev(a) for a in (x, xu, ys, yt, us, ut))
    want, want8 = R.merge(ys, yt), R.merge(us, ut)
    out, out8 = torch.full((2, 3, h, w), 7.0, device='cuda'), torch.full((2, h, w, 3), 7, dtype=torch.uint8, device='cuda')
    assert E.merge(dys, dyt, out=out) is out and _same(out, want)                                 # out=
    assert E.merge(dus, dut, out=out8) is out8 and _same(out8, want8)
    st = torch.cuda.Stream(device=cuda_device)                                                    # a side stream
    st.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(st):
        s, t = E.expand(dx)
        s8, t8 = E.expand(dxu)
        m, m8 = E.merge(dys, dyt), E.merge(dus, dut)
    st.synchronize()
    assert _same(s, R.expand(x)[0]) and _same(t, R.expand(x)[1]) and _same(s8, R.expand(xu)[0]) and _same(t8, R.expand(xu)[1])
    assert _same(m, want) and _same(m8, want8)
    for d, a in ((dx, x), (dxu, xu), (dys, ys), (dyt, yt), (dus, us), (dut, ut)):                 # inputs untouched
        assert _same(d, a)
    # the host tensors take the torch definition: the same bits
    assert _same(E.merge(torch.from_numpy(ys), torch.from_numpy(yt)), want)
    # a shape at the refusal limit returns the error code without launching (the argument check only: nothing that large exists)
    lib = _lib.load()
    p = ctypes.c_void_p(dx.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.femasr_dihedral_expand(stream, p, 1, 1, 1 << 16, 1 << 15, p, p) == -1 and b'2^31' in lib.femasr_last_error()
    assert lib.femasr_dihedral_merge(stream, p, p, 1, 1, 1 << 15, 1 << 16, p) == -1
    assert lib.femasr_dihedral_expand_u8(stream, p, 1, 1 << 16, 1 << 15, p, p) == -1
    assert lib.femasr_dihedral_merge_u8(stream, p, p, 1, 1 << 16, 1 << 15, p) == -1
    assert lib.femasr_dihedral_expand(stream, p, 0, 3, 8, 8, p, p) == -1 and lib.femasr_dihedral_expand(stream, None, 1, 3, 8, 8, p, p) == -1
    torch.cuda.synchronize()
    assert _same(dx, x)


# --------------------------------------------------------------------------------------------------------------- 2. the network
_REAL = {}


def _real(cn):
    if cn not in _REAL:
        import gpu_utils as G
        _REAL[cn] = G.build_net(cn, synth_weights(cn, 0, 'trained'))
    return _REAL[cn]


def _eight(run, x):
    """(straight, transposed) numpy results of eight separate calls per IMAGE (batch 1 each) on the torch-transformed inputs."""
    ys = [torch.cat([run(E.forward_variant(x[i:i + 1], k)) for i in range(x.shape[0])]).cpu().numpy() for k in range(8)]
    return np.stack(ys[:4]), np.stack(ys[4:])


def _inputs(b, h, w, seed=10):
    x = torch.from_numpy(synth.synth_input(seed, (b, 3, h, w))).cuda()
    return x, (x.permute(0, 2, 3, 1) * 255.0).round().clamp(0, 255).to(torch.uint8).contiguous()


@pytest.mark.parametrize('cn,h,w', [('x4', 20, 28), ('x4', 24, 24), ('x2', 20, 28), ('x2', 24, 24)])
def test_network_whole_image(cuda_device, cn, h, w):
    net = _real(cn)
    s = net.scale_factor
    x, xu8 = _inputs(2, h, w)
    want, want8 = R.merge(*_eight(net.test, x)), R.merge(*_eight(net.test_u8, xu8))
    y, y8 = net.test(x, self_ensemble=True), net.test_u8(xu8, self_ensemble=True)
    assert tuple(y.shape) == (2, 3, h * s, w * s) and _same(y, want) and _same(y8, want8)
    assert not torch.equal(y, net.test(x)) and not torch.equal(y8, net.test_u8(xu8))              # it is another image than the plain call's
    for i in range(2):                                                                            # B = 1; an image without batch axis
        assert torch.equal(net.test(x[i:i + 1], self_ensemble=True)[0], y[i]) and torch.equal(net.test_u8(xu8[i], self_ensemble=True), y8[i])
    out, out8 = torch.full_like(y, 7.0), torch.full_like(y8, 7)
    assert net.test(x, out=out, self_ensemble=True) is out and torch.equal(out, y)
    assert net.test_u8(xu8, out=out8, self_ensemble=True) is out8 and torch.equal(out8, y8)
    keep = net.max_tile_batch, net.num_streams
    try:
        net.max_tile_batch = 1                                                                    # eight (sixteen) calls of one variant
        assert torch.equal(net.test(x, self_ensemble=True), y) and torch.equal(net.test_u8(xu8, self_ensemble=True), y8)
        net.max_tile_batch = keep[0]
        net.num_streams = 3
        assert torch.equal(net.test(x, self_ensemble=True), y) and torch.equal(net.test_u8(xu8, self_ensemble=True), y8)
        net.num_streams = keep[1]
        net.use_graph = True
        assert torch.equal(net.test(x, self_ensemble=True), y)                                    # capture
        assert torch.equal(net.test(x, self_ensemble=True), y)                                    # replay
        assert net.test(x, out=out.fill_(7.0), self_ensemble=True) is out and torch.equal(out, y)
    finally:
        net.max_tile_batch, net.num_streams = keep
        net.use_graph = False
        net._graphs = {}
    # a colour fix on top comes after the merge
    assert torch.equal(net.test(x, self_ensemble=True, color_fix=True), CF.wavelet_color_fix(y, x, net.color_fix_levels))
    assert torch.equal(net.test_u8(xu8, self_ensemble=True, color_fix=True), CF.wavelet_color_fix(y8, xu8, net.color_fix_levels))


@pytest.mark.parametrize('h,w', [(20, 28), (24, 24)])
def test_network_half_precision_modes(cuda_device, h, w):
    """decoder_math='fp16' + linear_math='fp16': the ensemble of the eight calls made in those modes, the same bits for any split."""
    net = _real('x4')
    x, xu8 = _inputs(1, h, w, seed=12)
    plain_modes = net.decoder_math, net.linear_math, net.max_tile_batch
    y32 = net.test(x, self_ensemble=True)
    try:
        net.decoder_math, net.linear_math = 'fp16', 'fp16'
        want, want8 = R.merge(*_eight(net.test, x)), R.merge(*_eight(net.test_u8, xu8))
        y = net.test(x, self_ensemble=True)
        assert _same(y, want) and _same(net.test_u8(xu8, self_ensemble=True), want8) and not torch.equal(y, y32)
        net.max_tile_batch = 1
        assert torch.equal(net.test(x, self_ensemble=True), y)
    finally:
        net.decoder_math, net.linear_math, net.max_tile_batch = plain_modes


def test_network_tiled(cuda_device):
    """test_tile / test_tile_u8 at 40x52, 16/4 (edge tiles of other shapes): per-tile test(crop, self_ensemble=True) pasted by the reference
    rule; blend=True and color_fix=True on top equal the existing post-steps applied to the ensemble tiles / canvas."""
    net = _real('x4')
    x, xu8 = _inputs(1, 40, 52, seed=14)
    tiles = tiling.enumerate_tiles(40, 52, 16, 4)
    assert len({t.in_hw for t in tiles}) > 1
    want = R.paste(lambda t: net.test(x[:, :, t.y0p:t.y1p, t.x0p:t.x1p], self_ensemble=True), tiles, 4, torch.zeros(1, 3, 160, 208, device='cuda'), False)
    want8 = R.paste(lambda t: net.test_u8(xu8[:, t.y0p:t.y1p, t.x0p:t.x1p, :].contiguous(), self_ensemble=True), tiles, 4,
                    torch.zeros(1, 160, 208, 3, dtype=torch.uint8, device='cuda'), True)
    y, y8 = net.test_tile(x, 16, 4, self_ensemble=True), net.test_tile_u8(xu8, 16, 4, self_ensemble=True)
    assert torch.equal(y, want) and torch.equal(y8, want8)
    assert not torch.equal(y, net.test_tile(x, 16, 4)) and not torch.equal(y8, net.test_tile_u8(xu8, 16, 4))
    assert torch.equal(net.test_tile_u8(xu8[0], 16, 4, self_ensemble=True), y8[0])
    # the existing post-steps on the ensemble tiles: the plain tile driver around a `test` / `test_u8` that is the ensemble form
    plain, plain_u8 = net.test, net.test_u8
    try:
        net.test = lambda t, out=None: plain(t, out=out, self_ensemble=True)
        net.test_u8 = lambda t, bgr=False, out=None: plain_u8(t, bgr=bgr, out=out, self_ensemble=True)
        assert torch.equal(net.test_tile(x, 16, 4), y)
        blend, blend8 = net.test_tile(x, 16, 4, blend=True), net.test_tile_u8(xu8, 16, 4, blend=True)
    finally:
        del net.test, net.test_u8
    assert not torch.equal(blend, y)
    assert torch.equal(net.test_tile(x, 16, 4, blend=True, self_ensemble=True), blend)
    assert torch.equal(net.test_tile_u8(xu8, 16, 4, blend=True, self_ensemble=True), blend8)
    L = net.color_fix_levels
    assert torch.equal(net.test_tile(x, 16, 4, color_fix=True, self_ensemble=True), CF.wavelet_color_fix(y, x, L))
    assert torch.equal(net.test_tile_u8(xu8, 16, 4, color_fix=True, self_ensemble=True), CF.wavelet_color_fix(y8, xu8, L))
    assert torch.equal(net.test_tile(x, 16, 4, blend=True, color_fix=True, self_ensemble=True), CF.wavelet_color_fix(blend, x, L))
    from femasr_amd import distributed as fd                                                      # (no process group: the single-rank call)
    assert torch.equal(fd.test_tile_parallel(net, x, 16, 4, self_ensemble=True), y)


def test_cli(cuda_device, tmp_path):
    """--self-ensemble on both branches of the CLI: the PNGs are the `test_u8` / `test_tile_u8` results."""
    from PIL import Image
    from femasr_amd import inference
    import gpu_utils as G
    net = G.build_net('x4', synth_weights('x4', 1, 'trained'), decoder_math='fp32')              # the CLI's defaults
    u8 = (synth.synth_input(11, (1, 3, 40, 52), tag='se.png')[0].transpose(1, 2, 0) * 255).astype(np.uint8)
    img = torch.from_numpy(u8).cuda()
    src = tmp_path / 'in'
    src.mkdir()
    Image.fromarray(u8, 'RGB').save(src / 'se.png')
    common = ['-i', str(src), '-s', '4', '--synthetic-seed', '1', '--tile_size', '16', '--tile_pad', '4', '--streams', '1', '--self-ensemble']
    inference.main(common + ['-o', str(tmp_path / 'whole')])
    whole = net.test_u8(img, self_ensemble=True)
    assert np.array_equal(np.asarray(Image.open(tmp_path / 'whole' / 'se.png').convert('RGB')), whole.cpu().numpy())
    inference.main(common + ['-o', str(tmp_path / 'tiled'), '--max_size', '30'])
    tiled = net.test_tile_u8(img, 16, 4, self_ensemble=True)
    assert np.array_equal(np.asarray(Image.open(tmp_path / 'tiled' / 'se.png').convert('RGB')), tiled.cpu().numpy())
    assert not torch.equal(tiled, whole) and not torch.equal(whole, net.test_u8(img))

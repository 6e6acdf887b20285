"""DISTS on the GPU: the L2 pool and the backbone's stage maps bit for bit, the moments and the fp64 head against bounds derived from the
data, the score against the float64 definition (tests/dists_ref.py), bitwise properties, the guard arena under both poisons, and the
validation / CLI surfaces.

`python tests/test_gpu_dists.py` measures the end-to-end deviations again and writes profiles/dists_report.txt."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import yaml

if __name__ == '__main__':          # run as a script: the repository root is not on the path yet (tests/conftest.py puts it there for pytest)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import dists_ref as R
import dists_utils as U
import guard_arena as GA
from femasr_amd import _lib, synth
from femasr_amd import dists as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 7
# (B, H, W): 8x8 - the deepest maps are 1x1 (N = 1, every variance 0); 9x11 - odd sides, the pool's last window hangs over the padding;
# 17x23, 33x47 - non-square, several blocks per map
CASES = [(1, 8, 8), (2, 9, 11), (3, 17, 23), (1, 33, 47)]
UNRELATED = ('unrelated', 17, 23)      # one pair of unrelated images (a synthetic image against uniform noise): a large score


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@functools.lru_cache(maxsize=None)
def _sd():
    return synth.dists_state(SEED)


@functools.lru_cache(maxsize=None)
def _module():
    return D.DISTS(state_dict={k: torch.from_numpy(v) for k, v in _sd().items()}).cuda()


@functools.lru_cache(maxsize=None)
def _inputs(case):
    b, h, w = case
    if b == 'unrelated':
        return synth.synth_input(11, (1, 3, h, w)), synth.uniform(99, 'unrelated', (1, 3, h, w), 0.0, 1.0)
    return synth.synth_input(11, (b, 3, h, w)), synth.synth_input(12, (b, 3, h, w))


@functools.lru_cache(maxsize=None)
def _oracle_maps(case):
    """The five stage maps, NHWC (2B,h,w,C) float32: the float32 normalisation, oracle.conv2d + ReLU and the float32 pool restatement,
    chained on the host.  Computed once per case and shared (never written to)."""
    from oracle import oracle as orc
    x, y = _inputs(case)
    sd = _sd()
    cur = R.normalise_f32(np.concatenate([x, y]))
    maps = []
    for k, idx in enumerate(R.STAGES):
        if k:
            cur = R.l2pool_f32(cur)
        for i in idx:
            wt = np.ascontiguousarray(sd[f'stage{k + 1}.{i}.weight'].transpose(2, 3, 1, 0))
            ref = orc.conv2d(cur, wt, sd[f'stage{k + 1}.{i}.bias'], 3, 1, 1)
            cur = np.where(ref > 0, ref, np.float32(0)).astype(np.float32)
        cur.setflags(write=False)
        maps.append(cur)
    return tuple(maps)


def _six_maps(case):
    """([six NCHW float64 maps of x], [of y]) from the raw input and the oracle's stage maps."""
    x, y = _inputs(case)
    b = x.shape[0]
    mx, my = [torch.from_numpy(x.astype(np.float64))], [torch.from_numpy(y.astype(np.float64))]
    for f in _oracle_maps(case):
        t = torch.from_numpy(f.astype(np.float64)).permute(0, 3, 1, 2)
        mx.append(t[:b])
        my.append(t[b:])
    return mx, my


def _gpu_scores(case, per_layer=False):
    x, y = _inputs(case)
    out = _module()(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), per_layer=per_layer)
    return (out[0].cpu().numpy(), out[1].cpu().numpy()) if per_layer else out.cpu().numpy()


# ---------------------------------------------------------------- 1. the L2 pool, bit for bit
def _pool_input(c, h, w, b2, kind):
    rng = np.random.RandomState(c + 31 * h + w + b2)
    if kind == 'noise':
        f = rng.randn(b2, h, w, c).astype(np.float32)
        f[0, 0, 0, :] = 0.0
    elif kind == 'zeros':
        f = np.zeros((b2, h, w, c), np.float32)
    elif kind == 'corners':         # a single hot pixel in each corner, one corner per image (cyclic)
        f = np.zeros((b2, h, w, c), np.float32)
        for s in range(b2):
            f[s, (0, 0, h - 1, h - 1)[s % 4], (0, w - 1, 0, w - 1)[s % 4], :] = rng.rand(c).astype(np.float32) + 1
    else:                           # values near +-1e19 (q = 1e38 stays finite) and +-3e19 (q overflows to inf): inf must come out, not NaN
        f = (rng.choice([1e19, -1e19, 3e19, -3e19, 1.0], size=(b2, h, w, c)) * (1 + 0.1 * rng.rand(b2, h, w, c))).astype(np.float32)
    return f


@pytest.mark.parametrize('kind', ['noise', 'zeros', 'corners', 'huge'])
@pytest.mark.parametrize('c,h,w,b2', [(64, 1, 1, 2), (128, 2, 2, 2), (512, 3, 3, 2), (64, 8, 8, 6), (128, 9, 9, 2), (512, 17, 23, 2),
                                      (64, 17, 23, 6), (128, 2, 9, 6)])
def test_l2pool_bit_identical(cuda_device, kind, c, h, w, b2):
    f = _pool_input(c, h, w, b2, kind)
    want = R.l2pool_f32(f)
    got = GA.run_twice(lambda: U.l2pool(f), f'l2pool {kind} {(c, h, w, b2)}')
    assert got.shape == (b2, (h + 1) // 2, (w + 1) // 2, c)
    assert _bits_equal(got, want), float(np.nanmax(np.abs(got - want)))
    assert not np.isnan(got).any()
    if kind == 'zeros':
        assert np.all(got == np.sqrt(np.float32(1e-12)))
    if kind == 'huge':
        assert np.isinf(got).any() and np.isfinite(got).any()
    if kind == 'corners':
        assert (got > 0.2).sum() == b2 * c        # each corner pixel reaches exactly one output pixel


# ---------------------------------------------------------------- 2. the stage maps, bit for bit
@pytest.mark.parametrize('case', CASES)
def test_stage_maps_bit_identical_to_oracle_chain(cuda_device, case):
    x, y = _inputs(case)
    got = U.features(_module(), torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
    want = _oracle_maps(case)
    assert [g.shape for g in got] == [(2 * case[0], h, w, c) for h, w, c in D.map_shapes(case[1], case[2])[1:]]
    for k, (g, r) in enumerate(zip(got, want)):
        assert (r > 0).any(), f'stage {k + 1} is dead'
        assert _bits_equal(g, r), (k + 1, float(np.abs(g - r).max()))


# ---------------------------------------------------------------- 3. the moments: within the bound of any summation order
def _check_sums(got, fx, fy, what):
    """got (B,5,C); fx, fy (B,N,C) float32: every sum within N 2^-53 sum|terms| of the exact sum (long-double accumulation of the
    products, which are exact in float64)."""
    ax, ay = fx.astype(np.float64), fy.astype(np.float64)
    n = ax.shape[1]
    for q, t in enumerate((ax, ay, ax * ax, ay * ay, ax * ay)):
        ref = t.astype(np.longdouble).sum(1)
        bound = n * 2.0 ** -53 * np.abs(t).sum(1)
        err = np.abs(got[:, q].astype(np.longdouble) - ref).astype(np.float64)
        print(f'{what} sum {q}: max err {err.max():.3e}, bound there {bound.flat[err.argmax()]:.3e}')
        assert np.all(err <= bound), (what, q, float(err.max()))


# (C, H, W, B): one pixel; odd sides; one run and several runs of 64 pixels; a map of more than 512 * 64 pixels, where the runs grow
@pytest.mark.parametrize('c,h,w,b', [(64, 1, 1, 1), (128, 9, 11, 2), (512, 3, 5, 3), (256, 8, 8, 1), (64, 33, 47, 2), (64, 181, 200, 1)])
def test_moments_within_the_summation_bound(cuda_device, c, h, w, b):
    rng = np.random.RandomState(c + h + w)
    f = np.maximum(rng.randn(2 * b, h, w, c) + 0.5, 0).astype(np.float32)
    got = GA.run_twice(lambda: U.moments(f), f'moments {(c, h, w, b)}')
    _check_sums(got, f[:b].reshape(b, h * w, c), f[b:].reshape(b, h * w, c), f'moments {(c, h, w, b)}')


# (B, H, W): one run; two runs of 1024 pixels; an image of more than 512 * 1024 pixels, where the runs grow
@pytest.mark.parametrize('b,h,w', [(1, 8, 8), (3, 9, 11), (2, 33, 47), (1, 700, 751)])
def test_input_moments_within_the_summation_bound(cuda_device, b, h, w):
    x, y = synth.synth_input(3, (b, 3, h, w)), synth.synth_input(4, (b, 3, h, w))
    got = GA.run_twice(lambda: U.moments_input(x, y), f'moments_input {(b, h, w)}')
    _check_sums(got, x.reshape(b, 3, h * w).transpose(0, 2, 1), y.reshape(b, 3, h * w).transpose(0, 2, 1), f'moments_input {(b, h, w)}')


# ---------------------------------------------------------------- 4. the score against the fp64 statistics of the same maps
def _head_bound(mx, my, alpha, beta):
    """sum_kc (alpha + beta)_kc / w * 8 N_k 2^-53 kappa_kc, kappa = (E[x^2] + E[y^2] + c2) / (vx + vy + c2): a relative 2^-53 per term
    summation error amplified through sum^2 / N - m^2 and the quotient."""
    a, b = np.asarray(alpha, np.float64).reshape(-1), np.asarray(beta, np.float64).reshape(-1)
    w = a.sum() + b.sum()
    total, off = 0.0, 0
    for fx, fy in zip(mx, my):
        fx, fy = fx.numpy(), fy.numpy()
        c, n = fx.shape[1], fx.shape[2] * fx.shape[3]
        kappa = ((fx * fx).mean((2, 3)) + (fy * fy).mean((2, 3)) + R.C2) / (fx.var((2, 3)) + fy.var((2, 3)) + R.C2)
        total = total + ((a[off:off + c] + b[off:off + c]) / w * 8 * n * 2.0 ** -53 * kappa).sum(1)
        off += c
    return total


@pytest.mark.parametrize('case', CASES)
def test_score_against_fp64_statistics_of_the_same_maps(cuda_device, case):
    sd = _sd()
    mx, my = _six_maps(case)
    ref, ref_terms = R.score_from_maps(mx, my, sd['alpha'], sd['beta'])
    bound = _head_bound(mx, my, sd['alpha'], sd['beta'])
    got, terms = _gpu_scores(case, per_layer=True)
    print(f'{case}: score {got}, |gpu - ref| {np.abs(got - ref)}, bound {bound}')
    assert np.all(bound < 1e-9), bound          # the bound is not vacuous
    assert got.dtype == np.float64 and np.all(np.abs(got - ref) <= bound), (got - ref, bound)
    w = sd['alpha'].astype(np.float64).sum() + sd['beta'].astype(np.float64).sum()
    assert np.all(np.abs(terms - ref_terms) <= bound[:, None, None] * w)
    assert np.all(np.abs((1 - terms.sum((1, 2)) / w) - got) <= 1e-14)


# ---------------------------------------------------------------- 5. the score against the float64 definition, end to end
def _end_to_end(case):
    """(gpu, float64 definition, float32 stock-torch restatement) scores of a case."""
    x, y = _inputs(case)
    sd = _sd()
    s64, _ = R.dists(sd, x, y)
    s32, _ = R.dists(sd, x, y, dtype=torch.float32)
    return _gpu_scores(case), s64, s32


@pytest.mark.parametrize('case', CASES + [UNRELATED])
def test_score_against_the_float64_definition(cuda_device, case):
    """The only difference is float32 rounding in the features.  The float32 stock-torch restatement (float32 features, fp64 statistics)
    sits `dev` from the float64 definition; the GPU's fmaf chains are another float32 rounding of the same size: it is allowed 8 dev."""
    got, s64, s32 = _end_to_end(case)
    dev = np.abs(s32 - s64).max()
    print(f'{case}: score {s64}, |torch32 - def64| {np.abs(s32 - s64)}, |gpu - def64| {np.abs(got - s64)}, allowed {8 * dev:.3e}')
    assert 0 < dev < 1e-6
    assert np.all(np.abs(got - s64) <= 8 * dev), (np.abs(got - s64), 8 * dev)
    if case == UNRELATED:
        assert s64[0] > 0.25


# ---------------------------------------------------------------- 6. determinism
def test_bitwise_properties(cuda_device):
    m = _module()
    x, y = (torch.from_numpy(a).cuda() for a in _inputs((3, 17, 23)))
    ab, t_ab = m(x, y, per_layer=True)
    assert ab.shape == (3,) and ab.dtype == torch.float64 and t_ab.shape == (3, 6, 2)

    def same(s, t, what):
        assert torch.equal(s, ab) and torch.equal(t, t_ab), what
    for i in range(3):              # batch invariance: pair i alone == pair i inside the batch of 3
        one, t_one = m(x[i:i + 1], y[i:i + 1], per_layer=True)
        assert torch.equal(one, ab[i:i + 1]) and torch.equal(t_one, t_ab[i:i + 1]), i
    same(*m(x, y, per_layer=True), 'two runs')
    # a non-contiguous input: channels-last storage and a slice of a wider tensor
    wide = torch.zeros((3, 3, 17, 30), device='cuda')
    wide[..., 4:27] = y
    same(*m(x.contiguous(memory_format=torch.channels_last), wide[..., 4:27], per_layer=True), 'non-contiguous inputs')
    # a side stream
    side = torch.cuda.Stream(cuda_device)
    side.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(side):
        s_side, t_side = m(x, y, per_layer=True)
    torch.cuda.current_stream(cuda_device).wait_stream(side)
    same(s_side, t_side, 'side stream')
    # a caller-owned workspace
    ws = torch.empty(m.workspace_bytes(3, 17, 23), dtype=torch.uint8, device='cuda')
    same(*m(x, y, per_layer=True, workspace=ws), 'caller-owned workspace')
    with pytest.raises(ValueError, match='workspace'):
        m(x, y, workspace=ws[:-256])
    # symmetry and identity
    ba, t_ba = m(y, x, per_layer=True)
    same(ba, t_ba, 'DISTS(x, y) == DISTS(y, x)')
    xx = m(x, x)
    assert float(xx.abs().max()) <= 1e-12
    assert torch.all(ab > 1e-3)


def test_hand_captured_graph_replays(cuda_device):
    m = _module()
    x, y = (torch.from_numpy(a).cuda() for a in _inputs((2, 9, 11)))
    x2, y2 = torch.from_numpy(synth.synth_input(21, (2, 3, 9, 11))).cuda(), torch.from_numpy(synth.synth_input(22, (2, 3, 9, 11))).cuda()
    want, want2 = m(x, y).clone(), m(x2, y2).clone()
    assert not torch.equal(want, want2)
    sx, sy = x.clone(), y.clone()
    torch.cuda.synchronize(cuda_device)
    graph = torch.cuda.CUDAGraph()
    m._ws = None                                      # the graph owns its workspace
    with torch.cuda.graph(graph):
        static = m(sx, sy)
    m._ws = None
    graph.replay()
    torch.cuda.synchronize(cuda_device)
    assert torch.equal(static, want), 'first replay'
    sx.copy_(x2)
    sy.copy_(y2)
    graph.replay()
    torch.cuda.synchronize(cuda_device)
    assert torch.equal(static, want2), 'second replay, on other inputs: a launch outside the capture would have kept the first result'


# ---------------------------------------------------------------- 7. the whole forward on the guard arena
@pytest.mark.parametrize('case', [(2, 9, 11), (1, 33, 47)])
def test_forward_on_the_guard_arena(cuda_device, case):
    m = _module()
    x, y = (torch.from_numpy(a).cuda() for a in _inputs(case))
    got, terms = GA.run_twice(lambda: U.forward(m, x, y), f'dists_forward {case}')        # bit-identical between the poisons
    want, t_want = m(x, y, per_layer=True)
    assert np.array_equal(got, want.cpu().numpy()) and np.array_equal(terms, t_want.cpu().numpy())


def test_refused_before_any_launch(cuda_device):
    m = _module()
    lib, h = m._native(torch.device('cuda:0'))
    x = torch.rand((1, 3, 7, 40), device='cuda')
    with pytest.raises(_lib.FemasrError, match='>= 8'):
        m(x, x)
    out = torch.full((1,), 7.0, dtype=torch.float64, device='cuda')
    ws = torch.empty(1 << 20, dtype=torch.uint8, device='cuda')
    assert lib.femasr_dists_forward(h, None, _lib.ptr(x), _lib.ptr(x), 1, 7, 40, _lib.ptr(ws), 1 << 20, _lib.ptr(out), None) == -1
    x8 = torch.rand((1, 3, 8, 8), device='cuda')
    need = m.workspace_bytes(1, 8, 8)
    assert lib.femasr_dists_forward(h, None, _lib.ptr(x8), _lib.ptr(x8), 1, 8, 8, _lib.ptr(ws), need - 1, _lib.ptr(out), None) == -1
    torch.cuda.synchronize()
    assert out.item() == 7.0
    with pytest.raises(_lib.FemasrError, match='no CPU fallback'):
        m(x8.cpu(), x8.cpu())


# ---------------------------------------------------------------- 8. validation and CLI surfaces
def _png(path, arr):
    from PIL import Image
    Image.fromarray(arr, 'RGB').save(path)


def test_validation_reports_dists(cuda_device, tmp_path):
    from PIL import Image
    from helpers import synth_weights
    from femasr_amd import imgproc
    from femasr_amd.data import _read
    from femasr_amd.test import test_pipeline
    rng = np.random.RandomState(4)
    lq, gt, vis = tmp_path / 'lq', tmp_path / 'gt', tmp_path / 'vis'
    lq.mkdir(); gt.mkdir()
    for name, (h, w) in (('a.png', (12, 16)), ('b.png', (9, 11))):
        _png(str(lq / name), rng.randint(0, 256, (h, w, 3), dtype=np.uint8))
        _png(str(gt / name), rng.randint(0, 256, (4 * h, 4 * w, 3), dtype=np.uint8))
    ckpt = tmp_path / 'net_g.pth'
    torch.save({'params': {k: torch.from_numpy(v) for k, v in synth_weights('x4', 11, 'trained').items()}}, str(ckpt))
    dp = tmp_path / 'dists.pth'
    torch.save({k: torch.from_numpy(v) for k, v in synth.dists_state(9).items()}, str(dp))
    opt = dict(name='ds', model_type='FeMaSRModel', scale=4, root_path=str(tmp_path),
               datasets=dict(val=dict(name='tiny', type='PairedImageDataset', dataroot_lq=str(lq), dataroot_gt=str(gt),
                                      io_backend=dict(type='disk'))),
               network_g=dict(type='FeMaSRNet', gt_resolution=256, norm_type='gn', act_type='silu', scale_factor=4,
                              codebook_params=[[32, 1024, 512]], LQ_stage=True),
               path=dict(pretrain_network_g=str(ckpt), strict_load=False, visualization=str(vis)),
               val=dict(save_img=True, suffix='sr', metrics=dict(ds=dict(type='dists', better='lower', pretrained_model_path=str(dp)),
                                                                 skipped=dict(type='dists', better='lower'))))
    p = tmp_path / 'opt.yml'
    p.write_text(yaml.safe_dump(opt))
    r = test_pipeline(str(p))['tiny']
    assert r['skipped'] is None
    m = D.DISTS(pretrained_model_path=str(dp)).cuda()
    want = 0.0
    for name in ('a', 'b'):
        sr_u8 = torch.from_numpy(np.asarray(Image.open(str(vis / 'tiny' / f'{name}_sr.png')))).cuda()
        sr = imgproc.u8_to_input(sr_u8)
        g = _read(str(gt / f'{name}.png')).unsqueeze(0).cuda()
        want += m(sr, g).item()
    assert r['ds'] == want / 2 and 0 < r['ds'] < 1


def test_cli_scores_folders(cuda_device, tmp_path, capsys):
    from femasr_amd import imgproc
    from femasr_amd.dists_folder import main
    rng = np.random.RandomState(8)
    res, gt = tmp_path / 'res', tmp_path / 'gt'
    res.mkdir(); gt.mkdir()
    imgs = {}
    for name, (h, w) in (('x1', (40, 52)), ('x2', (33, 31))):
        g, r = rng.randint(0, 256, (h, w, 3), dtype=np.uint8), rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
        _png(str(gt / f'{name}.png'), g)
        _png(str(res / f'{name}_out.png'), r)
        imgs[name] = (g, r)
    dp = tmp_path / 'dists.pth'
    torch.save({'params': {'module.' + k: torch.from_numpy(v) for k, v in synth.dists_state(3).items()}}, str(dp))
    main(['-r', str(res), '-g', str(gt), '-w', str(dp), '--suffix', '_out'])
    lines = capsys.readouterr().out.strip().splitlines()
    m = D.DISTS(pretrained_model_path=str(dp)).cuda()
    vals = [m(imgproc.u8_to_input(torch.from_numpy(r).cuda()), imgproc.u8_to_input(torch.from_numpy(g).cuda())).item()
            for g, r in imgs.values()]
    assert len(lines) == 3
    for i, (name, v) in enumerate(zip(imgs, vals)):
        assert lines[i].split()[1] == name and lines[i].endswith(f'DISTS: {v:.6f}.')
    assert lines[2] == f'Average: DISTS: {sum(vals) / 2:.6f}'


def write_report(path=os.path.join(ROOT, 'profiles', 'dists_report.txt')):
    """The end-to-end figures of test_score_against_the_float64_definition and the head bound of
    test_score_against_fp64_statistics_of_the_same_maps, measured on this machine's GPU."""
    sd = _sd()
    lines = ['DISTS on the GPU against the float64 definition (tests/test_gpu_dists.py, synth.dists_state(%d)); one line per pair' % SEED,
             'case            score(def64)    |torch32-def64|  |gpu-def64|   allowed(8x case max)  |gpu-fp64 head of same maps|  head bound']
    for case in CASES + [UNRELATED]:
        got, s64, s32 = _end_to_end(case)
        mx, my = _six_maps(case)
        ref, _ = R.score_from_maps(mx, my, sd['alpha'], sd['beta'])
        bound = _head_bound(mx, my, sd['alpha'], sd['beta'])
        dev = np.abs(s32 - s64).max()
        for i in range(len(got)):
            lines.append(f'{str(case):15} {s64[i]:.12f}  {abs(s32[i] - s64[i]):.3e}        {abs(got[i] - s64[i]):.3e}     {8 * dev:.3e}'
                         f'             {abs(got[i] - ref[i]):.3e}                    {bound[i]:.3e}')
    with open(path, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    return lines


if __name__ == '__main__':
    print('\n'.join(write_report()))

"""Code-usage statistics (femasr_amd/codebook.py, femasr_amd/codebook_stats.py) on the host: the torch.bincount definition of `usage`
against numpy, perplexity, the reproducible sampling, the new C-ABI symbols, and the CLI's parsing and output schema with a stubbed net.
(One test at the end is marked gpu: the kernel's counts against the host definition on the same tensors.)"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from femasr_amd import _lib, codebook, codebook_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = -1        # FEMASR_ERR_INVALID of include/femasr_hip.h
NEW_SYMBOLS = ('femasr_encode_workspace_bytes', 'femasr_encode', 'femasr_index_histogram_workspace_bytes', 'femasr_index_histogram')


def test_usage_host_equals_numpy_bincount():
    rng = np.random.default_rng(0)
    for shape, n_e in [((1, 1, 4, 4), 16), ((3, 1, 8, 6), 1024), ((2, 5), 2), ((7,), 1), ((4, 1, 16, 16), 20000)]:
        a = rng.integers(0, n_e, shape, dtype=np.int64)
        t = torch.from_numpy(a)
        got = codebook.usage(t, n_e)
        assert got.dtype == torch.int64 and tuple(got.shape) == (n_e,)
        assert np.array_equal(got.numpy(), np.bincount(a.reshape(-1), minlength=n_e))
        per = codebook.usage(t, n_e, per_image=True) if a.ndim > 1 else None
        if per is not None:
            assert per.dtype == torch.int64 and tuple(per.shape) == (shape[0], n_e)
            ref = np.stack([np.bincount(a[i].reshape(-1), minlength=n_e) for i in range(shape[0])])
            assert np.array_equal(per.numpy(), ref) and np.array_equal(per.sum(0).numpy(), got.numpy())
    # a non-contiguous view counts its own elements
    a = rng.integers(0, 8, (4, 6), dtype=np.int64)
    assert np.array_equal(codebook.usage(torch.from_numpy(a)[:, ::2], 8).numpy(), np.bincount(a[:, ::2].reshape(-1), minlength=8))


@pytest.mark.parametrize('bad', [-1, 'n_e', 2 ** 32 + 5, -2 ** 63])
def test_usage_refuses_indices_out_of_range(bad):
    n_e = 1024
    a = np.arange(64, dtype=np.int64).reshape(2, 32)
    a[1, 7] = n_e if bad == 'n_e' else bad
    with pytest.raises(ValueError, match=r'1 of 64 indices are outside \[0, 1024\)'):
        codebook.usage(torch.from_numpy(a), n_e)
    counts, invalid = codebook.usage_counts(torch.from_numpy(a), n_e, per_image=True)
    assert invalid.tolist() == [0, 1] and int(counts.sum()) == 63 and int(counts[1, 39]) == 0      # in no bin (not code 5 either)
    assert int(counts[:, 5].sum()) == 1
    with pytest.raises(ValueError):
        codebook.usage(torch.from_numpy(a).to(torch.int32), n_e)
    with pytest.raises(ValueError):
        codebook.usage(torch.zeros(0, dtype=torch.int64), n_e)
    with pytest.raises(ValueError):
        codebook.usage(torch.from_numpy(a), 0)


def test_perplexity():
    for n_e in (1, 2, 1024):
        assert abs(codebook.perplexity(np.full(n_e, 7)) - n_e) <= 1e-9 * n_e
        one = np.zeros(n_e, np.int64)
        one[n_e // 2] = 123
        assert codebook.perplexity(one) == 1.0
    c = np.array([0, 3, 0, 1, 0], np.int64)
    p = np.array([0.75, 0.25])
    want = float(np.exp(-(p * np.log(p)).sum()))
    got = codebook.perplexity(torch.from_numpy(c))
    assert isinstance(got, float) and np.isfinite(got) and abs(got - want) < 1e-12
    both = codebook.perplexity(np.stack([c, np.full(5, 2)]))
    assert both.dtype == np.float64 and both.shape == (2,) and abs(both[0] - want) < 1e-12 and abs(both[1] - 5.0) < 1e-12
    assert codebook.perplexity(np.zeros(4)) == 1.0
    with pytest.raises(ValueError):
        codebook.perplexity(np.array([1, -1]))


def test_sample_index_maps():
    c = np.zeros(1024, np.int64)
    c[[3, 500, 1023]] = [10, 1, 5]
    a = codebook.sample_index_maps(c, 6, latent=8, seed=4)
    b = codebook.sample_index_maps(torch.from_numpy(c), 6, latent=8, seed=4)
    assert a.dtype == np.int64 and a.shape == (6, 1, 8, 8) and np.array_equal(a, b)
    assert set(np.unique(a)) <= {3, 500, 1023} and 3 in a
    assert not np.array_equal(a, codebook.sample_index_maps(c, 6, latent=8, seed=5))
    assert codebook.sample_index_maps(c, 2, latent=3).shape == (2, 1, 3, 3)
    assert np.array_equal(a, np.random.default_rng(4).choice(1024, size=(6, 1, 8, 8), p=c / c.sum()))
    with pytest.raises(ValueError):
        codebook.sample_index_maps(np.zeros(8), 1)


def test_new_symbols_declared_bound_and_version_kept():
    assert '#include "femasr_hip_encode.h"' in open(os.path.join(ROOT, 'include', 'femasr_hip.h')).read()      # part of the interface
    hdr = open(os.path.join(ROOT, 'include', 'femasr_hip_encode.h')).read()
    assert set(re.findall(r'^int\s+(femasr_[a-z0-9_]+)\s*\(', hdr, re.M)) == set(_lib.ENCODE_SIGNATURES) == set(NEW_SYMBOLS)
    ct = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'size_t': ctypes.c_size_t}
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        m = re.search(r'^int\s+' + name + r'\s*\(([^;]*)\)\s*;', hdr, re.M | re.S)
        assert m, f'{name} is not declared in include/femasr_hip_encode.h'
        want = []
        for arg in m.group(1).replace('\n', ' ').split(','):
            arg = arg.strip()
            if '*' in arg:
                want.append(ctypes.POINTER(ctypes.c_size_t) if arg.startswith('size_t *') else ctypes.c_void_p)
            else:
                want.append(ct[arg.rsplit(' ', 1)[0].replace('const ', '').strip()])
        res, args = _lib.ENCODE_SIGNATURES[name]
        assert res is ctypes.c_int and list(args) == want, (name, args, want)
        assert list(getattr(lib, name).argtypes) == want
    assert lib.femasr_version() == _lib.ABI_VERSION == 107


def test_the_new_size_queries_size_guarded_regions():
    """As tests/test_guard_arena_host.py asks of the queries of femasr_hip.h: the two size queries of femasr_hip_encode.h are asked through
    gpu_utils.qp by the guarded wrappers of tests/encode_utils.py."""
    queries = {n for n in _lib.ENCODE_SIGNATURES if n.endswith('_bytes')}
    assert queries == {'femasr_encode_workspace_bytes', 'femasr_index_histogram_workspace_bytes'}
    with open(os.path.join(ROOT, 'tests', 'encode_utils.py')) as fh:
        asked = set(re.findall(r"\bqp\('(femasr_\w+)'", fh.read()))
    assert asked == queries


def test_histogram_refusals_need_no_gpu():
    """Everything femasr_index_histogram refuses is refused before any launch - so also on a machine without a GPU."""
    lib = _lib.load()
    n = ctypes.c_size_t(0)
    assert lib.femasr_index_histogram_workspace_bytes(1, 1, 1, ctypes.byref(n)) == 0 and n.value == 8
    assert lib.femasr_index_histogram_workspace_bytes(2, 100003, 1024, ctypes.byref(n)) == 0 and n.value % (2 * 1025 * 4) == 0
    assert lib.femasr_index_histogram_workspace_bytes(1, 10, 65536, ctypes.byref(n)) == 0
    for g, m, n_e in [(0, 5, 4), (1, 0, 4), (1, 5, 0), (-1, 5, 4), (1, 5, (1 << 20) + 1)]:
        assert lib.femasr_index_histogram_workspace_bytes(g, m, n_e, ctypes.byref(n)) == ERR_INVALID, (g, m, n_e)
    assert lib.femasr_index_histogram_workspace_bytes(1, 5, 4, None) == ERR_INVALID
    p = ctypes.c_void_p(4096)
    for args in [(None, None, 1, 8, 4, p, p, p, 1 << 20), (None, p, 1, 8, 4, None, p, p, 1 << 20), (None, p, 1, 8, 4, p, None, p, 1 << 20),
                 (None, p, 1, 8, 4, p, p, None, 1 << 20), (None, p, 1, 8, 4, p, p, p, 19),         # (1 block x 5 words = 20 bytes)
                 (None, p, 0, 8, 4, p, p, p, 1 << 20), (None, p, 1, 0, 4, p, p, p, 1 << 20), (None, p, 1, 8, 0, p, p, p, 1 << 20)]:
        assert lib.femasr_index_histogram(*args) == ERR_INVALID, args


class _StubNet:
    """What codebook_stats.class_usage reads of a FeMaSRNet, on the host: the index of a token is a function of its pixels."""
    LQ_stage, max_depth, _cb = False, 3, [(32, 16, 4)]

    def __init__(self):
        self.seen = []

    def encode_indices(self, x, pad=False):
        assert not pad and x.shape[2] % 8 == 0 and x.shape[3] % 8 == 0
        self.seen.append(tuple(x.shape))
        v = torch.nn.functional.avg_pool2d(x.mean(1, keepdim=True), 8)
        return [(v * 15.999).to(torch.int64)]


def _png(path, arr):
    from PIL import Image
    Image.fromarray(arr, 'RGB').save(path)


def test_cli_parsing_listing_and_usage_schema(tmp_path):
    a = codebook_stats.build_parser().parse_args(['-i', 'x', '--synthetic-seed', '1', '-o', 'y'])
    assert (a.input, a.output, a.synthetic_seed, a.weight, a.lq_stage, a.out_scale) == ('x', 'y', 1, None, False, 4)
    assert (a.max_per_class, a.samples, a.latent, a.seed, a.reconstruct) == (None, 32, 8, 0, False)
    a = codebook_stats.build_parser().parse_args(['-i', 'x', '-w', 'm.pth', '--lq-stage', '-s', '2', '--max-per-class', '3', '--samples', '4',
                                                  '--latent', '5', '--seed', '6', '--reconstruct'])
    assert (a.weight, a.lq_stage, a.out_scale, a.max_per_class, a.samples, a.latent, a.seed, a.reconstruct) == ('m.pth', True, 2, 3, 4, 5, 6, True)
    with pytest.raises(SystemExit):
        codebook_stats.build_parser().parse_args(['-i', 'x', '-s', '3'])
    rng = np.random.default_rng(2)
    for cls, sizes in (('grass', [(16, 24), (19, 30), (8, 8)]), ('sky', [(24, 16)])):
        os.makedirs(tmp_path / 'in' / cls)
        for i, (h, w) in enumerate(sizes):
            _png(str(tmp_path / 'in' / cls / f'{i}.png'), rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    (tmp_path / 'in' / 'empty').mkdir()
    classes = codebook_stats.list_classes(str(tmp_path / 'in'), max_per_class=2)
    assert [(c, [os.path.basename(p) for p in ps]) for c, ps in classes] == [('grass', ['0.png', '1.png']), ('sky', ['0.png'])]
    flat = codebook_stats.list_classes(str(tmp_path / 'in' / 'grass'))
    assert [c for c, _ in flat] == ['grass'] and len(flat[0][1]) == 3
    with pytest.raises(SystemExit):
        codebook_stats.list_classes(str(tmp_path / 'in' / 'empty'))
    net, lines = _StubNet(), []
    stats = codebook_stats.class_usage(net, classes, device='cpu', log=lines.append)
    assert net.seen == [(1, 3, 16, 24), (1, 3, 16, 24), (1, 3, 24, 16)]          # 19x30 cropped to 16x24
    assert len(lines) == 1 and 'cropped' in lines[0] and 'multiple of 8' in lines[0]
    z0 = codebook_stats.write_usage(str(tmp_path / 'out'), stats)
    z = dict(np.load(str(tmp_path / 'out' / 'usage.npz'), allow_pickle=False))
    assert set(z) == set(z0) == {'classes', 'images', 'n_e', 'counts_0', 'tokens_0', 'codes_used_0', 'perplexity_0'}
    assert z['classes'].tolist() == ['grass', 'sky'] and z['images'].tolist() == [2, 1] and z['n_e'].tolist() == [16]
    assert z['counts_0'].dtype == np.int64 and z['counts_0'].shape == (2, 16) and z['tokens_0'].tolist() == [12, 6]
    assert np.array_equal(z['codes_used_0'], (z['counts_0'] > 0).sum(1)) and z['perplexity_0'].dtype == np.float64
    assert np.allclose(z['perplexity_0'], [codebook.perplexity(z['counts_0'][i]) for i in range(2)], rtol=0, atol=1e-12)
    rows = open(str(tmp_path / 'out' / 'usage.csv')).read().strip().splitlines()
    assert rows[0] == 'class,codebook,n_e,images,tokens,codes_used,perplexity' and len(rows) == 3 and rows[1].startswith('grass,0,16,2,12,')
    g = codebook_stats.texture_grid(torch.arange(3 * 3 * 4 * 4, dtype=torch.float32).reshape(3, 3, 4, 4), nrow=2)
    assert tuple(g.shape) == (3, 2 * 6 + 2, 2 * 6 + 2) and float(g.min()) == 0.0 and float(g.max()) == 1.0 and float(g[0, 0, 0]) == 0.0


@pytest.mark.gpu
def test_kernel_counts_equal_the_host_definition(cuda_device):
    rng = np.random.default_rng(3)
    for shape, n_e in [((3, 1, 9, 7), 1024), ((2, 4097), 1025), ((1, 100003), 20000)]:
        a = rng.integers(0, n_e, shape, dtype=np.int64)
        a.reshape(-1)[::13] = n_e - 1
        t = torch.from_numpy(a)
        for per in (False, True):
            h, d = codebook.usage(t, n_e, per_image=per), codebook.usage(t.to(cuda_device), n_e, per_image=per)
            assert d.device.type == 'cuda' and d.dtype == torch.int64 and torch.equal(d.cpu(), h)
    bad = torch.from_numpy(np.array([[0, 5, 2 ** 32 + 5, -1]], dtype=np.int64)).to(cuda_device)
    with pytest.raises(ValueError, match='2 of 4'):
        codebook.usage(bad, 1024)

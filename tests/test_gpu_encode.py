"""-m gpu: the network as an encoder (FeMaSRNet.encode_indices / encode_indices_u8, femasr_encode) and the code-usage histogram
(femasr_index_histogram, femasr_amd.codebook.usage).

  * the index maps are the bits `forward` / `test_with_all_indices` return - every config, batch, stream count and linear arithmetic,
    eagerly and from a hand-captured graph - and pass the near-tie rule against the recorded reference goldens;
  * nothing behind the last lookup runs: the slots only the decoder side launches into stay empty, fewer launches, no more workspace;
  * femasr_encode between guard bands under both poisons, and its refusal of a workspace one byte short before any launch;
  * the histogram between guard bands, exact against numpy.bincount, with out-of-range indices counted apart on all 64 bits.

Sizes: the goldens' small inputs, plus one per config whose mirror pad (LQ nets) is needed in rows and columns and is not square."""
import ctypes

import numpy as np
import pytest
import torch

import encode_utils as EU
import guard_arena as GA
import gpu_utils as G
from femasr_amd import _lib, codebook, imgproc, synth
from helpers import cfg_name_of, check_indices_near_tie, golden_cfg, load_golden, synth_weights, weights_from_arch

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_WORKSPACE = -1, -4        # include/femasr_hip.h
# config -> (golden, pad: test()'s geometry, the extra size).  x4 / x4mc: wsz 16, 17x26 -> 32x32; x2: wsz 32, 33x46 -> 64x64
CASES = {'hq': ('hq_small_trained', False, (24, 40)), 'hq2': ('hq2_small_trained', False, (24, 40)),
         'x4': ('x4_small_trained', True, (17, 26)), 'x2': ('x2_small_trained', True, (33, 46)),
         'x4mc': ('x4mc_small_trained', True, (17, 26))}
_NETS = {}


def _net(cfg, device):
    """(net, golden, golden input) of a config, built once per session; modes reset to the tests' defaults on every call."""
    if cfg not in _NETS:
        g = load_golden(CASES[cfg][0])
        x = synth.synth_input(int(g['input_seed']), tuple(int(v) for v in g['in_shape']))
        if 'codebook_params' in g:          # the two-codebook goldens carry their constructor arguments
            from femasr_amd.archs import build_network
            c = golden_cfg(g)
            w = weights_from_arch(c, int(g['seed']), str(g['codebook']), str(g['variant']))
            net = build_network(dict(type='FeMaSRNet', **c))
            net.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
            net = net.to(device).eval()
        else:
            cn = cfg_name_of(g)
            net = G.build_net(cn, synth_weights(cn, int(g['seed']), str(g['codebook'])), device)
        _NETS[cfg] = (net, g, x)
    net, g, x = _NETS[cfg]
    net.decoder_math, net.linear_math, net.num_streams, net.use_graph = 'fp32_strict', 'bf16_split', 1, False
    return net, g, x


def _full(net, x, pad):
    """The parent's way to the indices: the whole forward."""
    return net.test_with_all_indices(x)[1] if pad else net(x)[3]


def _inputs(cfg, x_golden, device):
    """The golden's input, and batches of 1 and 3 at the golden's size and at the config's extra size."""
    hw = tuple(x_golden.shape[2:])
    xs = [torch.from_numpy(x_golden).to(device)]
    for i, (b, (h, w)) in enumerate([(3, hw), (1, CASES[cfg][2]), (3, CASES[cfg][2])]):
        xs.append(torch.from_numpy(synth.synth_input(50 + i, (b, 3, h, w))).to(device))
    return xs


def _ws_bytes(net, x, pad):
    lib, h = net._native(x.device)
    b, _, hh, ww = x.shape
    enc, full = ctypes.c_size_t(), ctypes.c_size_t()
    _lib.check(lib.femasr_encode_workspace_bytes(h, b, hh, ww, int(pad), ctypes.byref(enc)))
    _lib.check(lib.femasr_workspace_bytes(h, b, hh, ww, int(pad), ctypes.byref(full)))
    return enc.value, full.value


@pytest.mark.parametrize('cfg', list(CASES))
def test_encode_indices_are_the_bits_of_the_forward(cuda_device, cfg):
    net, g, xg = _net(cfg, cuda_device)
    pad = CASES[cfg][1]
    xs = _inputs(cfg, xg, cuda_device)
    n_maps = len(net._cb)
    for linear_math in ('bf16_split', 'fp32', 'fp16'):
        net.linear_math = linear_math
        for streams in (1, 3):
            net.num_streams = streams
            for x in xs:
                what = f'{cfg} {tuple(x.shape)} {linear_math} streams {streams}'
                ref = _full(net, x, pad)
                got = net.encode_indices(x, pad=pad)
                assert len(got) == len(ref) == n_maps, what
                for k in range(n_maps):
                    assert got[k].dtype == torch.int64 and got[k].shape == ref[k].shape and got[k].dim() == 4 and got[k].shape[1] == 1, what
                    assert torch.equal(got[k], ref[k]), f'{what}: map {k}: {int((got[k] != ref[k]).sum())} of {ref[k].numel()} indices differ'
                enc, full = _ws_bytes(net, x, pad)
                assert 0 < enc <= full, (what, enc, full)
    # use_graph does not change the call (it runs eagerly and captures nothing), and decoder_math cannot change an index
    net, _, _ = _net(cfg, cuda_device)
    want = net.encode_indices(xs[1], pad=pad)
    net.use_graph = True
    again = net.encode_indices(xs[1], pad=pad)
    assert not net._graphs and all(torch.equal(a, b) for a, b in zip(again, want))
    net.use_graph = False
    net.decoder_math = 'fp32_direct'
    assert all(torch.equal(a, b) for a, b in zip(net.encode_indices(xs[1], pad=pad), want))


@pytest.mark.parametrize('cfg', list(CASES))
def test_encode_indices_against_the_reference_goldens(cuda_device, cfg):
    """The recorded reference indices, under the near-tie rule of the existing network tests (every map; a single-codebook golden has no
    mismatch at all, as test_gpu_network.py asserts of the forward)."""
    net, g, xg = _net(cfg, cuda_device)
    maps = net.encode_indices(torch.from_numpy(xg).to(cuda_device), pad=CASES[cfg][1])
    bad = acc = 0
    for q, m in enumerate(maps):
        pre = 'vq_' if q == 0 else f'vq{q}_'
        sub = {'vq_indices': g[pre + 'indices'], 'vq_d_best': g[pre + 'd_best'], 'vq_d_second': g[pre + 'd_second'], 'vq_idx_second': g[pre + 'idx_second']}
        assert tuple(m.shape) == sub['vq_indices'].shape
        b, a = check_indices_near_tie(m.cpu().numpy(), sub)
        bad, acc = bad + b, acc + a
    print(f'{cfg}: {bad} index mismatches vs the reference, {acc} near-ties')
    assert bad == acc, f'{bad} index mismatches, only {acc} are documented near-ties'
    if len(maps) == 1:
        assert bad == 0


def test_encode_indices_u8(cuda_device):
    net, _, _ = _net('x4', cuda_device)
    rng = np.random.default_rng(5)
    for (b, h, w, streams) in [(1, 24, 40, 1), (3, 17, 26, 3)]:
        net.num_streams = streams
        img = torch.from_numpy(rng.integers(0, 256, (b, h, w, 3), dtype=np.uint8)).to(cuda_device)
        for bgr in (False, True):
            want = net.encode_indices(torch.cat([imgproc.u8_to_input(img[i], bgr=bgr) for i in range(b)]), pad=True)
            got = net.encode_indices_u8(img, bgr=bgr)
            assert len(got) == 1 and torch.equal(got[0], want[0]), (b, h, w, bgr)
            assert torch.equal(net.encode_indices_u8(img[0], bgr=bgr)[0], want[0][:1])
            assert torch.equal(got[0], net.test_with_all_indices(torch.cat([imgproc.u8_to_input(img[i], bgr=bgr) for i in range(b)]))[1][0])
        assert not torch.equal(net.encode_indices_u8(img, bgr=False)[0], net.encode_indices_u8(img, bgr=True)[0])
    hq, _, _ = _net('hq', cuda_device)
    img = torch.from_numpy(rng.integers(0, 256, (24, 40, 3), dtype=np.uint8)).to(cuda_device)
    assert torch.equal(hq.encode_indices_u8(img, pad=False)[0], hq.encode_indices(imgproc.u8_to_input(img))[0])


def test_encode_errors_are_those_of_the_neighbours(cuda_device):
    net, _, xg = _net('x4', cuda_device)
    with pytest.raises(ValueError):
        net.encode_indices(torch.zeros(3, 24, 40, device=cuda_device))
    with pytest.raises(ValueError):
        net.encode_indices(torch.zeros(1, 4, 24, 40, device=cuda_device))
    with pytest.raises(_lib.FemasrError):
        net.encode_indices(torch.from_numpy(xg))
    with pytest.raises(_lib.FemasrError):
        net.encode_indices_u8(torch.zeros(24, 40, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        net.encode_indices_u8(torch.zeros(24, 40, 3, device=cuda_device))
    with pytest.raises(ValueError):
        net.encode_indices_u8(torch.zeros(24, 40, 4, dtype=torch.uint8, device=cuda_device))
    with pytest.raises(_lib.FemasrError):          # smaller than its mirror pad: the geometry's own refusal
        net.encode_indices(torch.zeros(1, 3, 4, 40, device=cuda_device), pad=True)
    lib, h = net._native(cuda_device)
    x = torch.from_numpy(xg).to(cuda_device)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=cuda_device)
    assert lib.femasr_encode(h, None, _lib.ptr(x), 0, 0, 1, 24, 40, 1, None, _lib.ptr(ws), ws.numel()) == ERR_INVALID     # indices are required


def test_encode_captured_by_hand_with_streams(cuda_device):
    """One call captured in torch.cuda.graph with three sub-batch streams, replayed on new inputs."""
    net, _, xg = _net('x4', cuda_device)
    net.num_streams = 3
    new = [torch.from_numpy(synth.synth_input(70 + i, (3, 3, 17, 26))).to(cuda_device) for i in range(3)]
    want = [[m.clone() for m in net.encode_indices(x, pad=True)] for x in new]
    xs = new[0].clone()
    torch.cuda.synchronize(cuda_device)
    graph = torch.cuda.CUDAGraph()
    net._ws = None                                   # the graph owns its workspace (as FeMaSRNet._run captures the forward)
    with torch.cuda.graph(graph):
        static = net.encode_indices(xs, pad=True)
    net._ws = None
    for x, w in zip(new[1:], want[1:]):
        xs.copy_(x)
        graph.replay()
        torch.cuda.synchronize(cuda_device)
        assert torch.equal(static[0], w[0])
    assert not torch.equal(want[1][0], want[2][0])
    del graph


def _launches(net, fn):
    net.enable_profile(True)
    fn()
    torch.cuda.synchronize()
    prof = {k: v[1] for k, v in net.profile().items()}
    net.enable_profile(False)
    return prof


def test_the_decoder_is_gone(cuda_device):
    """Profiled launches per slot of decode_indices (D), encode_indices (E) and test_with_all_indices (F) on x4.  The slots in which the
    decoder side alone launches - D records launches, the encoder call E does not - must be slots the whole forward F does launch into
    (so the set is about this network, not empty), and E must be a part of F in every slot.  (E's zero in those slots is the statement; the
    set is computed from the two profiles, no kernel is named.)"""
    net, _, xg = _net('x4', cuda_device)
    net.decoder_math = 'fp32'                      # the product default: Winograd forms behind the lookup
    x = torch.from_numpy(xg).to(cuda_device)
    idx = net.test_with_all_indices(x)[1]
    D = _launches(net, lambda: net.decode_indices(idx[0]))
    E = _launches(net, lambda: net.encode_indices(x, pad=True))
    F = _launches(net, lambda: net.test_with_all_indices(x))
    decoder_only = {s for s in D if D[s] > 0 and E.get(s, 0) == 0}
    shared = {s for s in D if E.get(s, 0) > 0}
    print(f'decoder-only slots: {sorted(decoder_only)}; slots both sides use: {sorted(shared)}')
    assert decoder_only, 'decode_indices launches into no slot that encode_indices leaves empty'
    assert all(F.get(s, 0) >= D[s] for s in decoder_only), (D, F)
    # the decoder's convs, not a side kernel: each has at most one GroupNorm launch in front of it, and those slots are shared
    assert 3 * sum(D[s] for s in decoder_only) >= sum(D.values()), (D, E)
    assert all(E[s] <= F.get(s, 0) for s in E), (E, F)
    assert sum(E.values()) < sum(F.values())
    assert sum(F.values()) - sum(E.values()) >= sum(D[s] for s in decoder_only)


@pytest.mark.parametrize('cfg', ['x4', 'hq2'])
def test_femasr_encode_between_guard_bands(cuda_device, cfg):
    net, _, xg = _net(cfg, cuda_device)
    pad = CASES[cfg][1]
    for b, streams in ((1, 1), (3, 1), (3, 3)):
        net.num_streams = streams
        x = torch.from_numpy(synth.synth_input(60 + b, (b, 3) + CASES[cfg][2])).to(cuda_device)
        want = net.encode_indices(x, pad=pad)

        def run():
            rc, maps = EU.encode(net, x, int(pad))
            _lib.check(rc)
            return maps
        maps = GA.run_twice(run, f'femasr_encode {cfg} B {b} streams {streams}')
        for k, m in enumerate(maps):
            assert np.array_equal(m, want[k].cpu().numpy())
        rc, maps = EU.encode(net, x, int(pad), ws_short=1)           # (guards checked inside)
        assert rc == ERR_WORKSPACE
        assert all((m == -1).all() for m in maps), 'a launch wrote indices although the workspace was refused'


HIST_SHAPES = [(1, 1), (1, 63), (1, 64), (1, 65), (3, 4097), (2, 100003)]
HIST_NE = [1, 2, 1024, 1025, 20000]
PLANTED = [-1, None, 2 ** 32 + 5, -2 ** 63]         # None: n_e itself


def _hist_ref(a, n_e):
    ok = (a >= 0) & (a < n_e)
    return np.stack([np.bincount(r[m], minlength=n_e) for r, m in zip(a, ok)]).astype(np.int64), (~ok).sum(1).astype(np.int64)


def _hist_check(a, n_e, offset8=False):
    what = f'index_histogram {a.shape} n_e {n_e}{" +8" if offset8 else ""}'
    counts, invalid = GA.run_twice(lambda: EU.index_histogram(a, n_e, offset8), what)
    rc, ri = _hist_ref(a, n_e)
    assert counts.dtype == np.int64 and np.array_equal(counts, rc), what
    assert np.array_equal(invalid, ri), (what, invalid, ri)
    assert np.array_equal(counts.sum(1) + invalid, np.full(a.shape[0], a.shape[1])), what


@pytest.mark.parametrize('content', ['one_code', 'ramp', 'random', 'planted'])
def test_index_histogram_exact(cuda_device, content):
    rng = np.random.default_rng(9)
    for n_e in HIST_NE:
        shapes = HIST_SHAPES + ([(1, n_e), (2, n_e)] if content == 'ramp' else [])       # (g, n_e): every code exactly once per group
        for g, m in shapes:
            if content == 'one_code':
                a = np.full((g, m), n_e - 1 if (g + m) % 2 else n_e // 2, np.int64)
            elif content == 'ramp':
                a = ((np.arange(g * m, dtype=np.int64).reshape(g, m) + 3 * np.arange(g)[:, None]) % n_e).astype(np.int64)
            else:
                a = rng.integers(0, n_e, (g, m), dtype=np.int64)
            if content == 'planted':
                pos = rng.permutation(m)[:min(m, 4 + m // 50)]
                for grp in range(g):
                    for j, p in enumerate(pos):
                        v = PLANTED[(j + grp) % 4]
                        a[grp, p] = n_e if v is None else v
            _hist_check(a, n_e)
            if content == 'ramp' and m == n_e:
                assert (_hist_ref(a, n_e)[0] == 1).all()
    if content in ('random', 'planted'):            # a slice whose base is on 8 but not on 16 bytes
        for g, m, n_e in [(1, 63, 1024), (1, 64, 2), (3, 4097, 1025), (2, 100003, 20000)]:
            a = rng.integers(0, n_e, (g, m), dtype=np.int64)
            if content == 'planted':
                a[:, ::7] = np.array([PLANTED[0], n_e, PLANTED[2], PLANTED[3]], np.int64)[np.arange(a[:, ::7].shape[1]) % 4]
            _hist_check(a, n_e, offset8=True)


def test_index_histogram_refusals_touch_nothing(cuda_device):
    lib = _lib.load()
    g, m, n_e = 2, 100, 16
    a = np.random.default_rng(1).integers(0, n_e, (g, m), dtype=np.int64)
    need = G.qp('femasr_index_histogram_workspace_bytes', g, m, n_e)
    ops = G.Operands('index_histogram refusals').inp('idx', a).out('counts', 8 * g * n_e).out('invalid', 8 * g).scratch('ws', need).build()
    i, c, v, w = ops.p('idx'), ops.p('counts'), ops.p('invalid'), ops.p('ws')
    for args in [(i, 0, m, n_e, c, v, w, need), (i, g, 0, n_e, c, v, w, need), (i, g, m, 0, c, v, w, need), (i, -1, m, n_e, c, v, w, need),
                 (i, g, m, (1 << 20) + 1, c, v, w, need), (None, g, m, n_e, c, v, w, need), (i, g, m, n_e, None, v, w, need),
                 (i, g, m, n_e, c, None, w, need), (i, g, m, n_e, c, v, None, need), (i, g, m, n_e, c, v, w, need - 1)]:
        assert lib.femasr_index_histogram(None, *args) == ERR_INVALID, args
        ops.check(f'refusal {args[1:4]}')
    assert (ops.get('counts', torch.int64) == -1).all() and (ops.get('invalid', torch.int64) == -1).all()
    n = ctypes.c_size_t()
    assert lib.femasr_index_histogram_workspace_bytes(1, 1, 65536, ctypes.byref(n)) == 0           # n_e up to 65536 (and beyond) is served
    assert lib.femasr_index_histogram(None, *(i, g, m, n_e, c, v, w, need)) == 0
    ops.check('the accepted call')
    assert np.array_equal(ops.get('counts', torch.int64, (g, n_e)).cpu().numpy(), _hist_ref(a, n_e)[0])


def test_index_histogram_walks_65536_bins(cuda_device):
    rng = np.random.default_rng(2)
    a = rng.integers(0, 65536, (2, 5000), dtype=np.int64)
    a[0, :3] = [65535, 0, 65536]
    _hist_check(a, 65536)


def test_usage_of_encoded_indices(cuda_device):
    net, _, _ = _net('x4', cuda_device)
    x = torch.from_numpy(synth.synth_input(80, (3, 3, 24, 40))).to(cuda_device)
    idx = net.encode_indices(x, pad=True)[0]
    n_e = net._cb[0][1]
    got = codebook.usage(idx, n_e)
    assert got.device.type == 'cuda' and torch.equal(got, torch.bincount(idx.flatten(), minlength=n_e))
    per = codebook.usage(idx, n_e, per_image=True)
    assert torch.equal(per, torch.stack([torch.bincount(idx[i].flatten(), minlength=n_e) for i in range(3)]))
    assert 1.0 <= codebook.perplexity(got) <= n_e

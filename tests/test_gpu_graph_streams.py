"""-m gpu: the two execution paths no other module runs - hipGraph replay (`FeMaSRNet.use_graph`) and launches on a stream
other than the default one.

Everything here is compared BIT FOR BIT (`torch.equal` on the image and on every VQ index map); no tolerance appears in this
module.  The eager path on the default stream is what the other modules hold to the oracle and to fp64; this module holds
graph replay and side-stream execution to that eager path and, in the two modes that are bit-identical to the CPU oracle, to the
oracle itself.

Graph capture is the DETERMINISTIC detector of stream discipline: a launch that does not go to the capturing stream is either
refused by the runtime during the capture or is simply not part of the graph - and then the replay on a second input returns
what the first input left behind (`test_replay_equals_eager`, step 3).  The side-stream tests at the end are PROBABILISTIC: they
make a stray launch on the default stream read a placeholder or be overtaken, which it does in practice but is not forced to.

No test here is written to make a capture or a replay fail on the device: the refusals are Python exceptions raised before
any launch."""
import functools

import numpy as np
import pytest
import torch

from femasr_amd import _lib, synth
from helpers import oracle_net, synth_weights

pytestmark = pytest.mark.gpu

# the smallest shapes that still reach every structure: x4 24x40 pads to 32x48 (Swin grid 16x24 = 2x3 windows, shifted blocks, decoder
# up to 128x192 with ragged Winograd and halo tiles); x2 40x72 pads to 64x96 (the same grid); hq 64x96 runs unpadded through forward()
SHAPES = {'x4': (24, 40), 'x2': (40, 72), 'hq': (64, 96)}
ORACLE_EXACT = ('fp32_strict', 'fp32_direct')      # the decoder modes that are bit-identical to OracleNet() / OracleNet(winograd=False)


@functools.lru_cache(maxsize=None)
def _weights(cfg, seed=5):
    return synth_weights(cfg, seed, 'trained')


def _net(cfg, dev, decoder_math='fp32_strict', linear_math='bf16_split', streams=1, seed=5, weights=None):
    import gpu_utils as G
    net = G.build_net(cfg, _weights(cfg, seed) if weights is None else weights, dev, decoder_math=decoder_math, linear_math=linear_math)
    net.num_streams = streams
    return net


@functools.lru_cache(maxsize=None)
def _pool(cfg, tag):
    """Five samples of the config's shape; every batch of a test is cut from these, so the oracle sees few distinct samples."""
    return synth.synth_input({'a': 71, 'b': 72}[tag], (5, 3) + SHAPES[cfg])


def _inputs(cfg, b, dev):
    """(xa, xb): two different batches of b samples.  The LAST sample of xb is always sample 0 of pool 'b' - the one sample the
    oracle is run on; in a batch split over sub-batch streams it lies in the last branch."""
    pa, pb = _pool(cfg, 'a'), _pool(cfg, 'b')
    xb = np.concatenate([pb[1:b], pb[0:1]], 0)
    return torch.from_numpy(pa[:b].copy()).to(dev), torch.from_numpy(xb).to(dev)


def _call(net, cfg, x):
    """(image, [index map per codebook]) through `test_with_all_indices` (`forward` for the hq config)."""
    if cfg == 'hq':
        y, _, _, idx = net(x)
        return y, list(idx)
    y, idx = net.test_with_all_indices(x)
    return y, list(idx)


def _same(got, want, what):
    assert got[0].shape == want[0].shape and torch.equal(got[0], want[0]), \
        f'{what}: image differs, max-abs {float((got[0] - want[0]).abs().max()):.3e}'
    assert len(got[1]) == len(want[1]) and len(got[1]) >= 1
    for k, (a, b) in enumerate(zip(got[1], want[1])):
        assert a.dtype == torch.int64 and a.shape == b.shape and torch.equal(a, b), f'{what}: index map {k} differs'


@functools.lru_cache(maxsize=None)
def _oracle_last_sample(cfg, decoder_math, linear_math):
    """The oracle on sample 0 of pool 'b' (8 - 25 s of CPU per x4 / x2 sample: once per mode for the whole module)."""
    onet = oracle_net(cfg, _weights(cfg), linear_math=linear_math, winograd=decoder_math != 'fp32_direct')
    x = _pool(cfg, 'b')[0:1]
    return onet.forward(x) if cfg == 'hq' else onet.test(x, return_indices=True)


# ------------------------------------------------------------------------------------------------ 1. replay equals eager
_DM = ('fp32', 'fp32_strict', 'fp32_direct', 'bf16x3')
_LM = ('bf16_split', 'fp32')
_BS = ((1, 1), (2, 3), (3, 3), (5, 2), (5, 3))          # (batch, num_streams): fewer samples than streams, equal, ragged split


def _matrix():
    cases = [('x4', d, l, 5, 3) for d in _DM for l in _LM]                                        # every mode at x4
    cases += [('x4', d, 'bf16_split', b, s) for d in ('fp32', 'bf16x3') for b, s in _BS]            # every (B, streams) pair at x4
    cases += [('x4', 'fp32_strict', 'bf16_split', b, s) for b, s in ((1, 1), (2, 3))]              # (against the oracle as well)
    for cfg in ('x2', 'hq'):
        # all four decoder modes at (5, 3).  The oracle-exact modes run linear_math 'fp32' here: the CPU oracle's restated bf16
        # matrix instruction costs ~3x the fmaf chain, and 'bf16_split' is held to the oracle in those modes by the x4 cases
        cases += [(cfg, d, 'fp32' if d in ORACLE_EXACT else 'bf16_split', 5, 3) for d in _DM]
        cases += [(cfg, 'fp32', 'bf16_split', 1, 1), (cfg, 'fp32_strict', 'fp32', 2, 3)]
    return list(dict.fromkeys(cases))


@pytest.mark.parametrize('cfg,dm,lm,b,s', _matrix(), ids=lambda v: str(v))
def test_replay_equals_eager(cuda_device, cfg, dm, lm, b, s):
    """Per case two different inputs xa, xb of one shape.  (1) eager references; (2) the first graph call captures and replays: equal
    to eager(xa); (3) the second call is a replay only, on NEW input: equal to eager(xb) - this is the assertion that fails when any
    launch escaped the capture, since such a launch ran once, on xa; (4) xa again: the first result, no new cache entry; (5) in
    the modes that are bit-identical to the CPU oracle the replay is held to the oracle directly, so the module does not rest on the
    eager path alone.  The oracle is run on ONE sample (an oracle forward costs 8 - 25 s of CPU at these shapes): the last one of
    xb, which is a replay-only result and, with sub-batch streams, comes out of the last parallel branch of the graph.  The oracle is
    per-sample by construction (OracleNet on a batch is bit-identical to OracleNet on each sample), the other samples are held
    through the eager path."""
    net = _net(cfg, cuda_device, dm, lm, s)
    xa, xb = _inputs(cfg, b, cuda_device)
    net.use_graph = False
    ea, eb = _call(net, cfg, xa), _call(net, cfg, xb)
    assert not torch.equal(ea[0], eb[0]) and not net._graphs
    net.use_graph = True
    g1 = _call(net, cfg, xa)
    assert len(net._graphs) == 1
    _same(g1, ea, 'capture + first replay')
    g2 = _call(net, cfg, xb)
    _same(g2, eb, 'replay on new input')
    g3 = _call(net, cfg, xa)
    _same(g3, g1, 'replay of the first input again')
    assert len(net._graphs) == 1
    if dm in ORACLE_EXACT:
        yo, io = _oracle_last_sample(cfg, dm, lm)
        y, idx = g2[0][b - 1:b].cpu().numpy(), g2[1][0][b - 1:b].cpu().numpy()
        assert np.array_equal(idx.reshape(-1), np.asarray(io).reshape(-1)), 'graph replay: VQ indices differ from the oracle'
        assert y.shape == yo.shape and np.array_equal(y, yo), f'graph replay vs oracle: max-abs {np.abs(y - yo).max():.3e}'


# ------------------------------------------------------------------------------------------------ 2. cache keys and eviction
def test_cache_keys(cuda_device):
    """Batch size, shape, num_streams, decoder_math and linear_math are each part of the key: a change of any of them adds exactly
    one entry (and gives the eager result); going back to an earlier setting reuses its entry."""
    net = _net('x4', cuda_device)
    settings = [dict(b=2, hw=(24, 40), streams=1, dm='fp32_strict', lm='bf16_split')]
    for change in (dict(b=3), dict(hw=(16, 24)), dict(streams=3), dict(dm='bf16x3'), dict(lm='fp32')):
        settings.append(dict(settings[-1], **change))

    def run(st, graph):
        net.num_streams, net.decoder_math, net.linear_math, net.use_graph = st['streams'], st['dm'], st['lm'], graph
        x = torch.from_numpy(synth.synth_input(31, (st['b'], 3) + st['hw'])).to(cuda_device)
        return _call(net, 'x4', x)

    refs = [run(st, False) for st in settings]
    assert not net._graphs
    for n, st in enumerate(settings):
        _same(run(st, True), refs[n], f'new key {st}')
        assert len(net._graphs) == n + 1, f'{st}: a new key adds one entry'
    for n in (0, 3, 1, 5, 4, 2):
        _same(run(settings[n], True), refs[n], f'earlier key {settings[n]}')
        assert len(net._graphs) == len(settings), 'an earlier key reuses its entry'


def test_cache_eviction_keeps_results(cuda_device):
    """Ten shapes on one net: the cache holds nine graphs and is cleared when the tenth is captured.  Every result is right,
    including those obtained before the clear and read after it (nothing is synchronised or compared until all ten calls are
    enqueued: a result is a copy of the graph's static output, made on the stream before the graph is dropped)."""
    net = _net('x4', cuda_device, streams=2)
    shapes = [(16, 16), (16, 24), (24, 16), (24, 32), (32, 24), (32, 40), (40, 32), (40, 56), (56, 40), (56, 56)]
    xs = [torch.from_numpy(synth.synth_input(40 + i, (2, 3) + hw)).to(cuda_device) for i, hw in enumerate(shapes)]
    refs = [_call(net, 'x4', x) for x in xs]
    net.use_graph = True
    got, sizes = [], []
    for x in xs:
        got.append(_call(net, 'x4', x))
        sizes.append(len(net._graphs))
    assert sizes == [1, 2, 3, 4, 5, 6, 7, 8, 9, 1]
    for i in range(len(xs)):
        _same(got[i], refs[i], f'shape {shapes[i]}')
    _same(_call(net, 'x4', xs[0]), refs[0], 'an evicted key is captured again')
    assert len(net._graphs) == 2


def _tile_image(dev):
    img = torch.from_numpy(synth.synth_input(10, (1, 3, 70, 100))).to(dev)        # (the image of test_gpu_r4.py: 3 x 4 tiles, 9 shape classes)
    u8 = (img[0].permute(1, 2, 0) * 255.0).round().clamp(0, 255).to(torch.uint8).contiguous()
    return img, u8


def test_tiled_under_graph(cuda_device):
    """`test_tile` with use_graph: every batched call of a shape class is a replay into the tile driver's result slab (`out=`), and
    the image has more (class, batch) keys than the cache still has room for, so the cache is cleared in the MIDDLE of the image
    while earlier tiles are still in flight.  `test_tile_u8` runs `test_u8`, which has no graph path: the switch must leave it
    alone.  Both equal the use_graph = False results."""
    from femasr_amd import tiling
    net = _net('x4', cuda_device, streams=2)
    net.max_tile_batch = 3
    img, u8 = _tile_image(cuda_device)
    ref, ref_u8 = net.test_tile(img, 32, 8), net.test_tile_u8(u8, 32, 8)
    classes = tiling.shape_classes(tiling.enumerate_tiles(70, 100, 32, 8))
    keys = {(min(3, len(tl) - i), hw) for hw, tl in classes.items() for i in range(0, len(tl), 3)}
    net.use_graph = True
    pre = [torch.from_numpy(synth.synth_input(3, (1, 3, 16, 16 + 8 * i))).to(cuda_device) for i in range(3)]
    for x in pre:
        net.test(x)
    assert len(net._graphs) == 3 and len(keys) + 3 > 9
    got = net.test_tile(img, 32, 8)
    assert 0 < len(net._graphs) < len(keys) + 3, 'the cache was cleared while the image was being tiled'
    assert torch.equal(got, ref)
    n = len(net._graphs)
    got_u8 = net.test_tile_u8(u8, 32, 8)
    assert len(net._graphs) == n and torch.equal(got_u8, ref_u8)
    assert torch.equal(net.test_tile(img, 32, 8), ref)


# ------------------------------------------------------------------------------------------------ 3. weights changed under a live graph
@pytest.mark.parametrize('streams', [1, 3])
def test_weights_changed_under_a_live_graph(cuda_device, streams):
    """A graph captured once keeps replaying while the weights change underneath it; after each change graph mode must equal a
    freshly built eager net holding those weights.  The graph bakes in the ADDRESSES of the handle's repacked weights, so this holds
    because femasr_set_weight / femasr_finalize_weights repack into the allocations of the first push: repacked weight buffers are never
    reallocated while a handle lives.  A stale graph shows as the previous weights' image."""
    dev = cuda_device
    net = _net('x4', dev, streams=streams)
    x = torch.from_numpy(_pool('x4', 'a')[:3].copy()).to(dev)
    net.use_graph = True
    last = _call(net, 'x4', x)
    keys = list(_weights('x4'))

    def check(what, differs=True):
        nonlocal last
        sd = net.state_dict()
        fresh = _net('x4', dev, streams=streams, weights={k: sd[k].detach().cpu().numpy() for k in keys})
        want = _call(fresh, 'x4', x)
        got = _call(net, 'x4', x)
        _same(got, want, what)
        assert torch.equal(got[0], last[0]) != differs, f'{what}: the weights were meant to change the image' if differs else what
        last = got

    # (a) load_state_dict of another seed
    net.load_state_dict({k: torch.from_numpy(v) for k, v in _weights('x4', 6).items()}, strict=False)
    check('(a) load_state_dict')
    assert len(net._graphs) == 1
    # (b) in-place ops: a conv in front of the lookup, the codebook, the last conv
    net.multiscale_encoder.in_conv.weight.mul_(1.03125)
    net.get_parameter('quantize_group.0.embedding.weight').mul_(0.96875)
    net.out_conv.weight.mul_(1.5)
    check('(b) in-place parameter updates')
    # (c) a write torch's version counter cannot see, announced through invalidate_weights()
    net.out_conv.weight.data.copy_(torch.from_numpy(_weights('x4')['out_conv.weight']))
    net.invalidate_weights()
    assert not net._graphs
    check('(c) .data write + invalidate_weights()')
    # (d) dtype / device round trips: new storage for every parameter, all re-pushed under the graph captured in (c); one bias is
    # changed while on the host so that a stale graph would show
    net.float()
    net.cpu()
    net.multiscale_encoder.in_conv.bias.add_(0.0625)
    net.to(dev)
    check('(d) .float() / .cpu() / .to(device) round trip')
    assert len(net._graphs) == 1


# ------------------------------------------------------------------------------------------------ 4. interleaving and out=
def test_interleaved_eager_and_graph(cuda_device):
    """Eager and graph calls alternate on one net; an eager call of a larger shape reallocates the net's workspace between two
    replays of an older graph (which owns its own)."""
    net = _net('x4', cuda_device, streams=3)
    small = torch.from_numpy(_pool('x4', 'a')[:2].copy()).to(cuda_device)
    small2 = torch.from_numpy(_pool('x4', 'b')[:2].copy()).to(cuda_device)
    big = torch.from_numpy(synth.synth_input(33, (3, 3, 40, 56))).to(cuda_device)
    ref = {k: _call(net, 'x4', v) for k, v in (('small', small), ('small2', small2), ('big', big))}
    net._ws = None                                                       # (start again without a workspace)
    inputs = dict(small=small, small2=small2, big=big)
    for step, (graph, name) in enumerate([(False, 'small'), (True, 'small'), (False, 'small2'), (True, 'small2'), (False, 'big'),
                                          (True, 'small'), (False, 'small2'), (True, 'big'), (True, 'small2'), (False, 'big'),
                                          (True, 'big'), (True, 'small')]):
        net.use_graph = graph
        _same(_call(net, 'x4', inputs[name]), ref[name], f'step {step}: {"graph" if graph else "eager"} {name}')
    assert len(net._graphs) == 2


def test_out_parameter_under_graph(cuda_device):
    """`test(x, out=buf)` with use_graph writes into `buf` and returns it; a tensor that does not fit raises ValueError as it does eagerly."""
    net = _net('x4', cuda_device, streams=2)
    x = torch.from_numpy(_pool('x4', 'a')[:3].copy()).to(cuda_device)
    y = net.test(x)
    net.use_graph = True
    slab = torch.full((5, 3, 96, 160), -7.0, device=cuda_device)
    r = net.test(x, out=slab[1:4])
    assert r.data_ptr() == slab[1:4].data_ptr() and torch.equal(slab[1:4], y)
    assert float(slab[0].max()) == -7.0 and float(slab[0].min()) == -7.0 and float(slab[4].max()) == -7.0 and float(slab[4].min()) == -7.0
    for bad in (torch.empty((3, 3, 96, 161), device=cuda_device), torch.empty((3, 3, 96, 160), device=cuda_device, dtype=torch.float16),
                torch.empty((3, 3, 160, 96), device=cuda_device).transpose(2, 3), torch.empty((1, 3, 96, 160), device=cuda_device)):
        with pytest.raises(ValueError):
            net.test(x, out=bad)
    small = x[:, :, :16, :24].contiguous()
    with pytest.raises(ValueError):                                       # refused before a graph of a new shape is captured
        net.test(small, out=slab[1:4])
    assert len(net._graphs) == 1
    assert torch.equal(net.test(x), y)


# ------------------------------------------------------------------------------------------------ 5. profiling and graph
def test_profiling_refuses_graph(cuda_device):
    """enable_profile(True) records an event pair around every launch; inside a capture those events would never be signalled.  The
    combination is refused in Python before anything is captured; with profiling off again the graph path works."""
    net = _net('x4', cuda_device, streams=3)
    x = torch.from_numpy(_pool('x4', 'a')[:2].copy()).to(cuda_device)
    ref = _call(net, 'x4', x)
    net.enable_profile(True)
    net.use_graph = True
    with pytest.raises(_lib.FemasrError, match=r'(?s)use_graph.*enable_profile'):
        net.test(x)
    assert not net._graphs
    net.use_graph = False
    _same(_call(net, 'x4', x), ref, 'eager while profiling')
    assert net.profile()                                                  # the profiler itself still reports
    net.enable_profile(False)
    net.use_graph = True
    _same(_call(net, 'x4', x), ref, 'graph after enable_profile(False)')
    _same(_call(net, 'x4', x), ref, 'replay after enable_profile(False)')
    assert len(net._graphs) == 1


# ------------------------------------------------------------------------------------------------ 6. side streams
@functools.lru_cache(maxsize=None)
def _busy_matrix(dev):
    n = 4096
    return torch.full((n, n), 1.0 / n, device=dev), torch.empty((n, n), device=dev)      # (a @ a == a: the chain neither grows nor decays)


def _tree(o, f):
    if torch.is_tensor(o):
        return f(o)
    return [_tree(e, f) for e in o]


def _placeholder(t):
    """Other values of the same kind (an image stays an image; not a map under which a metric of a pair is unchanged)."""
    if t.dtype == torch.uint8:
        return t // 3 + 40
    return torch.zeros_like(t) if t.dtype == torch.int64 else 0.75 * t * t + 0.125


def _side_stream_check(op, inputs, dev, what):
    """`ref = op(*inputs)` on the default stream (which also does every one-time step: weight push, workspace, graph capture).  Then
    on a fresh stream s: the staging tensors hold OTHER values; a few tens of ms of matmuls are enqueued on s; the real inputs are
    copied in on s; the op runs; its outputs are cloned on s.  Compared after s.synchronize() only.  A kernel that went to the
    default stream instead would start at once, read the placeholder and be overtaken by the clone.  (Probabilistic: see the module
    docstring; the capture of test_replay_equals_eager is the deterministic check.)"""
    ref = _tree(op(*inputs), lambda t: t.clone())
    stage = [_placeholder(t) for t in inputs]
    a, c = _busy_matrix(dev)
    torch.mm(a, a, out=c)                                                 # (one-time BLAS setup outside the timed window)
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        for _ in range(40):
            torch.mm(a, a, out=c)
        for st, t in zip(stage, inputs):
            st.copy_(t, non_blocking=True)
        got = _tree(op(*stage), lambda t: t.clone())
    s.synchronize()
    flat_ref, flat_got = [], []
    _tree(ref, flat_ref.append)
    _tree(got, flat_got.append)
    assert len(flat_ref) == len(flat_got) >= 1
    for k, (g, r) in enumerate(zip(flat_got, flat_ref)):
        assert g.dtype == r.dtype and g.shape == r.shape and torch.equal(g, r), f'{what}: output {k} on a side stream differs from the default stream'
    return ref


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graph'])
@pytest.mark.parametrize('streams', [1, 3])
def test_side_stream_forward(cuda_device, streams, graph):
    """`test` and `test_with_all_indices` on a side stream, one stream and forked into three sub-batch streams, eager and as a replay."""
    net = _net('x4', cuda_device, streams=streams)
    x = torch.from_numpy(_pool('x4', 'a')[:3].copy()).to(cuda_device)
    eager = _call(net, 'x4', x)
    net.use_graph = graph

    def op(t):
        y, idx = net.test_with_all_indices(t)
        return [net.test(t), y, list(idx)]
    ref = _side_stream_check(op, [x], cuda_device, f'test / test_with_all_indices, {streams} streams, graph={graph}')
    assert torch.equal(ref[0], eager[0])
    _same((ref[1], ref[2]), eager, 'default stream')
    assert len(net._graphs) == int(graph)


@pytest.mark.parametrize('bgr', [False, True], ids=['rgb', 'bgr'])
def test_side_stream_u8_and_decode(cuda_device, bgr):
    """`test_u8` (both channel orders) and `decode_indices` on a side stream."""
    net = _net('x4', cuda_device, streams=3)
    x = torch.from_numpy(_pool('x4', 'b')[:3].copy()).to(cuda_device)
    u8 = (x.permute(0, 2, 3, 1) * 255.0).round().clamp(0, 255).to(torch.uint8).contiguous()
    _side_stream_check(lambda t: net.test_u8(t, bgr=bgr), [u8], cuda_device, f'test_u8(bgr={bgr})')
    if not bgr:
        idx = net.test_with_all_indices(x)[1][0]
        idx2 = (idx * 7 + 3) % 1024                                       # (not the placeholder's all-zero map either)
        _side_stream_check(net.decode_indices, [idx2], cuda_device, 'decode_indices')


def test_side_stream_tiled(cuda_device):
    """`test_tile` / `test_tile_u8` (extract kernel, batched forwards with out=, paste kernel) on a side stream."""
    net = _net('x4', cuda_device, streams=2)
    net.max_tile_batch = 3
    img, u8 = _tile_image(cuda_device)
    _side_stream_check(lambda t: net.test_tile(t, 32, 8), [img], cuda_device, 'test_tile')
    _side_stream_check(lambda t: net.test_tile_u8(t, 32, 8), [u8], cuda_device, 'test_tile_u8')


@pytest.mark.parametrize('bgr', [False, True], ids=['rgb', 'bgr'])
def test_side_stream_imgproc(cuda_device, bgr):
    from femasr_amd import imgproc
    img, u8 = _tile_image(cuda_device)
    img = img * 1.5 - 0.25                                                 # (values on both sides of the clamp)
    _side_stream_check(lambda t: imgproc.u8_to_input(t, bgr=bgr), [u8], cuda_device, 'u8_to_input')
    _side_stream_check(lambda t: imgproc.output_to_u8(t, bgr=bgr), [img], cuda_device, 'output_to_u8')


@pytest.mark.parametrize('kind', ['alex', 'vgg'])
def test_side_stream_lpips(cuda_device, kind):
    from femasr_amd import lpips as L
    m = L.LPIPS(kind, state_dict={k: torch.from_numpy(v) for k, v in synth.lpips_state(L.expected_shapes(kind), 7).items()}).to(cuda_device)
    x0 = torch.from_numpy(synth.synth_input(11, (2, 3, 64, 96))).to(cuda_device)
    x1 = torch.from_numpy(synth.synth_input(12, (2, 3, 64, 96))).to(cuda_device)
    ref = _side_stream_check(lambda p, q: list(m(p, q, per_layer=True)), [x0, x1], cuda_device, f'LPIPS({kind})')
    assert float(ref[0].min()) > 0.0


@pytest.mark.parametrize('ty', [True, False], ids=['y', 'rgb'])
def test_side_stream_psnr_ssim(cuda_device, ty):
    from femasr_amd import psnr_ssim as P
    rng = np.random.RandomState(45 + 77)                                   # (a shape of test_gpu_psnr_ssim.py::test_bitwise_properties)
    a = rng.randint(0, 256, (6, 45, 77, 3)).astype(np.uint8)
    b = np.clip(a.astype(np.int64) + rng.randint(-20, 21, a.shape), 0, 255).astype(np.uint8)
    xa, xb = torch.from_numpy(a).to(cuda_device), torch.from_numpy(b).to(cuda_device)
    ref = _side_stream_check(lambda p, q: list(P.psnr_ssim(p, q, 4, ty)), [xa, xb], cuda_device, f'psnr_ssim(y={ty})')
    assert bool(torch.all(torch.isfinite(ref[0]))) and bool(torch.all(ref[1] < 1.0))

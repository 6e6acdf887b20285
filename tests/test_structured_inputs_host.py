"""CPU: the conditions tests/test_gpu_structured_inputs.py relies on, pinned with the oracle alone.

  * every integer family: the oracle's restatement of each form == the independent int64 reference of tests/structured_inputs.py
    EXACTLY, so the magnitudes keep every partial sum of every specified order inside the integers fp32 holds;
  * window attention with q = k = 0: exactly the window (region) mean; the VQ search: exactly the first-min argmin;
  * the network contents: finite oracle output and no token whose two best codes lie within (0, NEAR_TIE_ULP] ulp, so identical
    indices can be demanded of every mode;
  * a constant map on which the GroupNorm variance clamp is reached, in both summation orders."""
import numpy as np
import pytest

import structured_inputs as S
from helpers import oracle_net, synth_weights
from oracle import oracle as orc
from oracle.near_tie import NEAR_TIE_ULP, gap_ulp


def f32(a):
    return None if a is None else np.asarray(a, np.float32)


def oracle_conv(case, x, w, b, r1, r2):
    """The oracle's restatement of the case's form on fp32 copies of the integer operands."""
    name, shape, cout, k, s, p, up2, form = case
    if form == 'split' and k == 3:
        return orc.conv3x3_bf16s(f32(x), f32(w), f32(b), f32(r1), f32(r2), stride=s)
    if form == 'split':
        rows = int(np.prod(shape[:3]))
        y = orc.linear_bf16s(f32(x).reshape(rows, -1), f32(w).reshape(shape[3], cout).T, f32(b), 0, f32(r1).reshape(rows, cout), f32(r2).reshape(rows, cout))
        return y.reshape(r1.shape)
    # (the bf16x3 halo form has no restatement of its own - it is held to a tolerance elsewhere -: the direct form stands in, which
    # proves the magnitudes)
    return orc.conv2d(f32(x), f32(w), f32(b), k, s, p, up2, res1=f32(r1), res2=f32(r2), wino=form == 'wino')


@pytest.mark.parametrize('case', S.INT_CONV_CASES, ids=[c[0] for c in S.INT_CONV_CASES])
def test_integer_conv_families_oracle_equals_int64(case):
    """Winograd forms (F(4x4) and x2): weights in {-576, 0, 576}, inputs in {0, 1}.  576 = 24^2 clears the denominators of G, the
    products with the rounded constants 1/6 and 1/24 round back to the integers, and the EXACT assertion holds for this family at
    Cin 32 and 64 - so the Winograd forms are held to the int64 result exactly, not to the tolerance against the direct form."""
    name, shape, cout, k, s, p, up2, form = case
    x, w, b, r1, r2 = S.int_conv_operands(case)
    assert S.conv2d_abs_bound(x, w, b, s, p, up2, r1, r2) < 2 ** 24
    ref = S.conv2d_ref(x, w, b, s, p, up2, r1, r2)
    assert ref.shape == (shape[0],) + S.out_hw(shape, k, s, p, up2) + (cout,) and np.abs(ref).max() > 8
    bad = S.first_mismatch(oracle_conv(case, x, w, b, r1, r2), ref)
    assert not bad, f'{name}: oracle vs int64 (n, y, x, c): {bad}'
    if up2:         # the two definitions of the x2 conv agree: enlarge, then convolve
        assert np.array_equal(ref, S.conv2d_ref(x.repeat(2, axis=1).repeat(2, axis=2), w, b, s, p, False, r1, r2))


@pytest.mark.parametrize('n,k', S.INT_LINEAR_CASES)
def test_integer_linear_families_oracle_equals_int64(n, k):
    x, w, b, r1, r2 = S.int_linear_operands(n, k)
    ref = S.linear_ref(x, w, b, r1, r2)
    assert S.linear_ref(np.abs(x), np.abs(w), np.abs(b), np.abs(r1), np.abs(r2)).max() < 2 ** 24
    chain = orc.linear(f32(x), f32(w), f32(b), res=f32(r1)) + f32(r2)
    split = orc.linear_bf16s(f32(x), f32(w).T, f32(b), 0, f32(r1), f32(r2))
    for what, y in (('fp32 chain', chain), ('split-bf16', split)):
        bad = S.first_mismatch(y, ref)
        assert not bad, f'linear N {n} K {k} {what} (row, column): {bad}'


def test_references_tell_mutations_apart():
    """The independent references are not symmetric in what the GPU tests are meant to catch: swapped taps, a last-min rule and a
    roll by 3 all change them on the committed families."""
    case = S.INT_CONV_CASES[1]
    x, w, b, r1, r2 = S.int_conv_operands(case)
    wsw = w.copy()
    wsw[[0, 2]] = wsw[[2, 0]]
    assert not np.array_equal(S.conv2d_ref(x, w, b, 1, 1), S.conv2d_ref(x, wsw, b, 1, 1))
    z, cb = S.vq_operands(128, 64, 130)
    idx = S.vq_argmin_ref(z, cb)
    d = ((z[:, None, :] - cb[None, :, :]) ** 2).sum(-1)
    last = d.shape[1] - 1 - np.argmin(d[:, ::-1], axis=1)
    assert np.array_equal(idx, np.argmin(d, axis=1)) and not np.array_equal(idx, last)
    _, v = S.attention_operands(1, 16, 24, 1)
    s4, c4 = S.window_mean_ref(v, 1, 16, 24, 4)
    s3, c3 = S.window_mean_ref(v, 1, 16, 24, 3)
    assert not np.array_equal(s4, s3)
    assert sorted(set(c4.reshape(-1).tolist())) == [16, 32, 64]


@pytest.mark.parametrize('b,h,w,heads,shift', S.ATT_CASES)
def test_attention_with_zero_logits_is_the_window_mean_exactly(b, h, w, heads, shift):
    """q = k = 0 and a zero bias table: every allowed key weighs 1/n, n in {16, 32, 64}; the masked keys' exp(-100) vanish against
    n.  The oracle returns sums / n EXACTLY for shift 0 and shift 4, so the GPU test demands equality, not one ulp."""
    qkv, v = S.attention_operands(b, h, w, heads)
    sums, cnt = S.window_mean_ref(v, b, h, w, shift)
    assert set(cnt.reshape(-1).tolist()) <= {16, 32, 64} and (shift == 0) == (set(cnt.reshape(-1).tolist()) == {64})
    want = sums.astype(np.float64) / cnt[..., None]
    got = orc.window_attention(qkv, b, h, w, S.ATT_HEAD_DIM * heads, heads, shift, np.zeros((225, heads), np.float32))
    bad = S.first_mismatch(got, want)
    assert not bad, f'(image, token, channel): {bad}'


@pytest.mark.parametrize('n_e,d,m', S.VQ_CASES)
def test_vq_first_min_on_integer_ties(n_e, d, m):
    z, cb = S.vq_operands(n_e, d, m)
    idx = S.vq_argmin_ref(z, cb)
    dist = ((z[:, None, :] - cb[None, :, :]) ** 2).sum(-1)
    assert ((dist == dist.min(1, keepdims=True)).sum(1) > 1).any(), 'the family holds no exact tie'
    io, zq = orc.vq(f32(z), f32(cb))
    assert not S.first_mismatch(io, idx)
    assert np.array_equal(zq.view(np.uint32), f32(cb)[idx].view(np.uint32))


# ------------------------------------------------------------------ network contents
def net_reference(cfg, content, seed=S.NET_SEED):
    """(x fp32 NCHW, uint8 image, oracle output, oracle indices, gaps in ulp per token) of one (config, content), memoised by helpers."""
    w = synth_weights(cfg, seed, 'trained')
    u8 = S.image(content, *S.NET_LR[cfg])
    x = S.to_float(u8)
    net = oracle_net(cfg, w)
    net.probes = {}
    y, idx = net.test(x, return_indices=True)
    z = net.probes['z']
    net.probes = None
    _, _, d1, d2 = orc.vq(z.reshape(-1, z.shape[-1]), w['quantize_group.0.embedding.weight'], want_dists=True)
    return x, u8, y, idx, np.array([gap_ulp(a, b) for a, b in zip(d1, d2)])


@pytest.mark.parametrize('cfg,content', S.NET_CASES, ids=[f'{c}-{n}' for c, n in S.NET_CASES])
def test_network_contents_are_finite_and_free_of_near_ties(cfg, content):
    """Weight seed NET_SEED = 22 clears all ten x4 contents and the four x2 ones (so does seed 0; 22 is the first seed that also keeps
    the fp16 emulation's indices, see the next test): no content is dropped from the non-strict modes (S.NET_DROPPED is empty).  Exact
    ties (gap 0) would be fine - the first-min rule decides them."""
    x, u8, y, idx, gaps = net_reference(cfg, content)
    scale = 4 if cfg == 'x4' else 2
    assert y.shape == (1, 3, scale * S.NET_LR[cfg][0], scale * S.NET_LR[cfg][1]) and np.isfinite(y).all()
    assert np.isfinite(gaps).all() and (gaps >= 0).all()
    near = np.flatnonzero((gaps > 0) & (gaps <= NEAR_TIE_ULP))
    print(f'{cfg} {content}: {idx.size} tokens, {len(np.unique(idx))} distinct codes, smallest gap {gaps.min():.0f} ulp, output {y.min():.3f} .. {y.max():.3f}')
    assert len(near) == 0, f'tokens {near.tolist()} have gaps {gaps[near].tolist()} ulp'
    assert S.NET_DROPPED == ()
    assert y.min() < 0.0 or y.max() > 1.0               # the byte path's clamp has work to do


@pytest.mark.parametrize('cfg,content', S.NET_CASES, ids=[f'{c}-{n}' for c, n in S.NET_CASES])
def test_fp16_operands_keep_every_index_in_the_emulation(cfg, content):
    """What lets the GPU test demand identical indices of linear_math='fp16' too: with the layers in front of the lookup rounded once to
    fp16 (float64 sums; tests/fp16_front_ref.py) every token of every content still resolves to the oracle's code, and the two best
    codes of the emulation's own distances stay more than NEAR_TIE_ULP ulp apart."""
    import fp16_front_ref as FR
    from helpers import CONFIGS
    x, u8, y, idx, gaps = net_reference(cfg, content)
    net = FR.emulation_net(synth_weights(cfg, S.NET_SEED, 'trained'), CONFIGS[cfg], 'fp16')
    _, i16 = FR.run_net(net, cfg, x)
    assert np.array_equal(i16, idx), f'{int((i16 != idx).sum())} tokens flip under fp16 operands'
    d = np.sort(net.d0.numpy(), axis=1)
    g16 = (d[:, 1] - d[:, 0]) / np.spacing(d[:, 0])
    assert not ((g16 > 0) & (g16 <= NEAR_TIE_ULP)).any(), g16.min()


def test_oracle_refuses_a_mirror_pad_beyond_twice_the_image():
    """A mirror pad holds at most 2 h rows and 2 w columns (femasr_arch.py:459-460).  The library refuses a larger one; the oracle used
    to read in front of its input instead (row 2 h - 1 - y < 0), which made x2 at 13 rows return different garbage from run to run."""
    x = S.to_float(S.image('white', 13, 19))
    with pytest.raises(ValueError):
        orc.pad_nchw_to_nhwc(x, 32, 32)
    with pytest.raises(ValueError):
        oracle_net('x2', synth_weights('x2', S.NET_SEED, 'trained')).test(x)
    assert orc.pad_nchw_to_nhwc(x, 26, 38).shape == (1, 26, 38, 3)


# ------------------------------------------------------------------ GroupNorm variance clamp
def _tiled_order_sums(xg):
    """fp64 S, SS of one group (H, W, cg) in the 8x16-tile order of DESIGN.md's moments (cg a power of two): per tile four quarters,
    per quarter and channel two 16-pixel halves, the xor-butterfly over the channels, ((q0 + q1) + q2) + q3, tiles strided over 64
    lanes, the xor-butterfly 32..1 over the lanes."""
    hh, ww, cg = xg.shape
    x = xg.astype(np.float64)
    lanes_s, lanes_q = [0.0] * 64, [0.0] * 64
    t = 0
    for ty in range((hh + 7) // 8):
        for tx in range((ww + 15) // 16):
            quarters = []
            for q in range(4):
                per = []
                for e in range(cg):
                    half = []
                    for h in range(2):
                        s = ss = 0.0
                        for r in range(16):
                            m = 32 * q + 4 * h + (r & 3) + 8 * (r >> 2)
                            y, xx = 8 * ty + (m >> 4), 16 * tx + (m & 15)
                            if y < hh and xx < ww:
                                v = x[y, xx, e]
                                s, ss = s + v, ss + v * v
                        half.append((s, ss))
                    per.append((half[0][0] + half[1][0], half[0][1] + half[1][1]))
                d = 1
                while d < cg:
                    per = [(per[e][0] + per[e ^ d][0], per[e][1] + per[e ^ d][1]) for e in range(cg)]
                    d <<= 1
                quarters.append(per[0])
            lanes_s[t & 63] += ((quarters[0][0] + quarters[1][0]) + quarters[2][0]) + quarters[3][0]
            lanes_q[t & 63] += ((quarters[0][1] + quarters[1][1]) + quarters[2][1]) + quarters[3][1]
            t += 1
    d = 32
    while d >= 1:
        lanes_s = [lanes_s[l] + lanes_s[l ^ d] for l in range(64)]
        lanes_q = [lanes_q[l] + lanes_q[l ^ d] for l in range(64)]
        d >>= 1
    return lanes_s[0], lanes_q[0]


def _row_order_sums(xg):
    """fp64 S, SS of one group in the row order (other channel counts): per image row over x then channel, then the rows ascending."""
    big_s = big_q = 0.0
    for row in xg.astype(np.float64):
        s = ss = 0.0
        for v in row.reshape(-1):
            s, ss = s + v, ss + v * v
        big_s, big_q = big_s + s, big_q + ss
    return big_s, big_q


def unclamped_variance(shape, k, order):
    cg = shape[3] // 32
    s, ss = order(np.full((shape[1], shape[2], cg), np.float32(k) / np.float32(255), np.float32))
    n = float(shape[1] * shape[2] * cg)
    mean = s / n
    return ss / n - mean * mean


@pytest.mark.parametrize('clamp,order', [(S.GN_CLAMP_TILED, _tiled_order_sums), (S.GN_CLAMP_ROWS, _row_order_sums)], ids=['tiled', 'rows'])
def test_groupnorm_clamp_is_reached_on_a_flat_map(clamp, order):
    """The recorded gray level gives a NEGATIVE unclamped variance in the specified summation order (rounding of SS; the true
    variance is 0).  The restatement of the order is tied to the oracle with eps = 0: a clamped group has rstd = 1/sqrt(0) = inf, and
    a level whose variance in that order is positive reproduces the oracle's coefficient bit for bit."""
    shape, k = clamp
    var = unclamped_variance(shape, k, order)
    assert var < 0.0, var
    gamma, beta = np.ones(shape[3], np.float32), np.zeros(shape[3], np.float32)
    x = S.feature('const', shape, np.float32(k) / np.float32(255))
    a, _ = orc.gn_coeffs(x, gamma, beta, eps=0.0)
    assert np.isinf(a).all()
    a, b = orc.gn_coeffs(x, gamma, beta)                   # with the real eps: rstd = 1 / sqrt(eps) exactly, as for a true zero
    assert np.array_equal(a, np.full_like(a, np.float32(1.0) / np.sqrt(np.float32(0.0) + np.float32(1e-6))))
    pos = next(j for j in range(1, 256) if unclamped_variance(shape, j, order) > 0.0)
    vp = unclamped_variance(shape, pos, order)
    ap, _ = orc.gn_coeffs(S.feature('const', shape, np.float32(pos) / np.float32(255)), gamma, beta, eps=0.0)
    assert np.array_equal(ap, np.full_like(ap, np.float32(1.0) / np.sqrt(np.float32(vp)))), (pos, vp, ap.reshape(-1)[0])
    mean, var64 = S.group_moments(x)
    assert np.all(var64 <= 1e-14) and np.allclose(mean, k / 255.0)

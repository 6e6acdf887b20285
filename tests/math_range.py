"""The fp32 sweep set of the elementary-function tests (tests/test_math_range_host.py, tests/test_gpu_math_range.py): built from bit
patterns only, no RNG, so the host run and the GPU run see the same points.

sweep_set():
  (a) every exponent field 0..254 x 4096 mantissas: all values of the top 12 mantissa bits, the low 11 bits a multiplicative hash of
      the point's index (so the low bits are not all zero, and not the same in every binade);
  (b) every 8th bit pattern with |x| in [2^-4, 2^7): the range in which exp / erf / SiLU / GELU do their work;
  (c) the +-4096 bit patterns around the breakpoints of csrc/detmath.h: 0 (the subnormals), 1, 4 (erf's clamp), 4 sqrt2 (GELU's
      argument reaches erf's clamp), 87 and 88 (exp's clamp) and (k + 1/2) ln2, k = 0..127 (where exp's range reduction rounds
      x log2e to the next integer);
  both signs of everything, then +-0, +-inf and the quiet NaN 0x7fc00000.  Sorted by bit pattern, unique.

call_site_set(n): at most 131 072 values for the kernels that call the functions: every exponent x 256 mantissas (the sign alternates
with the mantissa index: 128 per sign, so that the set fits) plus +-64 around the breakpoints in both signs, the specials; optionally finite only and / or |x| <= cap; tiled (repeated from the start) to exactly n values.
"""
import math

import numpy as np

QNAN = np.uint32(0x7fc00000)
LOG2E_F32 = np.float32(1.44269504088896341)
_HASH = 2654435761                  # Knuth's multiplicative constant (2^32 / golden ratio)


def _bits(v):
    return int(np.float32(v).view(np.uint32))


def breakpoints():
    """Bit patterns (positive) of the breakpoints of (c)."""
    pts = [0.0, 1.0, 4.0, 4.0 * math.sqrt(2.0), 87.0, 88.0] + [(k + 0.5) * math.log(2.0) for k in range(128)]
    return [_bits(p) for p in pts]


def _exponent_grid(per_exp):
    """Every exponent field 0..254 x `per_exp` mantissas (top bits all values, low bits hashed)."""
    top = int(math.log2(per_exp))
    assert 1 << top == per_exp and top <= 23
    idx = np.arange(255 * per_exp, dtype=np.uint64)
    e, m = idx // per_exp, idx % per_exp
    low = ((idx * _HASH) & 0xffffffff) >> (32 - (23 - top)) if top < 23 else np.zeros_like(idx)
    return ((e << 23) | (m << (23 - top)) | low).astype(np.uint32)


def _around(radius):
    out = []
    for b in breakpoints():
        out.append(np.arange(max(b - radius, 0), b + radius + 1, dtype=np.int64))
    return np.concatenate(out).astype(np.uint32)


def _finish(pos):
    pos = pos[pos < 0x7f800000]
    both = np.concatenate([pos, pos | np.uint32(0x80000000),
                           np.array([0, 0x80000000, 0x7f800000, 0xff800000, QNAN], np.uint32)])
    return np.unique(both)


_CACHE = {}


def sweep_bits():
    if 'sweep' not in _CACHE:
        a = _exponent_grid(4096)
        b = np.arange(_bits(2.0 ** -4), _bits(2.0 ** 7), 8, dtype=np.int64).astype(np.uint32)
        _CACHE['sweep'] = _finish(np.concatenate([a, b, _around(4096)]))
        _CACHE['sweep'].setflags(write=False)
    return _CACHE['sweep']


def sweep_set():
    """The whole set as float32 (read-only, shared between the tests of a session)."""
    return sweep_bits().view(np.float32)


def call_site_set(n=None, finite=False, cap=None):
    """The call-site subset (<= 131 072 values), optionally finite only and / or |x| <= cap; with n, tiled to exactly n values."""
    grid = _exponent_grid(256)
    grid = grid | ((np.arange(grid.size, dtype=np.uint32) & np.uint32(1)) << np.uint32(31))      # odd mantissa index: negative
    x = np.unique(np.concatenate([grid, _finish(_around(64))])).view(np.float32)
    keep = np.ones(x.size, bool)
    if finite:
        keep &= np.isfinite(x)
    if cap is not None:
        keep &= ~(np.abs(x) > np.float32(cap))          # (a NaN stays unless finite is asked for)
    x = x[keep]
    assert x.size <= 131072
    if n is not None:
        x = np.resize(x, n)
    return np.ascontiguousarray(x)


def witnesses(x=None):
    """What the set must hold to tell a wrong rounding or a moved clamp apart: counts the host test asserts."""
    x = sweep_set() if x is None else x
    bits = np.ascontiguousarray(x).view(np.uint32)
    def has(v):
        b = _bits(v)
        i = np.searchsorted(bits, b)
        return i < bits.size and bits[i] == b

    def with_neighbours(v):
        b = _bits(v)
        return all(has(np.uint32(b + d).view(np.float32)) for d in (-1, 0, 1))

    finite = np.isfinite(x)
    inside = finite & (x >= np.float32(-87.0)) & (x <= np.float32(88.0))
    xi = x[inside]
    t = xi * LOG2E_F32                                                   # fl(x log2e) as the device forms it (float32 product)
    half = t - np.floor(t) == np.float32(0.5)
    even_up = np.floor(t[half]) + 1.0                                    # round-half-up
    differ = int(np.count_nonzero(np.rint(t[half]) != even_up))          # numpy's rint rounds half to even
    return dict(points=int(x.size),
                subnormals=int(np.count_nonzero(finite & (x != 0) & (np.abs(x) < np.float32(2.0 ** -126)))),
                clamp_neighbours=all(with_neighbours(v) for v in (-87.0, 88.0, 4.0, -4.0)),
                half_points=int(np.count_nonzero(half)), half_values=int(np.unique(t[half]).size), half_even_differs=differ,
                specials=all(np.any(bits == np.uint32(s)) for s in (0, 0x80000000, 0x7f800000, 0xff800000, int(QNAN))))


def same_bits(got, ref):
    """Boolean array: got == ref bit for bit; NaNs compared by position only (x86's default NaN is 0xffc00000, the GPU's 0x7fc00000);
    zeros with their sign."""
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    return (got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref))


def assert_same(got, ref, what, x=None):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = ~same_bits(got, ref)
    if bad.any():
        i = int(np.flatnonzero(bad.reshape(-1))[0])
        at = '' if x is None else f' x = {float(np.asarray(x).reshape(-1)[i])!r} ({int(np.asarray(x, np.float32).reshape(-1).view(np.uint32)[i]):#010x}):'
        raise AssertionError(f'{what}: {int(bad.sum())} of {got.size} differ; first at {i}:{at} got {float(got.reshape(-1)[i])!r} '
                             f'({int(got.reshape(-1).view(np.uint32)[i]):#010x}), want {float(ref.reshape(-1)[i])!r} '
                             f'({int(ref.reshape(-1).view(np.uint32)[i]):#010x})')


# ---------------------------------------------------------------- fast SiLU (csrc/halo_mma.h): the derived error bound
def fast_silu_bound(t):
    """Absolute error bound of fast_silu(t) = t * rcp(1 + exp2(t * c)), c = fl(-log2 e), against fp64 t sigma(t); t float64.
    With u = 2^-24 and relative errors throughout:
      * c differs from -log2 e by 0.23u (1.44269502162933 against 1.44269504088896) and the product t * c rounds once (<= u): the
        exponent's argument a = -t log2 e carries <= 1.23u |a| ABSOLUTE error, which exp2 turns into a relative error of
        ln2 * 1.23u * 1.4427 |t| = 1.23u |t| <= 1.3u |t| of e = 2^a = exp(-t);
      * v_exp_f32 is good to 1 ulp: <= 2u more on e;
      * d = 1 + e rounds once (u); an error of e reaches d scaled by e / (1 + e) = 1 - sigma(t);
      * v_rcp_f32 is good to 1 ulp (<= 2u), and the final multiply rounds once (u).
    Together |err| <= u |silu(t)| (4 + (1 - sigma(t)) (1.3 |t| + 2)) to first order; 4.5 instead of 4 covers the second-order terms
    (the largest, (1.3u |t|)^2 / 2 at |t| = 80, is 3e-11)."""
    t = np.asarray(t, np.float64)
    with np.errstate(over='ignore'):
        sig = 1.0 / (1.0 + np.exp(-t))
        one_minus = 1.0 / (1.0 + np.exp(t))
    return 2.0 ** -24 * np.abs(t * sig) * (4.5 + one_minus * (1.3 * np.abs(t) + 2.0))


# ---------------------------------------------------------------- softmax extremes: the window-attention cases
def _u(tag, shape, lo=-1.0, hi=1.0):
    from femasr_amd import synth
    return synth.uniform(61, 'mr' + tag, tuple(shape), lo, hi)


def _window_tokens(b, h, w, shift):
    """(units, 64) token index (row of qkv) of in-window position i of every window (n, wy, wx) of the SHIFTED frame, and the region
    label of that position (fp64_ref.region_ids)."""
    import fp64_ref as R
    reg = R.region_ids(h, w, 8, shift)
    toks, labs, wins = [], [], []
    for n in range(b):
        for wy in range(h // 8):
            for wx in range(w // 8):
                ys = wy * 8 + np.arange(8)[:, None]
                xs = wx * 8 + np.arange(8)[None, :]
                toks.append((n * h * w + ((ys + shift) % h) * w + (xs + shift) % w).reshape(-1))
                labs.append(reg[ys, xs].reshape(-1))
                wins.append((n, wy, wx))
    return np.stack(toks), np.stack(labs), wins


def attention_case(name):
    """One softmax-extremes case (ATTENTION_CASES, or 'nan_key': not comparable with fp64): dict(b, h, w, heads, shift, qkv (b, h w, 3C) float32, table (225, heads) float32, + what the host
    checks of the case need).  C = 32 heads."""
    shapes = {'dominant': (8, 16, 16, 2, 0), 'wide': (2, 16, 24, 2, 4), 'bias': (3, 8, 16, 2, 0), 'tiny': (2, 16, 8, 1, 0),
              'large_v': (2, 8, 8, 2, 0), 'mask_loses': (2, 16, 16, 2, 4),
              'shift1': (1, 16, 16, 1, 1), 'shift3': (2, 16, 24, 2, 3), 'shift5': (1, 16, 16, 2, 5), 'shift7': (1, 16, 24, 1, 7),
              'shift4_8x16': (2, 8, 16, 2, 4), 'shift4_16x8': (1, 16, 8, 1, 4), 'shift4_8x8': (3, 8, 8, 2, 4),
              'nan_key': (1, 16, 16, 2, 4)}
    b, h, w, heads, shift = shapes[name]
    c = 32 * heads
    q, k, v = (_u(name + t, (b * h * w, heads, 32), -2.0, 2.0) for t in 'qkv')
    table = _u(name + 'tab', (225, heads))
    case = dict(name=name, b=b, h=h, w=w, c=c, heads=heads, shift=shift)
    toks, labs, wins = _window_tokens(b, h, w, shift)
    if name == 'dominant':
        # q_i = 24 u_i, k_j = 24 u_((j + t) mod 64): one t = 0..63 per (window, head) unit; the logit of the pair with (j + t) mod 64 == i
        # is 24^2 / sqrt(32) = 101.8, the others 101.8 cos(u_i, u_j') with |cos| ~ 0.18
        u = _u('unit', (64, 32)).astype(np.float64)
        u = (u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)
        assert len(wins) * heads == 64
        for un, tk in enumerate(toks):
            for hd in range(heads):
                t = un * heads + hd
                q[tk, hd] = np.float32(24.0) * u
                k[tk, hd] = np.float32(24.0) * u[(np.arange(64) + t) % 64]
        case['t_of'] = {(win, hd): un * heads + hd for un, win in enumerate(wins) for hd in range(heads)}
    elif name == 'wide':
        q, k = _u('wq', q.shape, -30.0, 30.0), _u('wk', k.shape, -30.0, 30.0)
    elif name == 'bias':
        vals = np.linspace(-300.0, 300.0, 225).astype(np.float32)         # 225 distinct values, another order per head
        order = np.argsort(_u('bord', (225,)), kind='stable')
        table = np.stack([vals[order], vals[order][::-1]], 1)[:, :heads].copy()
        assert np.unique(table[:, 0]).size == 225
    elif name == 'tiny':
        q, k, v = (t * np.float32(1e-20) for t in (q, k, v))
    elif name == 'large_v':
        v = v * np.float32(2.0 ** 100)
    elif name == 'mask_loses':
        # the pixels the cyclic shift wrapped around (region row or column 2) share a key component worth +250 in every logit: after
        # the mask's -100 they still beat every unmasked key (logits of a few units)
        amp = np.float32(math.sqrt(250.0 / (32 ** -0.5)))
        q[:, :, 0] = amp
        k[:, :, 0] = 0.0
        wrapped = (labs // 3 == 2) | (labs % 3 == 2)
        k[toks[wrapped], :, 0] = amp
        case['wrapped'] = wrapped
    elif name == 'nan_key':
        # one key per window (in-window position 9 + 5 * window) has a NaN component: its logits are NaN for every query of the window
        for un, tk in enumerate(toks):
            k[tk[9 + 5 * un], :, 5] = np.nan
    case.update(toks=toks, labs=labs, wins=wins, table=np.ascontiguousarray(table, np.float32),
                qkv=np.ascontiguousarray(np.concatenate([t.reshape(b, h * w, c) for t in (q, k, v)], 2), np.float32))
    return case


ATTENTION_CASES = ('dominant', 'wide', 'bias', 'tiny', 'large_v', 'mask_loses', 'shift1', 'shift3', 'shift5', 'shift7',
                   'shift4_8x16', 'shift4_16x8', 'shift4_8x8')


def attention_probs(case):
    """fp64 softmax probabilities (units, heads, 64 queries, 64 keys) of a case, from fp64_ref's index maps: logits = scale q.k + bias
    (+ the ADDITIVE -100 mask, as the reference has it)."""
    import fp64_ref as R
    c, heads = case['c'], case['heads']
    qkv = case['qkv'].reshape(-1, 3, heads, 32).astype(np.float64)
    bias = case['table'].astype(np.float64)[R.rel_index(8).reshape(-1)].reshape(64, 64, heads).transpose(2, 0, 1)
    out = []
    for tk, lab in zip(case['toks'], case['labs']):
        q, k = qkv[tk, 0].transpose(1, 0, 2), qkv[tk, 1].transpose(1, 0, 2)          # (heads, 64, 32)
        logit = 32 ** -0.5 * q @ k.transpose(0, 2, 1) + bias
        if case['shift']:
            logit = logit + np.where(lab[:, None] != lab[None, :], -100.0, 0.0)[None]
        logit -= logit.max(-1, keepdims=True)
        p = np.exp(logit)
        out.append(p / p.sum(-1, keepdims=True))
    return np.stack(out)

"""The oracle's exp / erf / SiLU / GELU (oracle/femasr_oracle.c, the same specification as csrc/detmath.h) against fp64 on the whole
sweep set of tests/math_range.py, the set's own witness counts, and the conditions the softmax-extremes cases of
tests/test_gpu_math_range.py rely on - all without a GPU.

Bounds (u = 2^-24), taken from the project or derived, none tuned to the measurement:
  exp    relative <= 2u on [-87, 88] (outside: the value at the clamp; NaN: exp(-87), the fmaxf/fminf clamp).  The degree-7 Taylor
         remainder on |r| <= ln2 / 2 is r^8 / 8! <= 5.2e-9 = 0.09u relative to exp(r) >= 0.7; the Cody-Waite reduction is exact in its
         first step (n * 0.693359375 has <= 17 significant bits) and rounds once in the second (<= u |r| <= 0.35u, which exp' = exp
         passes on as 0.35u relative); the seven Horner fmafs each round once to a value near 1, the last one's error reaching the
         result whole, the earlier ones' damped by |r| <= 0.35 per step (0.35 + 0.35^2 + ... <= 0.54).  For p in [1, 1.42] a rounding
         is <= u of p: 1 + 0.54 = 1.54u; for p in [0.7, 1) it is <= 2^-25: (0.5 + 0.54) / 0.7 = 1.49u.  The scaling by 2^n is exact
         (n >= -126 on [-87, 88], no subnormal result).  0.09 + 0.35 + 1.54 = 1.98u < 2u.  Measured: 1.324u.
  SiLU   relative <= PRO_ERR[False] = 3u (tests/fp64_ref.py) for x >= -87, |x| > 1e-37.  Measured: 2.882u.
  erf    absolute <= 1.3e-7 (csrc/detmath.h's claim).  Measured: 1.261e-7.
  GELU   absolute <= 2e-6 for |x| <= 8 (tests/test_oracle_units.py's figure), measured 4.474e-7; relative <= 3u for x > 8 (erf is
         exactly 1 there: one multiply by 0.5, exact, and one by 2.0f, exact) - asserted from x >= 2^-10 on, measured 2.84u.  For
         x < -8 the true value x Phi(x) is below 5e-15 in magnitude and the specification gives -0 (1 + erf = 1 - 1): a relative
         bound cannot hold where the result is 0, so there the test requires x Phi(-8) <= y <= 0 (y = -0 in fact).
  SiLU below -87 (exp(-x) saturates at exp(88)): |silu(x)| <= |x| e^-87 (1 + 2^-22) - NOT -> -0: silu(-3.4e38) = -2.06.
The measured maxima are printed (pytest -s) and recorded in profiles/math_range_report.txt.
"""
import math

import numpy as np
import pytest
import torch

import fp64_ref as R
import math_range as M
from oracle import oracle as orc

U = 2.0 ** -24


@pytest.fixture(scope='module')
def sweep():
    x = M.sweep_set()
    return x, x.astype(np.float64)


def _rel(got, ref, sel):
    return float(np.max(np.abs(got[sel].astype(np.float64) - ref[sel]) / np.abs(ref[sel])))


def test_sweep_set_keeps_its_witnesses():
    """The set cannot quietly lose the points that tell a wrong rounding or a moved clamp apart.  Counts of this construction:
    27 048 525 points, 16 380 subnormals, 253 points inside the clamp where fl(x log2e) is exactly k + 1/2 (207 distinct values of
    k + 1/2), on 127 of which round-half-even and round-half-up differ."""
    wt = M.witnesses()
    print('sweep set:', wt)
    assert wt['points'] >= 27_048_525 and wt['subnormals'] >= 16380
    assert wt['clamp_neighbours'], '-87, 88 and +-4 must each be present with both neighbours'
    assert wt['half_points'] >= 253 and wt['half_even_differs'] >= 127
    assert wt['specials']
    x = M.sweep_set()
    assert np.all(np.diff(x.view(np.uint32).astype(np.int64)) > 0), 'sorted by bit pattern, unique'
    ws = M.witnesses(M.call_site_set())
    print('call-site set:', ws)
    assert ws['points'] <= 131072 and ws['clamp_neighbours'] and ws['specials'] and ws['half_even_differs'] >= 127 and ws['subnormals'] >= 256
    fin = M.call_site_set(finite=True, cap=2.0 ** 100)
    assert np.isfinite(fin).all() and np.abs(fin).max() <= 2.0 ** 100 and fin.size > 65536
    assert M.call_site_set(1000).size == 1000 and M.call_site_set(200000).size == 200000
    ex = (fin.view(np.uint32) >> 23) & 0xff
    assert set(range(0, 227)) <= set(ex.tolist()), 'every exponent field up to the cap'


def test_exp_nan_and_infinities_follow_the_device_rule():
    """exp clamps with fminf(fmaxf(x, -87), 88): a NaN becomes -87 (fmaxf returns its other operand), so exp(NaN) = exp(-87) and no NaN
    reaches the integer conversion; erf(NaN) = +-erf(4) = +-1 (fminf(|NaN|, 4) = 4, the sign bit of the NaN: DESIGN section 4); SiLU and
    GELU propagate a NaN (x itself is an operand of the final divide / multiply); GELU(-inf) = -inf * 0 = NaN."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    e = orc.math_eval('exp', np.array([nan, -87.0, inf, 88.0, -inf, -1e30, 1e30], np.float32))
    assert e[0].view(np.uint32) == e[1].view(np.uint32) == e[4].view(np.uint32) == e[5].view(np.uint32)
    assert e[2].view(np.uint32) == e[3].view(np.uint32) == e[6].view(np.uint32) and np.isfinite(e).all()
    assert abs(float(e[1]) / math.exp(-87.0) - 1) < 2 * U and abs(float(e[3]) / math.exp(88.0) - 1) < 2 * U
    s = orc.math_eval('silu', np.array([nan, inf, -inf], np.float32))
    assert np.isnan(s[0]) and s[1] == inf and s[2] == -inf
    g = orc.math_eval('gelu', np.array([nan, inf, -inf], np.float32))
    assert np.isnan(g[0]) and g[1] == inf and np.isnan(g[2])
    r = orc.math_eval('erf', np.array([inf, -inf, 0.0, -0.0], np.float32))
    assert r[0] == 1.0 and r[1] == -1.0 and r[2].view(np.uint32) == 0 and r[3].view(np.uint32) == 0x80000000
    rn = orc.math_eval('erf', np.array([nan, -nan, 4.0], np.float32))
    assert rn[0] == rn[2] == 1.0 and rn[1] == -1.0


def test_exp_against_fp64(sweep):
    x, xd = sweep
    got = orc.math_eval('exp', x)
    ref = np.exp(np.clip(np.where(np.isnan(xd), -87.0, xd), -87.0, 88.0))
    worst = _rel(got, ref, np.ones(x.size, bool))
    print(f'exp: max relative error {worst / U:.3f} u')
    assert worst <= 2 * U


def test_erf_against_fp64(sweep):
    x, xd = sweep
    got = orc.math_eval('erf', x)
    ref = torch.erf(torch.from_numpy(xd)).numpy()
    ok = ~np.isnan(x)
    worst = float(np.max(np.abs(got[ok] - ref[ok])))
    print(f'erf: max absolute error {worst:.4g}')
    assert worst <= 1.3e-7
    assert np.array_equal(np.signbit(got[ok]), np.signbit(x[ok])), 'erf carries the sign of x, zeros included'


def test_silu_against_fp64(sweep):
    x, xd = sweep
    got = orc.math_eval('silu', x)
    fin = np.isfinite(x)
    with np.errstate(over='ignore', invalid='ignore'):
        ref = xd / (1.0 + np.exp(-xd))
    sel = fin & (x >= np.float32(-87.0)) & (np.abs(x) > np.float32(1e-37))
    worst = _rel(got, ref, sel)
    print(f'silu: max relative error {worst / U:.3f} u on x >= -87, |x| > 1e-37')
    assert worst <= R.PRO_ERR[False] * U
    small = fin & (np.abs(x) <= np.float32(1e-37))          # x / 2 exactly, up to the subnormal rounding
    assert np.all(np.abs(got[small].astype(np.float64) - 0.5 * xd[small]) <= 2.0 ** -149)
    # below -87 the exponential saturates: |silu(x)| <= |x| e^-87 (1 + 2^-22), and it is NOT -> -0
    low = x < np.float32(-87.0)
    bound = np.abs(xd[low]) * math.exp(-87.0) * (1 + 2.0 ** -22)
    assert np.all(np.abs(got[low].astype(np.float64)) <= bound) and np.all(got[low] < 0)
    lf = low & fin
    ratio = np.abs(got[lf].astype(np.float64)) / (np.abs(xd[lf]) * 2.0 ** -126)
    print(f'silu below -87: |silu(x)| / (|x| 2^-126) in [{ratio.min():.5f}, {ratio.max():.5f}]; '
          f"silu(-3.4e38) = {float(orc.math_eval('silu', np.array([-3.4e38], np.float32))[0]):.3f}")
    assert np.isnan(got[np.isnan(x)]).all()


def test_gelu_against_fp64(sweep):
    x, xd = sweep
    got = orc.math_eval('gelu', x)
    with np.errstate(invalid='ignore'):
        ref = 0.5 * xd * (1.0 + torch.erf(torch.from_numpy(xd / math.sqrt(2.0))).numpy())
    mid = np.abs(x) <= np.float32(8.0)
    worst_abs = float(np.max(np.abs(got[mid] - ref[mid])))
    pos = np.isfinite(x) & (x >= np.float32(2.0 ** -10))
    worst_rel = _rel(got, ref, pos)
    print(f'gelu: max absolute error {worst_abs:.4g} on |x| <= 8; max relative error {worst_rel / U:.3f} u on x >= 2^-10')
    assert worst_abs <= 2e-6
    assert worst_rel <= 3 * U
    neg = np.isfinite(x) & (x < np.float32(-8.0))
    phi8 = 0.5 * math.erfc(8.0 / math.sqrt(2.0))
    assert np.all(got[neg] <= 0) and np.all(got[neg].astype(np.float64) >= xd[neg] * phi8)
    assert got[x == np.inf][0] == np.inf and np.isnan(got[np.isnan(x) | (x == -np.inf)]).all()


def test_fast_silu_bound_is_consistent():
    """The bound of test_gpu_math_range.py's fast-SiLU test, evaluated on the call-site set: above the IEEE form's own error (the oracle
    passes it), and equal to PRO_ERR[True] = 8 ulp of |silu| where (1 - sigma(t)) (1.3 |t| + 2) = 3.5, i.e. at t = -1.67: the bound
    guarantees the constant for t >= -1.6 only (tests/fp64_ref.py)."""
    t = M.call_site_set(finite=True).astype(np.float64)
    t = t[(t >= -80) & (np.abs(t) > 1e-37)]
    with np.errstate(over='ignore'):
        sig = 1.0 / (1.0 + np.exp(-t))
    got = orc.math_eval('silu', t.astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(got - t * sig) <= M.fast_silu_bound(t))
    assert M.fast_silu_bound(np.array([10.0]))[0] / (U * 10.0 * (1 / (1 + math.exp(-10.0)))) < 4.6
    neg = M.fast_silu_bound(np.array([-20.0]))[0] / (U * 20.0 / (1 + math.exp(20.0)))
    assert 30 < neg < 33          # 4.5 + 1.3 * 20 + 2 ulp of |silu| at t = -20: four times PRO_ERR[True]
    at = lambda t: M.fast_silu_bound(np.array([t]))[0] / (U * abs(t) / (1 + math.exp(-t)))
    assert at(-1.6) < 8.0 < at(-1.7)


@pytest.fixture(scope='module')
def dominant():
    case = M.attention_case('dominant')
    return case, M.attention_probs(case)


def test_dominant_key_visits_every_slot(dominant):
    """The dominant-key case: in unit t the query at in-window position i has its maximum at key (i - t) mod 64, with more than 0.99 of
    the probability; over the 64 (window, head) units every query row therefore has its maximum at each of the 64 key slots once (each
    accumulator register of each half-wave of the score tile)."""
    case, p = dominant
    am = p.argmax(-1)                      # (units, heads, 64)
    seen = np.zeros((64, 64), int)
    for un, win in enumerate(case['wins']):
        for hd in range(case['heads']):
            t = case['t_of'][(win, hd)]
            assert np.array_equal(am[un, hd], (np.arange(64) - t) % 64), (win, hd, t)
            seen[np.arange(64), am[un, hd]] += 1
    assert np.all(seen == 1)
    assert p.max(-1).min() > 0.99


def test_mask_that_loses_on_fp64_alone():
    """The mask-that-loses case: the reference's mask is ADDITIVE (-100, not -inf), so keys that share a +250 logit component win
    through it.  On the fp64 probabilities alone: in every masked window (one that holds two regions) some query puts > 0.99 of its
    probability on keys of ANOTHER region."""
    case = M.attention_case('mask_loses')
    p = M.attention_probs(case)
    masked_windows = 0
    for un, lab in enumerate(case['labs']):
        if np.unique(lab).size == 1:
            continue
        masked_windows += 1
        other = lab[:, None] != lab[None, :]                            # (64 queries, 64 keys)
        on_masked = (p[un] * other[None]).sum(-1)                       # (heads, 64)
        assert np.all(on_masked.max(-1) > 0.99), (case['wins'][un], on_masked.max(-1))
    assert masked_windows == case['b'] * 3          # of the 2 x 2 windows of a 16 x 16 image: last row, last column, corner


def test_attention_cases_against_fp64_on_the_oracle():
    """Every softmax-extremes case, the oracle against fp64_ref.attention_ref on all windows with that reference's own bound (the GPU
    test compares the kernel with both); the outputs stay finite."""
    for name in M.ATTENTION_CASES + ('nan_key',):
        c = M.attention_case(name)
        got = orc.window_attention(c['qkv'], c['b'], c['h'], c['w'], c['c'], c['heads'], c['shift'], c['table'])
        assert np.isfinite(got).all(), name
        if name == 'nan_key':           # a NaN logit loses the softmax (weight exp(-87)) instead of poisoning the row
            assert np.isnan(c['qkv']).sum() == 4 * c['heads']
            continue
        rows, ref, bound = R.attention_ref(torch.from_numpy(c['qkv'].reshape(-1, 3 * c['c'])), c['b'], c['h'], c['w'], c['c'], c['heads'],
                                           c['shift'], c['table'], c['wins'])
        assert len(rows) == c['b'] * c['h'] * c['w']
        R.check(got.reshape(-1, c['c'])[rows], ref, bound, name)

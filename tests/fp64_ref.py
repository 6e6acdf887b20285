"""fp64 restatements of the network's kernel operations, their error bounds, and the inventories of the launches the benchmarked
workloads make (WORKLOADS, tests/test_gpu_fp64_anchor.py) and of those the CLI and the Python API make by default (PRODUCT_WORKLOADS,
tests/test_gpu_product_anchor.py); CPU self-checks in tests/test_fp64_anchor_host.py, case runners in tests/anchor_cases.py.

Nothing here reads the oracle: each reference is the plain definition of the operation, evaluated in float64 with torch at sampled
output positions (the network's inputs are gathered on whichever device holds them).

Bounds, per element, u = 2^-24:
  conv / linear   |got - ref| <= C_FORM[form] * u * sum_k |t_k w_k| + 2u (|bias| + sum |res| + |ref|) + sum_k |w_k| e_k
                  t = the activated input (silu(a x + b), nearest-x2, + in_add), e_k its documented error (PRO_ERR), evaluated in fp64;
                  a GELU epilogue multiplies the accumulation terms by 1.2 (|gelu'| <= 1.13) and adds 4u |ref|
  GroupNorm       |da| <= C_GN u |a|,  |db| <= C_GN u (|beta| + |mean a| + |a| mean|x|)   (the last term: the mean's own rounding)
  LayerNorm       C_LN u (|gamma| rstd (|x - mean| + mean|x|) + |beta| + |ref|)
  attention       C_ATTN u (1 + max_j L_j) sum_j p_j |v_j|,  L_j = |scale| sum_d |q_d k_jd| + |bias_j|   (first order in the logits)
  VQ              index == the fp64 first-min, unless the fp64 gap to another code is within NEAR_TIE_ULP ulp of the fp32 best
                  distance (oracle/near_tie.py's rule); zq == the chosen codebook row bit for bit

C_FORM calibration (tests/test_fp64_anchor_host.py::test_calibration, the CPU oracle - bit-identical to each strict-mode kernel - at
the network's channel counts on reduced grids; worst ratio = max over elements of the c the element needs):
  form         K                worst c   C_FORM
  direct       9*64, 9*256        4.0        20    (16 until the stride-2 row below was calibrated)
  direct x2    9*256, 9*128       2.3        20    (nearest-x2 as four phase filters; decoder_math 'fp32_direct', linear_math 'fp32')
  direct s2    9*64, 9*128        4.09       20    (stride 2, the generic implicit GEMM; linear_math 'fp32')
  wino4        9*64 .. 9*256     48.7       256
  wino_up2     9*128, 9*256      61.4       256
  split3x3     9*256              1.4         8
  split1x1     256, 1024          1.2         8
  gemm_fp32    48 (Cin 3, k4)     3.0        20    (16 until the 1x1 rows below were calibrated)
  gemm_fp32    256, 1024 (1x1)    4.42       20    (the LDS-DMA GEMM at qkv 256->768 - the worst -, proj, fc1 + GELU, fc2 1024->256,
                                                    before_quant 256->512; linear_math 'fp32')
  bf16x3       9*64 .. 9*512     27.1       128    (against the CPU MODEL of the specified arithmetic, test_bf16x3_model_calibrates_its_
                                                    constant: N(0,1) inputs 19.4 / 15.7 / 14.9 / 9.6 and SiLU-shaped inputs 27.1 / 21.9 /
                                                    16.5 / 9.1 at Cin 64 / 128 / 256 / 512; never above C_BF16X3_MAX = 208, the analytic
                                                    worst case: 3 x 2^-18 for the two representation errors and the dropped lo*lo term,
                                                    + 16 for the fp32 accumulation.  What the GPU needs of it - the matrix instruction's
                                                    own accumulation - is NOT MEASURED yet: tests/test_gpu_mode_anchor.py prints the
                                                    worst err / bound per slot in its last test)
Every constant is >= 4x the worst calibrated ratio (the host test asserts it).  One bf16 rounding of the operands (no split) is
rejected by every form's constant (test_conv_bound_rejects_wrong_reference), so the constants separate fp32-grade results from
bf16-grade ones; the bf16x3 constant also rejects the model with either cross term (hi*lo, lo*hi) left out, at Cin 64 and 512, with
more than half of the elements over their own bound (test_bf16x3_bound_rejects_a_missing_cross_term).  The Winograd forms need ~10-15x the direct form's c: the transforms' rounding, not a defect.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
C_FORM = {'direct': 20.0, 'wino4': 256.0, 'wino_up2': 256.0, 'split3x3': 8.0, 'split1x1': 8.0, 'gemm_fp32': 20.0, 'bf16x3': 128.0}
C_BF16X3_MAX = 3 * 2.0 ** -18 / 2.0 ** -24 + 16.0     # 208: two representation errors + the dropped lo*lo term, + 16 for the fp32 accumulation:
                                                      # frozen at that figure on purpose (the tighter cap); it does not follow C_FORM['direct']
PRO_ERR = {False: 3.0, True: 8.0}       # SiLU error in ulp of |silu|: IEEE expf / division (exact), v_exp_f32 + v_rcp_f32 (fast_act,
                                        # and the bf16x3 kernels' prologue in every mode)
# Range of validity (tests/test_gpu_math_range.py, tests/test_math_range_host.py; profiles/math_range_report.txt).  PRO_ERR[False] = 3
# holds for every x >= -87 with |x| > 1e-37 (measured 2.882 on 27 million points; below -87 exp saturates and |silu| <= |x| e^-87).
# PRO_ERR[True] = 8 holds for t >= -5: measured on an MI355X over every unit interval of t, the largest error is 6.12 ulp of |silu|
# on [-5, -4) and 3.08 or less for t >= -1; below -5 the rounding of the exponent's argument t * -log2e dominates (about 1.3 |t|
# ulp of the exponential, all of which reaches silu once 1 - sigma(t) is near 1): 8.77 on [-6, -5), 17 near -20, 33 near -40, 64
# near -80.  Guaranteed by the derived bound u |silu| (4.5 + (1 - sigma(t)) (1.3 |t| + 2)) only for t >= -1.6.  The conv anchors
# that use the constant stay valid because |silu(t)| itself falls as |t| e^t there: 64 ulp of |silu(-80)| is 6e-39.
C_GN, C_LN, C_ATTN = 16.0, 16.0, 16.0
NEAR_TIE_ULP = 4.0                      # oracle/near_tie.py (the one near-tie rule of the parity checks)


# ---------------------------------------------------------------- sampling
def axis_samples(n, tile, extra=(), rng=None, nrand=3):
    """Border rows / columns, the seams of `tile`-wide tiles (both sides), the last (partial) tile, plus random ones."""
    s = {0, 1, n - 2, n - 1}
    for t in tile:
        last = (n - 1) // t * t
        s |= {t - 1, t, last - 1, last, min(last + t - 1, n - 1)}
    s |= set(extra)
    if rng is not None:
        s |= set(int(v) for v in rng.integers(0, n, nrand))
    return sorted(v for v in s if 0 <= v < n)


def straddle_images(B, image_bytes, step=2 ** 31):
    """The images of a (B, ...) tensor of `image_bytes` bytes per image that hold a multiple of `step` bytes (the image a 32-bit
    byte offset, signed or unsigned, wraps in) and the image after each: sorted indices, empty when the tensor is <= `step` bytes."""
    s = set()
    k = step
    while k < B * image_bytes:
        n = k // image_bytes                     # byte k is in image n (or is its first byte)
        s |= {n, min(n + 1, B - 1)}
        if k % image_bytes == 0 and n > 0:       # the boundary is an image seam: the image that ends there too
            s.add(n - 1)
        k += step
    return sorted(s)


def conv_positions(B, Ho, Wo, seed, tiles_y=(8, 16), tiles_x=(16,), max_pos=900, images=()):
    """(S, 3) int64 (n, y, x): the structured rows x columns on the first and the last image and on every image of `images`
    (straddle_images: where the offsets of a large tensor wrap; max_pos applies per image), random positions on all images."""
    rng = np.random.default_rng(seed)
    ys, xs = axis_samples(Ho, tiles_y, rng=rng), axis_samples(Wo, tiles_x, rng=rng)
    imgs = sorted({0, B - 1} | {int(n) for n in images if 0 <= n < B})
    grid = [(n, y, x) for n in imgs for y in ys for x in xs]
    max_pos = max_pos * max(1, (len(imgs) + 1) // 2)
    if len(grid) > max_pos:
        keep = rng.choice(len(grid), max_pos, replace=False)
        border = [i for i, (n, y, x) in enumerate(grid) if y in (0, Ho - 1) or x in (0, Wo - 1)]
        grid = [grid[i] for i in sorted(set(keep.tolist()) | set(border))]
    r = np.stack([rng.integers(0, B, 64), rng.integers(0, Ho, 64), rng.integers(0, Wo, 64)], 1)
    return np.concatenate([np.asarray(grid, np.int64).reshape(-1, 3), r.astype(np.int64)])


# ---------------------------------------------------------------- conv
def gather_taps(x, pos, ksz, stride, pad, up2, phase_shift=0):
    """x (B,H,W,C) tensor -> (S, ksz*ksz, C) float64 CPU patches of the (virtual, nearest-x2 when up2) input under each output
    position, zeros outside, and the (S, ksz*ksz) validity mask.  phase_shift: a deliberately wrong x2 source map (self-checks)."""
    B, H, W, C = x.shape
    Hv, Wv = (2 * H, 2 * W) if up2 else (H, W)
    p = torch.as_tensor(pos, device=x.device)
    d = torch.arange(ksz, device=x.device)
    vy = p[:, 1, None] * stride - pad + d[None, :]              # (S, k)
    vx = p[:, 2, None] * stride - pad + d[None, :]
    vy = vy[:, :, None].expand(-1, ksz, ksz).reshape(len(p), -1)
    vx = vx[:, None, :].expand(-1, ksz, ksz).reshape(len(p), -1)
    ok = (vy >= 0) & (vy < Hv) & (vx >= 0) & (vx < Wv)
    sy = (vy + phase_shift) // 2 if up2 else vy
    sx = (vx + phase_shift) // 2 if up2 else vx
    sy, sx = sy.clamp(0, H - 1), sx.clamp(0, W - 1)
    n = p[:, 0, None].expand_as(sy)
    t = x[n, sy, sx].to('cpu', torch.float64)                  # (S, k*k, C)
    return t, ok.cpu()


def conv_ref(x, w_oihw, bias, pos, ksz, stride=1, pad=1, up2=False, pro=None, fast_act=False, in_add=None, res=(), act=0,
             mutate=None):
    """fp64 conv at `pos` (S,3): returns (ref (S,Cout), mag = sum|t w| (S,Cout), pro_term = sum |w| e (S,Cout), rest (S,Cout)).
    x NHWC (any device), w_oihw / bias CPU float32 arrays, pro = (a, b) per (n, c) float32 arrays, res = NHWC residual tensors.
    mutate: None or one of 'drop_border_tap', 'neighbour_bias', 'drop_residual', 'bf16_operands', 'phase_swap' (self-checks)."""
    t, ok = gather_taps(x, pos, ksz, stride, pad, up2, phase_shift=1 if mutate == 'phase_swap' else 0)
    if in_add is not None:
        t2, _ = gather_taps(in_add, pos, ksz, stride, pad, up2)
        e_in = U * (t + t2).abs()                              # the fp32 add while staging
        t = t + t2
    else:
        e_in = torch.zeros_like(t)
    n = torch.as_tensor(pos[:, 0])
    if pro is not None:
        a = torch.as_tensor(np.asarray(pro[0]), dtype=torch.float64)[n][:, None, :]
        b = torch.as_tensor(np.asarray(pro[1]), dtype=torch.float64)[n][:, None, :]
        z = a * t + b
        s = z * torch.sigmoid(z)
        # fmaf rounding (|silu'| <= 1.1) + the SiLU's own error
        e = 1.1 * (U * z.abs() + a.abs() * e_in) + PRO_ERR[bool(fast_act)] * U * s.abs()
        t = s
    else:
        e = e_in
    t = t * ok[:, :, None]
    e = e * ok[:, :, None]
    if mutate == 'drop_border_tap':          # the last valid tap of every position
        last = (ok.cumsum(1) == ok.sum(1, keepdim=True)) & ok
        t = t * (~last)[:, :, None]
    w = torch.as_tensor(np.asarray(w_oihw, np.float32), dtype=torch.float64)      # (O, I, kh, kw)
    wk = w.permute(2, 3, 1, 0).reshape(ksz * ksz * w.shape[1], w.shape[0])         # [(ky, kx, c)][o]
    tf = t.reshape(len(pos), -1)
    if mutate == 'bf16_operands':
        tf = tf.to(torch.float32).to(torch.bfloat16).to(torch.float64)
        wk = wk.to(torch.float32).to(torch.bfloat16).to(torch.float64)
    acc = tf @ wk
    mag = tf.abs() @ wk.abs()
    pro_term = e.reshape(len(pos), -1) @ wk.abs()
    bb = torch.as_tensor(np.asarray(bias, np.float32), dtype=torch.float64)
    if mutate == 'neighbour_bias':
        bb = torch.roll(bb, 1)
    ref = acc + bb[None, :]
    if act == 1:
        ref = 0.5 * ref * (1.0 + torch.erf(ref / math.sqrt(2.0)))
        mag, pro_term = 1.2 * mag, 1.2 * pro_term
    rest = bb.abs()[None, :].expand_as(ref).clone()
    p = torch.as_tensor(pos)
    for i, r in enumerate(res):
        if r is None:
            continue
        rv = r[p[:, 0].to(r.device), p[:, 1].to(r.device), p[:, 2].to(r.device)].to('cpu', torch.float64)
        rest = rest + rv.abs()
        if not (mutate == 'drop_residual' and i == len(res) - 1):
            ref = ref + rv
    rest = rest + ref.abs() * (3.0 if act == 1 else 1.0)
    return ref, mag, pro_term, rest


def conv_bound(mag, pro_term, rest, form):
    """(form 'bf16x3': evaluate conv_ref with fast_act=True - the kernel's prologue SiLU is the hardware one in every mode.)"""
    return C_FORM[form] * U * mag + 2.0 * U * rest + pro_term


def check(got, ref, bound, what):
    """Returns the worst err / bound; raises with the worst element if any element is over its bound."""
    got = torch.as_tensor(got, dtype=torch.float64)
    err = (got - ref).abs()
    ratio = err / bound.clamp_min(1e-300)
    worst = float(ratio.max())
    if not worst <= 1.0:
        i = int(torch.argmax(torch.nan_to_num(ratio, nan=float('inf'))))
        idx = np.unravel_index(i, tuple(ratio.shape))
        raise AssertionError(f'{what}: err / bound = {worst:.3g} at {idx}: got {float(got.reshape(-1)[i])!r} '
                             f'ref {float(ref.reshape(-1)[i])!r} bound {float(bound.reshape(-1)[i]):.3e}')
    return worst


def check_whole_conv3x3(x, w_khwc, bias, got, form, up2=False, pro=None, res=(), what='conv'):
    """Every element of a small 3x3 stride-1 pad-1 conv output `got` (B, Ho, Wo, Cout) against fp64 with the per-element bound of
    `form` (numpy inputs; w_khwc [3][3][Cin][Cout] as the unit tests hold it; res: the residual arrays given, None entries skipped).
    Returns the worst err / bound."""
    B, Ho, Wo, _ = got.shape
    n, y, xx = np.meshgrid(np.arange(B), np.arange(Ho), np.arange(Wo), indexing='ij')
    pos = np.stack([n.reshape(-1), y.reshape(-1), xx.reshape(-1)], 1).astype(np.int64)
    rs = [torch.as_tensor(np.asarray(r, np.float32)) for r in res if r is not None]
    ref, mag, pt, rest = conv_ref(torch.as_tensor(np.asarray(x, np.float32)), np.asarray(w_khwc, np.float32).transpose(3, 2, 0, 1),
                                  bias, pos, 3, 1, 1, up2, pro=pro, fast_act=form == 'bf16x3', res=rs)
    g = torch.as_tensor(np.asarray(got, np.float32)).reshape(len(pos), -1)
    return check(g, ref, conv_bound(mag, pt, rest, form), what)


def rejects(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


# ---------------------------------------------------------------- GroupNorm
def gn_coeffs_ref(x, gamma, beta, groups=32, eps=1e-6, group_shift=0):
    """(a, b, bound_a, bound_b) (B, C) float64 CPU: a = gamma rstd, b = beta - mean a over the (c / (C/groups)) group.
    x NHWC on any device; moments in fp64 on its device.  group_shift: a deliberately wrong channel -> group map (self-checks)."""
    B, H, W, C = x.shape
    cg = C // groups
    if B > 1 and x.numel() > 2 ** 28:          # large launches: image by image, so the fp64 copies stay one image in size
        parts = [gn_coeffs_ref(x[n:n + 1], gamma, beta, groups, eps, group_shift) for n in range(B)]
        return tuple(torch.cat([p[i] for p in parts]) for i in range(4))
    xd = x.to(torch.float64)
    s1 = xd.sum((1, 2))                                          # (B, C)
    s2 = (xd * xd).sum((1, 2))
    g_of = (torch.arange(C, device=x.device) + group_shift).clamp(0, C - 1) // cg
    m1 = torch.zeros(B, groups, dtype=torch.float64, device=x.device).index_add_(1, torch.arange(C, device=x.device) // cg, s1)
    m2 = torch.zeros(B, groups, dtype=torch.float64, device=x.device).index_add_(1, torch.arange(C, device=x.device) // cg, s2)
    ma = torch.zeros(B, groups, dtype=torch.float64, device=x.device).index_add_(1, torch.arange(C, device=x.device) // cg,
                                                                                 xd.abs().sum((1, 2)))
    cnt = H * W * cg
    mean = m1 / cnt
    var = (m2 / cnt - mean * mean).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    mean_c, rstd_c, mabs_c = mean[:, g_of].cpu(), rstd[:, g_of].cpu(), (ma / cnt)[:, g_of].cpu()
    g = torch.as_tensor(np.asarray(gamma, np.float32), dtype=torch.float64)[None]
    bt = torch.as_tensor(np.asarray(beta, np.float32), dtype=torch.float64)[None]
    a = g * rstd_c
    b = bt - mean_c * a
    return a, b, C_GN * U * a.abs(), C_GN * U * (bt.abs() + (mean_c * a).abs() + a.abs() * mabs_c)


# ---------------------------------------------------------------- LayerNorm
def layernorm_ref(x_rows, gamma, beta, eps=1e-5):
    """x_rows (S, C) float64 -> (ref, bound)."""
    g = torch.as_tensor(np.asarray(gamma, np.float32), dtype=torch.float64)[None]
    b = torch.as_tensor(np.asarray(beta, np.float32), dtype=torch.float64)[None]
    mean = x_rows.mean(1, keepdim=True)
    var = ((x_rows - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    ref = (x_rows - mean) * rstd * g + b
    bound = C_LN * U * (g.abs() * rstd * ((x_rows - mean).abs() + x_rows.abs().mean(1, keepdim=True)) + b.abs() + ref.abs())
    return ref, bound


# ---------------------------------------------------------------- window attention (network_swinir.py WindowAttention, ws 8)
def rel_index(ws=8):
    c = np.stack(np.meshgrid(np.arange(ws), np.arange(ws), indexing='ij')).reshape(2, -1)
    r = (c[:, :, None] - c[:, None, :]).transpose(1, 2, 0) + (ws - 1)
    return r[..., 0] * (2 * ws - 1) + r[..., 1]                  # (64, 64)


def region_ids(H, W, ws, shift):
    """Region label of each SHIFTED-frame pixel (the img_mask slices of SwinTransformerBlock.calculate_mask)."""
    def lab(n):
        v = np.zeros(n, np.int64)
        if shift:
            v[n - ws:n - shift] = 1
            v[n - shift:] = 2
        return v
    return lab(H)[:, None] * 3 + lab(W)[None, :]


def attention_ref(qkv, b, H, W, C, heads, shift, table, windows, ws=8, mask_shift=0):
    """Output rows of the listed windows (n, wy, wx) of the SHIFTED frame: returns (rows (S,) int64 token indices in the input
    layout, ref (S, C), bound (S, C)) in float64.  qkv (B*H*W, 3C) tensor on any device.  mask_shift: the region map moved by one
    window (self-checks)."""
    hd = C // heads
    scale = hd ** -0.5
    ri = torch.as_tensor(rel_index(ws))
    tab = torch.as_tensor(np.asarray(table, np.float32), dtype=torch.float64)     # (225, heads)
    bias = tab[ri.reshape(-1)].reshape(ws * ws, ws * ws, heads).permute(2, 0, 1)   # (heads, 64, 64)
    reg = region_ids(H, W, ws, shift)
    if mask_shift:
        reg = np.roll(reg, ws * mask_shift, axis=1)
    rows_all, ref_all, bnd_all = [], [], []
    for (n, wy, wx) in windows:
        sy = wy * ws + np.arange(ws)[:, None]
        sx = wx * ws + np.arange(ws)[None, :]
        oy, ox = (sy + shift) % H, (sx + shift) % W                               # shifted frame -> input layout
        rows = (n * H * W + oy * W + ox).reshape(-1)
        t = qkv[torch.as_tensor(rows, device=qkv.device)].to('cpu', torch.float64)    # (64, 3C)
        q, k, v = t[:, :C], t[:, C:2 * C], t[:, 2 * C:]
        q = q.reshape(64, heads, hd).transpose(0, 1)
        k = k.reshape(64, heads, hd).transpose(0, 1)
        v = v.reshape(64, heads, hd).transpose(0, 1)
        logit = scale * q @ k.transpose(1, 2) + bias
        lmag = scale * q.abs() @ k.abs().transpose(1, 2) + bias.abs()
        if shift:
            r = torch.as_tensor(reg[sy, sx].reshape(-1))
            logit = logit + torch.where(r[:, None] != r[None, :], -100.0, 0.0)[None]
        p = torch.softmax(logit, -1)
        out = (p @ v).transpose(0, 1).reshape(64, C)
        pv = (p @ v.abs()).transpose(0, 1).reshape(64, C)
        lm = lmag.amax(-1).transpose(0, 1).repeat_interleave(hd, 1)             # (64, C) max_j L_j per head
        rows_all.append(rows)
        ref_all.append(out)
        bnd_all.append(C_ATTN * U * (1.0 + lm) * pv)
    return np.concatenate(rows_all), torch.cat(ref_all), torch.cat(bnd_all)


def attention_windows(B, H, W, ws, seed, nrand=6, images=()):
    """Every border window of the first and the last image (the shifted-mask windows are the last row / column) and of `images`,
    plus random ones."""
    nwy, nwx = H // ws, W // ws
    s = set()
    for n in sorted({0, B - 1} | {int(n) for n in images if 0 <= n < B}):
        for wy in range(nwy):
            s |= {(n, wy, 0), (n, wy, nwx - 1)}
        for wx in range(nwx):
            s |= {(n, 0, wx), (n, nwy - 1, wx)}
    rng = np.random.default_rng(seed)
    for _ in range(nrand):
        s.add((int(rng.integers(0, B)), int(rng.integers(0, nwy)), int(rng.integers(0, nwx))))
    return sorted(s)


# ---------------------------------------------------------------- VQ
def vq_check(z_rows, codebook, idx, zq, rows, what, runner_up=False):
    """z_rows (M, D) tensor, codebook (N, D) float32 array, idx (M,) int64 tensor, zq (M, D) tensor; checks the sampled rows.
    runner_up: check against the fp64 runner-up instead of the best (self-checks).  Returns the smallest fp64 gap seen (in ulp)."""
    cb = torch.as_tensor(np.asarray(codebook, np.float32))
    cbd = cb.to(torch.float64)
    z = z_rows[torch.as_tensor(rows, device=z_rows.device)].to('cpu', torch.float64)
    d = (z * z).sum(1, keepdim=True) + (cbd * cbd).sum(1)[None] - 2.0 * z @ cbd.T       # (S, N)
    order = torch.argsort(d, dim=1, stable=True)
    best, second = order[:, 0], order[:, 1]
    db = d.gather(1, best[:, None])[:, 0]
    ulp = torch.as_tensor(np.spacing(np.abs(db.numpy().astype(np.float32))), dtype=torch.float64)
    got = idx[torch.as_tensor(rows, device=idx.device)].cpu()
    want = second if runner_up else best
    gap_ulp = (d.gather(1, got[:, None])[:, 0] - db) / ulp
    for i in range(len(rows)):
        g, w = int(got[i]), int(want[i])
        if g != w and not (not runner_up and float(gap_ulp[i]) <= NEAR_TIE_ULP):
            raise AssertionError(f'{what}: row {int(rows[i])}: index {g}, fp64 first-min {w} '
                                 f'(the pick is {float(gap_ulp[i]):.3g} ulp of the best distance above it)')
    zr = zq[torch.as_tensor(rows, device=zq.device)].cpu()
    assert torch.equal(zr, cb[got]), f'{what}: zq is not the chosen codebook row bit for bit'
    g2 = (d.gather(1, second[:, None])[:, 0] - db) / ulp
    return float(g2.min())


def vq_rows(z_rows, codebook, seed, n=384, nclose=64):
    """Random rows plus the rows whose fp64 runner-up gap is smallest among a wider random pool, and the first / last rows."""
    M = z_rows.shape[0]
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(0, M, 4096))
    cbd = torch.as_tensor(np.asarray(codebook, np.float32), dtype=torch.float64).to(z_rows.device)
    z = z_rows[torch.as_tensor(pool, device=z_rows.device)].to(torch.float64)
    d = (z * z).sum(1, keepdim=True) + (cbd * cbd).sum(1)[None] - 2.0 * z @ cbd.T
    top = torch.topk(d, 2, largest=False).values
    close = pool[torch.argsort(top[:, 1] - top[:, 0]).cpu().numpy()[:nclose]]
    return np.unique(np.concatenate([close, rng.integers(0, M, n), [0, M - 1]]))


# ---------------------------------------------------------------- the launches of the benchmarked workloads
WORKLOADS = {
    # bench.py's headline (tiles16) and its --full legs x2b32 / hq8; bench runs 3 sub-batch streams (femasr_set_streams)
    'x4_b16_128': dict(cfg=dict(codebook_params=[[32, 1024, 512]], LQ_stage=True, scale_factor=4), batch=16, hw=128, fn='test'),
    'x2_b32_256': dict(cfg=dict(codebook_params=[[32, 1024, 512]], LQ_stage=True, scale_factor=2), batch=32, hw=256, fn='test'),
    'hq_b8_512': dict(cfg=dict(codebook_params=[[32, 1024, 512]], LQ_stage=False), batch=8, hw=512, fn='forward'),
}
BENCH_STREAMS = 3


def sub_batches(B, S):
    """model.hip sub_range: the sizes of the S sub-batches of B samples (each runs its own launches)."""
    q, r = divmod(B, S)
    return sorted({q + (1 if i < r else 0) for i in range(min(S, B))})


# ---------------------------------------------------------------- the launches the CLI and the Python API make by default
CLI_TILE, CLI_PAD, MAX_TILE_BATCH = 240, 16, 16           # inference.py / FeMaSRNet.test_tile defaults, FeMaSRNet.max_tile_batch
PRODUCT_STREAMS = (1, 2, 3)                               # num_streams: the module's default, two, the CLI's default
_X4 = dict(codebook_params=[[32, 1024, 512]], LQ_stage=True, scale_factor=4)
_X2 = dict(codebook_params=[[32, 1024, 512]], LQ_stage=True, scale_factor=2)


def tiled_calls(height, width, tile_size=CLI_TILE, tile_pad=CLI_PAD, max_tile_batch=MAX_TILE_BATCH):
    """{(h, w) window class: sorted sizes of the batched test() calls FeMaSRNet._tiled makes on one image} (one rank)."""
    from femasr_amd import tiling
    out = {}
    for hw, tl in tiling.shape_classes(tiling.enumerate_tiles(height, width, tile_size, tile_pad)).items():
        out[hw] = sorted({len(tl[i:i + max_tile_batch]) for i in range(0, len(tl), max_tile_batch)})
    return out


def _product_workloads():
    """Derived, not typed in: the tiled branch on a 1440x1440 and a 1356x2040 image (every window class, every batched call, its
    sub-batches at 1, 2 and 3 streams) and the whole-image branch (h*w < 600^2) at B = 1."""
    W = {}
    for (ih, iw) in ((1440, 1440), (1356, 2040)):
        for (h, w), calls in tiled_calls(ih, iw).items():
            subs = sorted({b for c in calls for s in PRODUCT_STREAMS for b in sub_batches(c, s)})
            W[f'tiled{ih}x{iw}_win{h}x{w}'] = dict(cfg=_X4, hw=(h, w), fn='test', sub_batches=subs, calls=calls)
    for (h, w) in ((599, 599), (339, 510), (16, 600)):
        W[f'whole{h}x{w}_x4'] = dict(cfg=_X4, hw=(h, w), fn='test', sub_batches=[1], calls=[1])
    W['whole599x599_x2'] = dict(cfg=_X2, hw=(599, 599), fn='test', sub_batches=[1], calls=[1])
    return W


PRODUCT_WORKLOADS = _product_workloads()        # (separate from WORKLOADS: the bench-anchored tests and their ids stay as they are)


def _wino_ok(B, H, W, cin, cout, up2):
    # kernels_wino.hip / kernels_wino_up2.hip shape rules at the default limits (32-bit byte offsets)
    if cin % 32 or cout % 64 or cin > 1024:
        return False
    ho, wo = (2 * H, 2 * W) if up2 else (H, W)
    return (B * H * W * cin < 2 ** 31 and B * ho * wo * cout < 2 ** 31 and H * W * cin < 2 ** 27 and ho * wo * cout < 2 ** 27
            and 36 * cin * cout < 2 ** 29)


def _bf16x3_ok(L):
    # kernels_conv_bf16.hip femasr_conv_bf16x3_shape_ok (32-bit element offsets into the input and the output)
    return (L['ksz'] == 3 and L['stride'] == 1 and L['pad'] == 1 and L['cin'] % 32 == 0 and L['cin'] <= 1024 and L['act'] == 0
            and not (L['up2'] and L['pro']) and L['B'] * L['H'] * L['W'] * L['cin'] < 2 ** 31
            and L['B'] * L['H'] * L['W'] * (4 if L['up2'] else 1) * L['cout'] < 2 ** 31)


def workload_layers(cfg, batch, hw, fn, weight_shapes, decoder_math='fp32'):
    """The conv / linear layers and the small kernels one sub-batch of the workload runs, in order, on inputs of hw = side or (h, w)
    pixels, with the shapes the network's resolution schedule gives them (femasr_arch.py geometry, model.hip plan_geometry / run_tail) and the channel counts of the
    architecture's weights.  Returns a list of dicts; conv entries: key, B, H, W, cin, cout, ksz, stride, pad, up2, pro (GN+SiLU
    prologue), nres, act, behind (decoder side of the single lookup), gn_out (the output feeds a GroupNorm).
    decoder_math decides where the encoder skip of a decoder stage is added (model.hip run_tail): by the NEXT stage's x2 conv while it
    stages its input (in_add) when that conv runs in the 'wino_up2' form under decoder_math, otherwise as a second residual (nres = 2)
    of this stage's last conv."""
    lq = cfg['LQ_stage']
    sf = cfg.get('scale_factor', 4) if lq else 1
    gt, cbs = 256, cfg['codebook_params'][0][0]
    max_depth = int(math.log2(gt // cbs))
    enc_depth = int(math.log2(gt // sf // cbs))
    h_in, w_in = (hw, hw) if isinstance(hw, int) else hw
    if fn == 'test':
        wsz = 8 // sf * 8
        H, W = (h_in // wsz + 1) * wsz, (w_in // wsz + 1) * wsz
    else:
        H, W = h_in, w_in
    B = batch
    L = []

    def co(key):
        return int(weight_shapes[key + '.weight'][0])

    def conv(key, H, W, cin, ksz=3, stride=1, pad=1, up2=False, pro=False, nres=0, act=0, behind=False, gn_out=False, in_add=False):
        L.append(dict(kind='conv', key=key, B=B, H=H, W=W, cin=cin, cout=co(key), ksz=ksz, stride=stride, pad=pad, up2=up2, pro=pro,
                      nres=nres, act=act, behind=behind, gn_out=gn_out, in_add=in_add))
        hv, wv = (2 * H, 2 * W) if up2 else (H, W)
        return (hv + 2 * pad - ksz) // stride + 1, (wv + 2 * pad - ksz) // stride + 1, co(key)

    def resblock(p, H, W, c, behind, nres2=0, gn_out=False):
        L.append(dict(kind='gn', B=B, H=H, W=W, c=c, key=p + '.conv.0.norm'))
        conv(p + '.conv.2', H, W, c, pro=True, behind=behind, gn_out=True)
        L.append(dict(kind='gn', B=B, H=H, W=W, c=c, key=p + '.conv.3.norm'))
        conv(p + '.conv.5', H, W, c, pro=True, nres=1 + nres2, behind=behind, gn_out=gn_out)

    L.append(dict(kind='pad', B=B, H=H, W=W, c=3, h_in=h_in, w_in=w_in, Hp=H, Wp=W))
    e = 'multiscale_encoder'
    h, w, c = conv(e + '.in_conv', H, W, 3, ksz=4, pad=1)
    feats = []
    bi = 0
    for i in range(enc_depth):
        p = f'{e}.blocks.{bi}'
        h, w, c = conv(p + '.0', h, w, c, stride=2)
        resblock(p + '.1', h, w, c, False, gn_out=True)
        resblock(p + '.2', h, w, c, False)
        feats.append((h, w, c))
        bi += 1
    if lq:
        p = f'{e}.blocks.{bi}'
        rows = B * h * w
        for r in range(4):
            for k in range(6):
                bp = f'{p}.swin_blks.{r}.residual_group.blocks.{k}'
                L.append(dict(kind='ln', rows=rows, c=c, key=bp + '.norm1'))
                L.append(dict(kind='conv', key=bp + '.attn.qkv', B=1, H=rows, W=1, cin=c, cout=co(bp + '.attn.qkv'), ksz=1, stride=1, pad=0,
                              up2=False, pro=False, nres=0, act=0, behind=False, gn_out=False, in_add=False))
                L.append(dict(kind='attn', B=B, H=h, W=w, c=c, shift=0 if k % 2 == 0 else 4, key=bp + '.attn'))
                L.append(dict(kind='conv', key=bp + '.attn.proj', B=1, H=rows, W=1, cin=c, cout=c, ksz=1, stride=1, pad=0,
                              up2=False, pro=False, nres=1, act=0, behind=False, gn_out=False, in_add=False))
                L.append(dict(kind='ln', rows=rows, c=c, key=bp + '.norm2'))
                L.append(dict(kind='conv', key=bp + '.mlp.fc1', B=1, H=rows, W=1, cin=c, cout=co(bp + '.mlp.fc1'), ksz=1, stride=1, pad=0,
                              up2=False, pro=False, nres=0, act=1, behind=False, gn_out=False, in_add=False))
                L.append(dict(kind='conv', key=bp + '.mlp.fc2', B=1, H=rows, W=1, cin=co(bp + '.mlp.fc1'), cout=c, ksz=1, stride=1, pad=0,
                              up2=False, pro=False, nres=1, act=0, behind=False, gn_out=False, in_add=False))
            conv(f'{p}.swin_blks.{r}.conv', h, w, c, nres=1)
        feats = [(h, w, c)]
        bi += 1
        for u in range(2):             # the LQ up-blocks make the decoder's skip features (behind the single lookup)
            p = f'{e}.blocks.{bi}'
            h, w, c = conv(p + '.1', h, w, c, up2=True, behind=True, gn_out=True)
            resblock(p + '.2', h, w, c, True, gn_out=True)
            resblock(p + '.3', h, w, c, True)
            feats.append((h, w, c))
            bi += 1
    else:
        feats = feats[::-1]
    # quantise at the codebook scale (one codebook), then the decoder
    h, w, c = feats[0]
    zc = co('before_quant_group.0')
    conv('before_quant_group.0', h, w, c, ksz=1, pad=0)
    L.append(dict(kind='vq', M=B * h * w, d=zc, key='quantize_group.0.embedding.weight'))
    h, w, c = conv('after_quant_group.0.conv', h, w, zc, behind=True)
    skip_in_next = False
    for i in range(max_depth):
        p = f'decoder_group.{i}.block'
        nxt = lq and i + 1 < max_depth
        h2, w2, c2 = 2 * h, 2 * w, co(p + '.1')
        next_wino = nxt and conv_form(dict(B=B, H=h2, W=w2, cin=c2, cout=co(f'decoder_group.{i + 1}.block.1'), ksz=3, stride=1, pad=1, up2=True,
                                           pro=False, act=0, behind=True), decoder_math, 'bf16_split') == 'wino_up2'
        h, w, c = conv(p + '.1', h, w, c, up2=True, behind=True, gn_out=True, in_add=skip_in_next)
        resblock(p + '.2', h, w, c, True, gn_out=True)
        resblock(p + '.3', h, w, c, True, nres2=1 if (nxt and not next_wino) else 0)
        skip_in_next = bool(nxt and next_wino)
    conv('out_conv', h, w, c, behind=True)
    L.append(dict(kind='crop', B=B, H=h, W=w, c=3))
    return L


def conv_form(layer, decoder_math, linear_math):
    """model.hip conv_form for one layer entry: 'bf16x3', 'wino_up2', 'wino4', 'split3x3', 'split1x1' or 'direct' (+ the GN-apply pass).
    decoder_math: 'fp32', 'fp32_strict', 'fp32_direct' or 'bf16x3'; linear_math: 'bf16_split' or 'fp32'."""
    L = layer
    if L['behind'] and decoder_math == 'bf16x3' and L['cout'] > 4 and _bf16x3_ok(L):      # out_conv: the exact VALU kernel in every mode
        return 'bf16x3'
    if L['behind'] and decoder_math in ('fp32', 'fp32_strict') and L['ksz'] == 3 and L['stride'] == 1 and L['pad'] == 1 and L['act'] == 0:
        if L['up2'] and not L['pro'] and _wino_ok(L['B'], L['H'], L['W'], L['cin'], L['cout'], True):
            return 'wino_up2'
        if not L['up2'] and _wino_ok(L['B'], L['H'], L['W'], L['cin'], L['cout'], False):
            return 'wino4'
    if linear_math == 'bf16_split' and not L['behind'] and not L['up2'] and L['cin'] % 64 == 0:
        if L['ksz'] == 3 and L['pad'] == 1 and L['stride'] in (1, 2) and L['act'] == 0 and L['cin'] <= 1024 and \
                L['B'] * L['H'] * L['W'] * L['cin'] < 2 ** 31:
            return 'split3x3'
        if L['ksz'] == 1 and L['pad'] == 0 and L['stride'] == 1:
            return 'split1x1'
    return 'direct'


def gemm_fp32_layer(layer):
    return layer['ksz'] == 1 and layer['cin'] % 32 == 0 and not layer['pro'] and not layer['up2']

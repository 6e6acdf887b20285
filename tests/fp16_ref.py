"""The checker of decoder_math='fp16' (femasr_conv_args.w_f16): the specified arithmetic restated with torch in float64, its per-element
bound, CPU models of the kernel (right and deliberately wrong ones) and the network-level emulation.  tests/test_decoder_fp16_host.py
exercises all of it on the CPU before tests/test_gpu_decoder_fp16.py lets it judge a GPU.

Specification (include/femasr_hip.h):
  t   = the activated input: silu(a x + b) with the kernel's hardware-unit SiLU, nearest-x2 folded in, zero outside the image
  t16 = fp16_rne(clamp(t, +-65504)),  w16 = fp16_rne(w);  fp16 subnormals take part with their value
  out = bias + residuals + sum_k t16_k w16_k, products exact in fp32, accumulation / bias / residuals in fp32

Bound per element, u = 2^-24 (fp64_ref.U):
  |got - conv64(t16, w16)| <= C_F16 u sum_k |t16_k w16_k| + 2u (|bias| + sum |res| + |ref|) + sum_k |w16_k| ulp16(t_k) near_k
  C_F16 = 128 = fp64_ref.C_FORM['bf16x3']: the same instruction family with fp32 accumulation and the same K blocking.  It is NOT
    measured for the f16 instruction on the CPU; the GPU test prints the worst err / bound per instantiation.
  near_k = 1 exactly where the fp64 value of the activated input lies within the prologue's documented error of an fp16 rounding
    boundary (a midpoint between neighbouring halves, or +-65504 for the clamp - which never matters at these magnitudes): the
    hardware SiLU's PRO_ERR[True] = 8 ulp of |silu| plus the fp32 rounding of a x + b seen through |silu'| <= 1.1, i.e. the very
    `e` fp64_ref.conv_ref charges the bf16x3 prologue.  There the kernel may round to the other neighbour: one fp16 ulp of t_k.
    Without a prologue near is all zero: the rounded operands are exact functions of the inputs.
"""
import numpy as np
import torch

import fp64_ref as R

C_F16 = 128.0
F16_MAX = 65504.0


# ---------------------------------------------------------------- number formats, in float64 (no double rounding through fp32)
def _quantum(v, mant_bits, min_exp):
    """Spacing of the format (mant_bits stored bits, smallest normal exponent min_exp) at |v|: 2^(max(floor(log2|v|), min_exp) - mant_bits)."""
    _, e = torch.frexp(v.abs())                       # |v| = m 2^e, m in [0.5, 1)
    e = (e - 1).clamp_min(min_exp)
    return torch.ldexp(torch.ones_like(v), e - mant_bits)


def fp16_rne(v):
    """float64 -> the nearest fp16 value (ties to even, subnormals kept), after the clamp to +-65504; returned in float64."""
    v = v.clamp(-F16_MAX, F16_MAX)
    q = _quantum(v, 10, -14)
    return (torch.round(v / q) * q).clamp(-F16_MAX, F16_MAX)     # (torch.round: half to even; v / q is exact)


def fp16_trunc(v):
    """The WRONG conversion: toward zero (v_cvt_pkrtz_f16_f32)."""
    v = v.clamp(-F16_MAX, F16_MAX)
    q = _quantum(v, 10, -14)
    return torch.trunc(v / q) * q


def bf16_rne(v):
    """The WRONG grade: operands rounded to bfloat16 (8 significand bits)."""
    q = _quantum(v, 7, -126)
    return torch.round(v / q) * q


def ulp16(v):
    return _quantum(v.clamp(-F16_MAX, F16_MAX), 10, -14)


def boundary_distance(v):
    """Distance from v to the nearest fp16 rounding boundary (midpoint of two neighbouring halves of v's binade; the spacing doubles above a
    power of two, where the nearest boundary is the one below it anyway)."""
    q = ulp16(v)
    f = v.abs() / q
    return (f - torch.floor(f) - 0.5).abs() * q


# ---------------------------------------------------------------- the reference and its bound at sampled positions
def conv_ref(x, w_oihw, bias, pos, up2=False, pro=None, res=(), operand='fp16'):
    """conv64(t16, w16) + bias + residuals at pos (S, 3) of a 3x3 stride-1 pad-1 conv: returns (ref, mag = sum |t16 w16|, near_term, rest),
    each (S, Cout) float64.  x NHWC tensor (any device), w_oihw / bias float32 arrays, pro = (a, b) per (n, c), res NHWC tensors.
    operand: 'fp16' (the specification), 'fp16_trunc' or 'bf16' (self-checks: the models the bound has to reject)."""
    rnd = {'fp16': fp16_rne, 'fp16_trunc': fp16_trunc, 'bf16': bf16_rne}[operand]
    t, ok = R.gather_taps(x, pos, 3, 1, 1, up2)
    if pro is not None:
        n = torch.as_tensor(pos[:, 0])
        a = torch.as_tensor(np.asarray(pro[0]), dtype=torch.float64)[n][:, None, :]
        b = torch.as_tensor(np.asarray(pro[1]), dtype=torch.float64)[n][:, None, :]
        z = a * t + b
        s = z * torch.sigmoid(z)
        e = 1.1 * R.U * z.abs() + R.PRO_ERR[True] * R.U * s.abs()
        near = (boundary_distance(s) <= e) | ((F16_MAX - s.abs()).abs() <= e)
        t = s
    else:
        near = torch.zeros_like(t, dtype=torch.bool)
    okf = ok[:, :, None]
    t = t * okf
    near = near & okf
    w = torch.as_tensor(np.asarray(w_oihw, np.float32), dtype=torch.float64)
    wk = rnd(w.permute(2, 3, 1, 0).reshape(9 * w.shape[1], w.shape[0]))          # [(ky, kx, c)][o]
    t16 = rnd(t).reshape(len(pos), -1)
    acc = t16 @ wk
    mag = t16.abs() @ wk.abs()
    near_term = (ulp16(t) * near).reshape(len(pos), -1) @ wk.abs()
    bb = torch.as_tensor(np.asarray(bias, np.float32), dtype=torch.float64)
    ref = acc + bb[None, :]
    rest = bb.abs()[None, :].expand_as(ref).clone()
    p = torch.as_tensor(pos)
    for r in res:
        rv = r[p[:, 0].to(r.device), p[:, 1].to(r.device), p[:, 2].to(r.device)].to('cpu', torch.float64)
        ref = ref + rv
        rest = rest + rv.abs()
    rest = rest + ref.abs()
    return ref, mag, near_term, rest


def conv_bound(mag, near_term, rest, c=C_F16):
    return c * R.U * mag + 2.0 * R.U * rest + near_term


def all_positions(B, Ho, Wo):
    n, y, x = np.meshgrid(np.arange(B), np.arange(Ho), np.arange(Wo), indexing='ij')
    return np.stack([n.reshape(-1), y.reshape(-1), x.reshape(-1)], 1).astype(np.int64)


# ---------------------------------------------------------------- CPU models of the kernel
def model_fp32_sequential(x, w_oihw, bias, pos, up2=False, pro=None, res=(), operand='fp16'):
    """The specified arithmetic with ONE fp32 accumulator per output, taps in (ky, kx, c) order: exact products (float64 holds 22 bits),
    each addition rounded to fp32; bias and residuals added last in fp32.  operand as in conv_ref.  With pro the activated input is the
    fp32 evaluation of the prologue, so near-boundary flips against the fp64 reference occur as they do on the GPU."""
    rnd = {'fp16': fp16_rne, 'fp16_trunc': fp16_trunc, 'bf16': bf16_rne}[operand]
    t, ok = R.gather_taps(x, pos, 3, 1, 1, up2)
    if pro is not None:
        n = torch.as_tensor(pos[:, 0])
        a = torch.as_tensor(np.asarray(pro[0]), dtype=torch.float32)[n][:, None, :]
        b = torch.as_tensor(np.asarray(pro[1]), dtype=torch.float32)[n][:, None, :]
        z = (a.double() * t + b.double()).float()                   # fmaf: one rounding
        t = (z * torch.sigmoid(z)).double()
    t = rnd(t * ok[:, :, None]).reshape(len(pos), -1)
    w = torch.as_tensor(np.asarray(w_oihw, np.float32), dtype=torch.float64)
    wk = rnd(w.permute(2, 3, 1, 0).reshape(9 * w.shape[1], w.shape[0]))
    acc = torch.zeros((len(pos), wk.shape[1]), dtype=torch.float32)
    for k in range(wk.shape[0]):
        acc = (acc.double() + t[:, k, None] * wk[None, k, :]).float()
    acc = acc + torch.as_tensor(np.asarray(bias, np.float32))[None, :]
    p = torch.as_tensor(pos)
    for r in res:
        acc = acc + r[p[:, 0], p[:, 1], p[:, 2]].to('cpu', torch.float32)
    return acc


# ---------------------------------------------------------------- the network-level emulation (CPU)
def emulation_net(sd, cfg, operand):
    """oracle/torch_ref.TorchRefNet whose 3x3 convs BEHIND every lookup (out_conv excluded) round input and weight once to the 16-bit
    type ('fp16' / 'bf16'; None = plain fp32 run) and accumulate in float64: what a one-pass 16-bit mode does to the image."""
    from oracle.torch_ref import TorchRefNet
    import torch.nn.functional as F
    rnd = {'fp16': fp16_rne, 'bf16': bf16_rne, None: None}[operand]

    class Net(TorchRefNet):
        def _behind(self, p):
            if p.startswith(('decoder_group.', 'after_quant_group.')):
                return True
            pre = 'multiscale_encoder.blocks.'
            return self.LQ_stage and p.startswith(pre) and int(p[len(pre):].split('.')[0]) > self.encode_depth

        def _conv(self, x, p, stride=1, pad=1):
            w = self.sd[p + '.weight']
            if rnd is None or w.shape[-1] != 3 or w.shape[0] <= 4 or not self._behind(p):
                return super()._conv(x, p, stride, pad)
            y = F.conv2d(rnd(x.double()), rnd(w.double()), None, stride=stride, padding=pad)
            return y.float() + self.sd[p + '.bias'][None, :, None, None]

    return Net(sd, codebook_params=cfg['codebook_params'], LQ_stage=cfg['LQ_stage'], scale_factor=cfg.get('scale_factor', 4))


_EMU = {}


def emulated_images(name):
    """{operand: (image, indices)} of the golden case `name` under the emulation (None = the fp32 run), computed once per session."""
    if name not in _EMU:
        from femasr_amd import synth
        from helpers import CONFIGS, cfg_name_of, load_golden, synth_weights
        g = load_golden(name)
        cn = cfg_name_of(g)
        w = synth_weights(cn, int(g['seed']), str(g['codebook']))
        x = synth.synth_input(int(g['input_seed']), tuple(g['in_shape']))
        out = {}
        for op in (None, 'fp16', 'bf16'):
            net = emulation_net(w, CONFIGS[cn], op)
            y, idx = net.forward(x) if cn == 'hq' else net.test(x, return_indices=True)
            out[op] = (y.numpy(), idx.numpy())
        _EMU[name] = out
    return _EMU[name]


def psnr(a, b, peak):
    return float(10.0 * np.log10(peak * peak / np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))

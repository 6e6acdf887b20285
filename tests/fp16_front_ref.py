"""The checker of linear_math='fp16' (one-pass fp16 for the layers in FRONT of the codebook lookup): the specified arithmetic of the fp16 GEMM
restated with torch in float64 with its per-element bound, CPU models of the kernel (right and deliberately wrong ones), the network-level
emulation and the near-tie rule that judges a flipped VQ index.  tests/test_linear_fp16_host.py exercises all of it on the CPU before
tests/test_gpu_linear_fp16.py lets it judge a GPU.

Specification of the GEMM (include/femasr_hip.h, femasr_conv_args.w_f16 with ksz = 1):
  a16 = fp16_rne(clamp(a, +-65504)),  w16 = fp16_rne(w);  fp16 subnormals take part with their value
  out = epi(bias + sum_k a16_k w16_k), products exact in fp32, accumulated in fp32; bias in fp32; GELU; one residual in fp32

Bound per element, u = 2^-24 (fp64_ref.U):
  |got - ref64| <= C u sum_k |a16_k w16_k| + 2u (|bias| + |res| + |ref64|),     C = fp64_ref.C_FORM['bf16x3'] = 128
  C is the project's constant for this instruction family (fp32 accumulation inside v_mfma_f32_32x32x16_*) and K blocking; DESIGN.md 15
  measured at least 8x room on the f16 instruction.  No prologue here, so there is no near-boundary term: the rounded operands are exact
  functions of the inputs.  The GELU epilogue is not bounded but held bit-identical to the oracle's GELU of the same launch without
  activation (the GPU test).

Near-tie rule of a flipped token i -> j (i: the fp32-grade run's code, j: the mode's), against the REFERENCE arithmetic's own distances
(CPU TorchRefNet, fp32):
  d_ref(j) - d_ref(i) <= 2 Delta |e_j - e_i|_2 + 4 ulp(d_ref(i)),     Delta = 2 max_token |z_emu - z_ref|_2
  A flip needs the perturbed distances to cross: d(j) - d(i) changes by -2 delta . (e_j - e_i) when z moves by delta, so the reference gap
  can be at most 2 |delta| |e_j - e_i|.  Delta is the largest movement of a token under the CPU emulation, doubled - the margin DESIGN.md 15
  used between GPU and emulation (measured ratio 0.93 - 1.07); 4 ulp is oracle/near_tie.py's constant for the lookup's own rounding.
"""
import numpy as np
import torch
import torch.nn.functional as F

import fp16_ref as F16
import fp64_ref as R
from oracle.near_tie import NEAR_TIE_ULP

C_GEMM = R.C_FORM['bf16x3']
FLIP_CAP = 0.05               # flipped tokens per case: at most 5 %

_RND = {'fp16': F16.fp16_rne, 'fp16_trunc': F16.fp16_trunc, 'bf16': F16.bf16_rne, None: None}


# ---------------------------------------------------------------- the GEMM: reference, bound, CPU models
def gemm_ref(a, w, bias=None, res=None, operand='fp16'):
    """a (M, K), w (N, K), bias (N) or None, res (M, N) or None, float32 tensors -> (ref, mag, rest) float64 (M, N): the exact value of
    bias + sum_k a16 w16 + res, sum_k |a16 w16| and |bias| + |res| + |ref|.  (No activation: see the module docstring.)"""
    rnd = _RND[operand]
    a16, w16 = rnd(a.detach().cpu().double()), rnd(w.detach().cpu().double())
    ref = a16 @ w16.t()
    mag = a16.abs() @ w16.abs().t()
    rest = torch.zeros_like(ref)
    if bias is not None:
        b = bias.detach().cpu().double()[None, :]
        ref = ref + b
        rest = rest + b.abs()
    if res is not None:
        r = res.detach().cpu().double()
        ref = ref + r
        rest = rest + r.abs()
    return ref, mag, rest + ref.abs()


def gemm_bound(mag, rest, c=C_GEMM):
    return c * R.U * mag + 2.0 * R.U * rest


def model_fp32_sequential(a, w, bias=None, res=None, operand='fp16'):
    """The specified arithmetic with ONE fp32 accumulator per output, k ascending: exact products (float64 holds 22 bits), each addition
    rounded to fp32; bias, then the residual, added last in fp32.  operand: 'fp16', or the wrong models 'fp16_trunc' / 'bf16'."""
    rnd = _RND[operand]
    a16, w16 = rnd(a.double()), rnd(w.double())
    acc = torch.zeros((a.shape[0], w.shape[0]), dtype=torch.float32)
    for k in range(a.shape[1]):
        acc = (acc.double() + a16[:, k, None] * w16[None, :, k]).float()
    if bias is not None:
        acc = acc + bias.float()[None, :]
    if res is not None:
        acc = acc + res.float()
    return acc


# ---------------------------------------------------------------- the network-level emulation (CPU)
def emulation_net(sd, cfg, operand, forced_indices=None, decoder_operand=None):
    """oracle/torch_ref.TorchRefNet whose layers under the mode's rule round input (clamped) and weight once to the operand type ('fp16' /
    'bf16'; None = the plain fp32 run) and accumulate in float64:
      * the 1x1 stride-1 layers with Cin % 64 == 0: the Swin qkv / proj / fc1 / fc2, every before_quant;
      * the 3x3 stride-1 pad-1 convs with Cin % 64 == 0 that are not behind every lookup (encoder ResBlock convs, RSTB tail convs).
    Stride-2 convs, in_conv, attention, LayerNorm and the lookup stay fp32.  decoder_operand: additionally round the 3x3 convs BEHIND every
    lookup (out_conv excluded) the same way - decoder_math='fp16' as tests/fp16_ref.py emulates it.
    The net records the first lookup's input rows in .z0 (tokens, e_dim) and its distance matrix in .d0 (tokens, n_e).
    forced_indices (one array per lookup, or one array for the first lookup): _quantize returns those codes instead of the argmin."""
    from oracle.torch_ref import TorchRefNet, _HEADS, _WS
    rnd, drnd = _RND[operand], _RND[decoder_operand]
    cbs = [list(c) for c in cfg['codebook_params']]
    if forced_indices is not None and not isinstance(forced_indices, (list, tuple)):
        forced_indices = [forced_indices]

    class Net(TorchRefNet):
        z0 = d0 = None

        def _behind(self, p):           # model.hip behind_every_lookup
            dec, aq, oc = p.startswith('decoder_group.'), p.startswith('after_quant_group.'), p.startswith('out_conv')
            pre = 'multiscale_encoder.blocks.'
            if len(cbs) == 1:
                return dec or aq or oc or (self.LQ_stage and p.startswith(pre) and int(p[len(pre):].split('.')[0]) > self.encode_depth)
            last_stage = int(np.log2(cbs[-1][0] // cbs[0][0]))
            return oc or (aq and int(p.split('.')[1]) == len(cbs) - 1) or (dec and int(p.split('.')[1]) >= last_stage)

        def _conv(self, x, p, stride=1, pad=1):
            w = self.sd[p + '.weight']
            k, cin, cout = w.shape[-1], w.shape[1], w.shape[0]
            behind = self._behind(p)
            up2 = p.endswith('.block.1') or (p.startswith('multiscale_encoder.blocks.') and p.count('.') == 3 and p.endswith('.1'))
            r = None
            if stride == 1 and k == 1 and pad == 0 and cin % 64 == 0:
                r = rnd                                      # the split GEMM's k1 rule
            elif stride == 1 and k == 3 and pad == 1 and not behind and not up2 and cin % 64 == 0:
                r = rnd                                      # its 3x3 rule, stride 1 only
            elif stride == 1 and k == 3 and pad == 1 and behind and cout > 4 and cin % 32 == 0:
                r = drnd                                     # decoder_math 'fp16' (tests/fp16_ref.py)
            if r is None:
                return super()._conv(x, p, stride, pad)
            y = F.conv2d(r(x.double()), r(w.double()), None, stride=stride, padding=pad)
            return y.float() + self.sd[p + '.bias'][None, :, None, None]

        def _lin(self, t, p):
            w, b = self.sd[p + '.weight'], self.sd[p + '.bias']
            if rnd is None or w.shape[1] % 64:
                return F.linear(t, w, b)
            return F.linear(rnd(t.double()), rnd(w.double())).float() + b

        def _swin_block(self, x, h, w, p, shift):       # TorchRefNet._swin_block with its four linears through _lin
            b, n, c = x.shape
            hd = c // _HEADS
            t = F.layer_norm(x, (c,), self.sd[p + '.norm1.weight'], self.sd[p + '.norm1.bias'], eps=1e-5).reshape(b, h, w, c)
            if shift:
                t = torch.roll(t, shifts=(-shift, -shift), dims=(1, 2))
            win = t.reshape(b, h // _WS, _WS, w // _WS, _WS, c).permute(0, 1, 3, 2, 4, 5).reshape(-1, _WS * _WS, c)
            qkv = self._lin(win, p + '.attn.qkv').reshape(-1, _WS * _WS, 3, _HEADS, hd).permute(2, 0, 3, 1, 4)
            q, k, v = qkv[0] * (hd ** -0.5), qkv[1], qkv[2]
            att = q @ k.transpose(-2, -1)
            bias = self.sd[p + '.attn.relative_position_bias_table'][self._rel_index].reshape(_WS * _WS, _WS * _WS, _HEADS)
            att = att + bias.permute(2, 0, 1).unsqueeze(0)
            if shift:
                m = self._shift_mask(h, w, shift)
                nw = m.shape[0]
                att = (att.reshape(-1, nw, _HEADS, _WS * _WS, _WS * _WS) + m[None, :, None]).reshape(-1, _HEADS, _WS * _WS, _WS * _WS)
            att = torch.softmax(att, dim=-1)
            o = self._lin((att @ v).transpose(1, 2).reshape(-1, _WS * _WS, c), p + '.attn.proj')
            o = o.reshape(b, h // _WS, w // _WS, _WS, _WS, c).permute(0, 1, 3, 2, 4, 5).reshape(b, h, w, c)
            if shift:
                o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
            x = x + o.reshape(b, n, c)
            t = F.layer_norm(x, (c,), self.sd[p + '.norm2.weight'], self.sd[p + '.norm2.bias'], eps=1e-5)
            return x + self._lin(F.gelu(self._lin(t, p + '.mlp.fc1')), p + '.mlp.fc2')

        def _quantize(self, z, qi):
            cb = self.sd[f'quantize_group.{qi}.embedding.weight']
            b, d, h, w = z.shape
            zf = z.permute(0, 2, 3, 1).reshape(-1, d)
            dist = (zf * zf).sum(1, keepdim=True) + (cb * cb).sum(1) - 2.0 * (zf @ cb.t())
            if qi == 0:
                self.z0, self.d0 = zf.clone(), dist
            idx = torch.argmin(dist, dim=1)
            if forced_indices is not None and qi < len(forced_indices) and forced_indices[qi] is not None:
                idx = torch.as_tensor(np.asarray(forced_indices[qi])).reshape(-1).to(torch.int64)
                assert idx.numel() == zf.shape[0], (idx.numel(), zf.shape)
            zq = zf + (cb[idx] - zf)
            return zq.reshape(b, h, w, d).permute(0, 3, 1, 2).contiguous(), idx.reshape(b, 1, h, w)

    return Net(sd, codebook_params=cfg['codebook_params'], LQ_stage=cfg['LQ_stage'], scale_factor=cfg.get('scale_factor', 4))


def run_net(net, cn, x):
    """(image, first index map) as numpy, test() geometry for the LQ nets, forward() for 'hq'."""
    y, idx = net.forward(x) if cn == 'hq' else net.test(x, return_indices=True)
    return y.numpy(), idx.numpy()


# ---------------------------------------------------------------- the near-tie rule
def token_delta(z_emu, z_ref):
    """Delta = 2 max_token |z_emu - z_ref|_2 (float64)."""
    return 2.0 * float((z_emu.double() - z_ref.double()).norm(dim=1).max())


def near_tie_failures(idx_base, idx_mode, d_ref, codebook, delta):
    """Flipped tokens (idx_base != idx_mode) that FAIL the rule; returns (number of flips, [(token, i, j, gap, allowed), ...] of the failures).
    d_ref (tokens, n_e): the reference arithmetic's distances (fp32), codebook (n_e, e_dim)."""
    i_all = np.asarray(idx_base).reshape(-1).astype(np.int64)
    j_all = np.asarray(idx_mode).reshape(-1).astype(np.int64)
    d = np.asarray(d_ref, np.float32)
    cb = np.asarray(codebook, np.float64)
    assert i_all.shape == j_all.shape == (d.shape[0],)
    flips = np.nonzero(i_all != j_all)[0]
    bad = []
    for t in flips:
        i, j = int(i_all[t]), int(j_all[t])
        gap = float(np.float64(d[t, j]) - np.float64(d[t, i]))
        allowed = 2.0 * delta * float(np.linalg.norm(cb[j] - cb[i])) + NEAR_TIE_ULP * float(np.spacing(np.abs(d[t, i])))
        if not gap <= allowed:
            bad.append((int(t), i, j, gap, allowed))
    return len(flips), bad


# ---------------------------------------------------------------- golden cases, computed once per session
_CASES = {}


def golden_case(name):
    """(config name or dict, weights, input, CONFIG dict) of a golden fixture (single- or multi-codebook)."""
    if name not in _CASES:
        from femasr_amd import synth
        from helpers import CONFIGS, cfg_name_of, load_golden, synth_weights
        g = load_golden(name)
        x = synth.synth_input(int(g['input_seed']), tuple(g['in_shape']))
        if 'variant' in g:                  # the multi-codebook fixtures carry their architecture
            from helpers import golden_cfg, weights_from_arch
            cfg = golden_cfg(g)
            _CASES[name] = (None, weights_from_arch(cfg, int(g['seed']), str(g['codebook']), str(g['variant'])), x, cfg)
        else:
            cn = cfg_name_of(g)
            _CASES[name] = (cn, synth_weights(cn, int(g['seed']), str(g['codebook'])), x, CONFIGS[cn])
    return _CASES[name]


_EMU = {}


def emulated(name, operand, forced=None, decoder_operand=None, tag=None):
    """dict(y, idx, z0, d0) of the golden case under the emulation; memoised by (name, operand, decoder_operand, tag) - pass a tag that
    names the forced index map."""
    key = (name, operand, decoder_operand, tag)
    assert (forced is None) == (tag is None)
    if key not in _EMU:
        cn, w, x, cfg = golden_case(name)
        net = emulation_net(w, cfg, operand, forced_indices=forced, decoder_operand=decoder_operand)
        y, idx = run_net(net, cn, x)
        _EMU[key] = dict(y=y, idx=idx, z0=net.z0, d0=net.d0.numpy())
    return _EMU[key]


def codebook0(name):
    return golden_case(name)[1]['quantize_group.0.embedding.weight']

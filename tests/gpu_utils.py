"""Thin wrappers over the C ABI for the GPU parity tests (torch only moves memory)."""
import ctypes

import numpy as np
import torch

from femasr_amd import _lib
import guard_arena as GA


def dev(a, device='cuda'):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def lib_weight_layout(w_khwc):
    """Oracle layout [kh][kw][Cin][Cout] -> the library's packed FRAGMENT-MAJOR layout (numpy restatement of
    femasr_repack_oihw, include/femasr_hip.h): out[q][ntile][lane][kk], zero padded."""
    kh, kw, cin, cout = w_khwc.shape
    if kh == 1 and kw == 1 and cin % 32 == 0:       # GEMM layout of the 1x1 / linear layers: [q][ntile][j][lane][t]
        npad = (cout + 31) // 32 * 32
        full = np.zeros((cin, npad), np.float32)
        full[:, :cout] = w_khwc.reshape(cin, cout)
        # k = 32q + 8j + 4h + t, n = 32*ntile + c:  [q][j][h][t][ntile][c] -> [q][ntile][j][h][c][t]
        t = full.reshape(cin // 32, 4, 2, 4, npad // 32, 32).transpose(0, 4, 1, 2, 5, 3)
        return np.ascontiguousarray(t).reshape(-1)
    if cin % 32 == 0:       # K order: channel blocks of 32 outermost
        rows = w_khwc.reshape(kh, kw, cin // 32, 32, cout).transpose(2, 0, 1, 3, 4).reshape(-1, cout)
    else:
        rows = w_khwc.reshape(-1, cout)
    k = rows.shape[0]
    kp, npad = (k + 31) // 32 * 32, (cout + 31) // 32 * 32
    full = np.zeros((kp, npad), np.float32)
    full[:k, :cout] = rows
    # [q][kk][kslot][ntile][col] -> [q][ntile][kslot][col][kk]
    t = full.reshape(kp // 32, 16, 2, npad // 32, 32).transpose(0, 3, 2, 4, 1)
    out = np.ascontiguousarray(t).reshape(-1)
    if cout <= 4 and kh == 3 and kw == 3 and cin % 32 == 0:       # compact [k][4] copy for the direct (VALU) out_conv kernel
        tail = np.zeros((k, 4), np.float32)
        tail[:, :cout] = rows
        out = np.concatenate((out, tail.reshape(-1)))
    return out


def q(name, *args):
    """A size query of the library that returns its value (femasr_*_bytes / _floats / _partials / _entries), noted in guard_arena.QUERIED."""
    GA.QUERIED.add(name)
    return int(getattr(_lib.load(), name)(*args))


def qp(name, *args):
    """A size query that returns through a trailing size_t* (the femasr_*workspace_bytes family)."""
    GA.QUERIED.add(name)
    n = ctypes.c_size_t(0)
    _lib.check(getattr(_lib.load(), name)(*args, ctypes.byref(n)))
    return int(n.value)


class Operands:
    """The operands of one call (or of a repack -> call chain) as regions of one guard arena (tests/guard_arena.py), each at its
    exact size.  add() in call order, then build(); p(name) is the region's device pointer (None for an operand left out)."""

    def __init__(self, what, device='cuda'):
        self.what, self.device, self.specs, self.r, self.arena = what, device, [], {}, None

    def inp(self, name, data):
        if data is not None:
            data = data if isinstance(data, torch.Tensor) else np.ascontiguousarray(data)
            self.specs.append((name, 'in', GA._bytes(data).numel(), data, None))
        return self

    def out(self, name, nbytes, kind='out', compared=None):
        self.specs.append((name, kind, int(nbytes), None, compared))
        return self

    def scratch(self, name, nbytes):
        return self.out(name, nbytes, 'scratch')

    def build(self):
        self.arena = GA.new_arena([sp[2] for sp in self.specs], self.device)
        for name, kind, n, data, compared in self.specs:
            self.r[name] = self.arena.add(name, kind, n, data, compared)
        self.arena.arm()
        return self

    def p(self, name):
        return ctypes.c_void_p(self.r[name].ptr) if name in self.r else None

    def addr(self, name):
        return self.r[name].ptr if name in self.r else None

    def check(self, step=''):
        self.arena.check(f'{self.what}{" " + step if step else ""}')

    def packed(self, name, rc):
        """After a repack call: check the guards, then the image is an input of what follows."""
        _lib.check(rc)
        self.check(name)
        self.arena.freeze(self.r[name])

    def get(self, name, dtype, shape=(-1,)):
        """Copy of a region's contents (a tensor of its own on the arena's device)."""
        return self.r[name].as_(dtype, shape).clone()


def conv_form_of(ksz, bf16x3=False, wino=False, up2=False, bf16s=False, f16=False):
    if bf16s:
        return 'split3x3' if ksz == 3 else 'split1x1'
    return 'bf16x3' if bf16x3 else 'f16' if f16 else ('wino_up2' if up2 else 'wino4') if wino else 'direct'


def conv2d(x, w_khwc, bias, ksz, stride=1, pad=0, up2=False, prologue=0, pro=(None, None, None), act=0,
           res1=None, res2=None, bf16x3=False, gn_part=False, wino=False, fast_act=False, in_add=None, bf16s=False, f16=False):
    """x NHWC numpy -> numpy, through femasr_conv2d (weights given in the oracle's [kh][kw][Cin][Cout] layout).
    bf16s: the 1x1 / Linear layer on the bf16 matrix pipe (femasr_conv_args.w_bf16s, three-term split).
    f16: the one-pass fp16 forms (femasr_conv_args.w_f16: 3x3 halo form, or the k1 GEMM with ksz = 1).
    Every operand - input, each weight image, bias, prologue coefficients, residuals, in_add, out, gn_part - is a region of one
    guard arena at the size the library's own queries give; each repack and the conv are checked for stray stores."""
    lib = _lib.load()
    w_khwc = np.asarray(w_khwc)
    cout = w_khwc.shape[-1]
    b, h, w, cin = x.shape
    w_oihw = np.ascontiguousarray(w_khwc.transpose(3, 2, 0, 1))
    hv, wv = (2 * h, 2 * w) if up2 else (h, w)
    ho, wo = (hv + 2 * pad - ksz) // stride + 1, (wv + 2 * pad - ksz) // stride + 1
    ops = Operands(f'conv2d B{b} {h}x{w} {cin}->{cout} k{ksz}s{stride}p{pad}{" up2" if up2 else ""}')
    ops.inp('x', x)
    ops.inp('w', lib_weight_layout(w_khwc))
    assert ops.specs[-1][2] == 4 * q('femasr_packed_weight_floats', cout, cin, ksz, ksz), 'packed image and femasr_packed_weight_floats differ'
    ops.inp('bias', bias)
    for name, t in zip(('pro_a', 'pro_b', 'pro_c', 'res1', 'res2', 'in_add'), tuple(pro) + (res1, res2, in_add)):
        ops.inp(name, t)
    repacks = []        # (region, call)
    need_oihw = False
    if bf16s and ksz == 3:       # the 3x3 conv as the split-bf16 GEMM over K = 9 Cin: planes packed on the GPU from OIHW
        ops.out('w_bf16s', q('femasr_packed_weight_conv3x3_bf16s_bytes', cout, cin))
        repacks.append(('w_bf16s', lambda: lib.femasr_repack_oihw_bf16s(None, ops.p('w_oihw'), cout, cin, ops.p('w_bf16s'))))
    elif bf16s:
        ops.out('w_bf16s', q('femasr_packed_weight_bf16s_bytes', cout, cin))
        repacks.append(('w_bf16s', lambda: lib.femasr_repack_k1_bf16s(None, ops.p('w_oihw'), cout, cin, ops.p('w_bf16s'))))
    if bf16x3:      # opt-in split-bf16 path: weights repacked on the GPU from OIHW
        ops.out('w_bf16x3', q('femasr_packed_weight_bf16x3_bytes', cout, cin, ksz, ksz))
        repacks.append(('w_bf16x3', lambda: lib.femasr_repack_oihw_bf16x3(None, ops.p('w_oihw'), cout, cin, ksz, ksz, ops.p('w_bf16x3'))))
    if f16 and ksz == 1:
        ops.out('w_f16', q('femasr_packed_weight_k1_f16_bytes', cout, cin))
        repacks.append(('w_f16', lambda: lib.femasr_repack_k1_f16(None, ops.p('w_oihw'), cout, cin, ops.p('w_f16'))))
    elif f16:
        ops.out('w_f16', q('femasr_packed_weight_f16_bytes', cout, cin, ksz, ksz))
        repacks.append(('w_f16', lambda: lib.femasr_repack_oihw_f16(None, ops.p('w_oihw'), cout, cin, ksz, ksz, ops.p('w_f16'))))
    if up2 and ksz == 3 and stride == 1 and pad == 1 and cin % 32 == 0 and not (bf16x3 or f16):    # phase-filter form of nearest-x2 + conv
        ops.out('w_up2', 4 * q('femasr_up2_weight_floats', cout, cin))
        repacks.append(('w_up2', lambda: lib.femasr_repack_oihw_up2(None, ops.p('w_oihw'), cout, cin, ops.p('w_up2'))))
    if wino and up2:     # the 25-component form of nearest-x2 + conv (kernels_wino_up2.hip)
        ops.out('w_wino', 4 * q('femasr_wino_up2_weight_floats', cout, cin))
        repacks.append(('w_wino', lambda: lib.femasr_repack_oihw_wino_up2(None, ops.p('w_oihw'), cout, cin, ops.p('w_wino'))))
    elif wino:           # Winograd-domain weights, transformed and packed on the GPU from OIHW
        ops.out('w_wino', 4 * q('femasr_wino_weight_floats', cout, cin))
        repacks.append(('w_wino', lambda: lib.femasr_repack_oihw_wino(None, ops.p('w_oihw'), cout, cin, ops.p('w_wino'))))
    if repacks:
        ops.inp('w_oihw', w_oihw)
    ops.out('out', 4 * b * ho * wo * cout)
    a = _lib.ConvArgs()
    a.B, a.H, a.W, a.Cin = b, h, w, cin
    a.Cout, a.ksz, a.stride, a.pad, a.up2, a.prologue = cout, ksz, stride, pad, int(up2), prologue
    a.act = act
    a.Ho, a.Wo = ho, wo
    a.fast_act = int(fast_act)      # 0 exact, 1 hardware SiLU
    tiles = 0
    if gn_part:
        import anchor_cases as AC
        form = conv_form_of(ksz, bf16x3, wino, up2, bf16s, f16)
        tiles = AC._gn_tiles('bf16x3' if form == 'f16' else form, a)       # (the fp16 halo form shares the bf16x3 form's tile rule)
        if tiles == 0:              # outside every form's rule: the library refuses the call; size as the plain halo form would
            tiles = ((ho + 7) // 8) * ((wo + 15) // 16)
        ops.out('gn_part', 8 * b * tiles * 32 * 2)
    ops.build()
    for name, call in repacks:
        ops.packed(name, call())
    a.in_ = ops.addr('x'); a.w = ops.addr('w'); a.bias = ops.addr('bias')
    a.pro_a, a.pro_b, a.pro_c = ops.addr('pro_a'), ops.addr('pro_b'), ops.addr('pro_c')
    a.res1, a.res2, a.in_add = ops.addr('res1'), ops.addr('res2'), ops.addr('in_add')
    a.out = ops.addr('out')
    a.w_bf16x3, a.w_up2, a.w_wino = ops.addr('w_bf16x3'), ops.addr('w_up2'), ops.addr('w_wino')
    a.w_bf16s, a.w_f16, a.gn_part = ops.addr('w_bf16s'), ops.addr('w_f16'), ops.addr('gn_part')
    _lib.check(lib.femasr_conv2d(None, ctypes.byref(a)))
    ops.check('femasr_conv2d')
    out = ops.get('out', torch.float32, (b, ho, wo, cout)).cpu().numpy()
    if gn_part:
        return out, ops.get('gn_part', torch.float64, (b, tiles, 32, 2))
    return out


def conv_variant_name(x_shape, cout, ksz, stride=1, pad=0, up2=False, prologue=0, act=0, nres=0, bf16x3=False, wino=False,
                      fast_act=False, in_add=False, bf16s=False, f16=False):
    """Instantiation name of the launch conv2d() makes with these arguments (femasr_debug_conv_variant_name: reads no pointer)."""
    b, h, w, cin = x_shape
    a = _lib.ConvArgs()
    a.B, a.H, a.W, a.Cin = b, h, w, cin
    a.Cout, a.ksz, a.stride, a.pad, a.up2, a.prologue, a.act = cout, ksz, stride, pad, int(up2), prologue, act
    hv, wv = (2 * h, 2 * w) if up2 else (h, w)
    a.Ho, a.Wo = (hv + 2 * pad - ksz) // stride + 1, (wv + 2 * pad - ksz) // stride + 1
    a.fast_act = int(fast_act)
    a.w = 1
    a.res1 = 1 if nres >= 1 else None
    a.res2 = 1 if nres >= 2 else None
    a.in_add = 1 if in_add else None
    a.w_bf16x3 = 1 if bf16x3 else None
    a.w_bf16s = 1 if bf16s else None
    a.w_f16 = 1 if f16 else None
    a.w_wino = 1 if wino else None
    a.w_up2 = 1 if (up2 and ksz == 3 and stride == 1 and pad == 1 and cin % 32 == 0 and not (bf16x3 or f16)) else None
    buf = ctypes.create_string_buffer(256)
    _lib.check(_lib.load().femasr_debug_conv_variant_name(ctypes.byref(a), buf, len(buf)))
    return buf.value.decode()


def gn_silu_apply(x, a, b):
    """silu(fmaf(x, a[n][c], b[n][c])) on an NHWC array through femasr_gn_silu_apply."""
    lib = _lib.load()
    bb, h, w, c = x.shape
    ops = Operands(f'gn_silu_apply {x.shape}').inp('x', x).inp('a', a).inp('b', b).out('y', 4 * x.size).build()
    _lib.check(lib.femasr_gn_silu_apply(None, ops.p('x'), bb, h, w, c, ops.p('a'), ops.p('b'), ops.p('y')))
    ops.check()
    return ops.get('y', torch.float32, x.shape).cpu().numpy()


MATH_FN = {'exp': 0, 'erf': 1, 'silu': 2, 'gelu': 3, 'exp2': 4, 'erf2': 5, 'silu2': 6, 'gelu2': 7, 'fast_silu': 8}


def math_eval(fn, x):
    """The device's own elementary functions through femasr_debug_math_eval (fn: a key of MATH_FN; the '2' forms take the pairs
    (x[2i], x[2i+1]))."""
    x = np.ascontiguousarray(x, np.float32)
    ops = Operands(f'debug_math_eval {fn} n {x.size}').inp('x', x).out('y', 4 * x.size).build()
    _lib.check(_lib.load().femasr_debug_math_eval(None, MATH_FN[fn], ops.p('x'), x.size, ops.p('y')))
    ops.check()
    return ops.get('y', torch.float32, x.shape).cpu().numpy()


def gn_coeffs(x, gamma, beta, eps=1e-6, groups=32):
    lib = _lib.load()
    b, h, w, c = x.shape
    ops = Operands(f'gn_coeffs {x.shape}').inp('x', x).inp('gamma', gamma).inp('beta', beta).out('a', 4 * b * c).out('b', 4 * b * c)
    ops.scratch('scratch', q('femasr_gn_scratch_bytes', b, h, w, c, groups)).build()
    _lib.check(lib.femasr_gn_coeffs(None, ops.p('x'), b, h, w, c, groups, ops.p('gamma'), ops.p('beta'), eps,
                                    ops.p('a'), ops.p('b'), ops.p('scratch')))
    ops.check()
    return ops.get('a', torch.float32, (b, c)).cpu().numpy(), ops.get('b', torch.float32, (b, c)).cpu().numpy()


def gn_coeffs_from_partials(part, h, w, c, gamma, beta, eps=1e-6):
    lib = _lib.load()
    b, tiles = part.shape[0], part.shape[1]
    ops = Operands(f'gn_coeffs_from_partials B{b} tiles {tiles} {h}x{w}x{c}').inp('part', part).inp('gamma', gamma).inp('beta', beta)
    ops.out('a', 4 * b * c).out('b', 4 * b * c).build()
    _lib.check(lib.femasr_gn_coeffs_from_partials(None, ops.p('part'), b, tiles, h, w, c, 32, ops.p('gamma'), ops.p('beta'), eps,
                                                  ops.p('a'), ops.p('b')))
    ops.check()
    return ops.get('a', torch.float32, (b, c)).cpu().numpy(), ops.get('b', torch.float32, (b, c)).cpu().numpy()


def ln_stats(x, eps=1e-5):
    lib = _lib.load()
    rows, c = x.shape
    ops = Operands(f'ln_stats {x.shape}').inp('x', x).out('stats', 4 * rows * 2).build()
    _lib.check(lib.femasr_ln_stats(None, ops.p('x'), rows, c, eps, ops.p('stats')))
    ops.check()
    return ops.get('stats', torch.float32, (rows, 2)).cpu().numpy()


def layernorm(x, gamma, beta, eps=1e-5):
    lib = _lib.load()
    rows, c = x.shape
    ops = Operands(f'layernorm {x.shape}').inp('x', x).inp('gamma', gamma).inp('beta', beta).out('y', 4 * rows * c).build()
    _lib.check(lib.femasr_layernorm(None, ops.p('x'), rows, c, ops.p('gamma'), ops.p('beta'), eps, ops.p('y')))
    ops.check()
    return ops.get('y', torch.float32, (rows, c)).cpu().numpy()


def window_attention(qkv, b, h, w, c, heads, shift, table):
    lib = _lib.load()
    ops = Operands(f'window_attention B{b} {h}x{w}x{c} shift {shift}').inp('qkv', qkv).inp('table', table).out('out', 4 * b * h * w * c).build()
    _lib.check(lib.femasr_window_attention(None, ops.p('qkv'), b, h, w, c, heads, shift, ops.p('table'), ops.p('out')))
    ops.check()
    return ops.get('out', torch.float32, (b, h * w, c)).cpu().numpy()


def _vq_prepare(ops, n_e, d, packed=True, aux=False):
    """The codebook's derived images, each written into an exact-size region and checked: cbT (femasr_repack_oihw), ee
    (femasr_row_sqsum) and, for the two-pass search, aux (femasr_vq_prepare)."""
    lib = _lib.load()
    if packed:
        ops.packed('cbT', lib.femasr_repack_oihw(None, ops.p('cb'), n_e, d, 1, 1, ops.p('cbT')))
    ops.packed('ee', lib.femasr_row_sqsum(None, ops.p('cb'), n_e, d, ops.p('ee')))
    if aux:
        ops.packed('aux', lib.femasr_vq_prepare(None, ops.p('cb'), ops.p('ee'), n_e, d, ops.p('aux')))


def vq(z_rows, codebook, mode='gemm'):
    """mode 'gemm': femasr_vq (single pass, fp32 MFMA); 'twopass': femasr_vq_twopass (bf16 candidates + exact re-check)."""
    lib = _lib.load()
    m, d = z_rows.shape
    n_e = codebook.shape[0]
    ops = Operands(f'vq {mode} M {m} D {d} n_e {n_e}').inp('z', z_rows).inp('cb', codebook)
    ops.out('cbT', 4 * q('femasr_packed_weight_floats', n_e, d, 1, 1)).out('ee', 4 * n_e)
    if mode != 'gemm':
        assert lib.femasr_vq_twopass_ok(n_e, d)
        ops.out('aux', q('femasr_vq_aux_bytes', n_e, d))
    ops.out('idx', 8 * m).out('zq', 4 * m * d).scratch('scratch', q('femasr_vq_scratch_bytes', m, n_e)).build()
    _vq_prepare(ops, n_e, d, aux=mode != 'gemm')
    if mode == 'gemm':
        _lib.check(lib.femasr_vq(None, ops.p('z'), m, d, ops.p('cb'), ops.p('cbT'), ops.p('ee'), n_e,
                                 ops.p('idx'), ops.p('zq'), ops.p('scratch')))
    else:
        _lib.check(lib.femasr_vq_twopass(None, ops.p('z'), m, d, ops.p('cb'), ops.p('aux'), ops.p('ee'), n_e,
                                         ops.p('idx'), ops.p('zq'), ops.p('scratch')))
    ops.check()
    return (ops.get('idx', torch.int64).cpu().numpy(), ops.get('zq', torch.float32, (m, d)).cpu().numpy(),
            ops.get('cbT', torch.float32).cpu().numpy(), ops.get('ee', torch.float32).cpu().numpy())


def vq_candidates(z_rows, codebook):
    """Pass 1 of the two-pass search: (cand (M,32) uint16, cnt (M,) uint16; 0xFFFF = every code)."""
    lib = _lib.load()
    m, d = z_rows.shape
    n_e = codebook.shape[0]
    ops = Operands(f'vq_candidates M {m} D {d} n_e {n_e}').inp('z', z_rows).inp('cb', codebook)
    ops.out('ee', 4 * n_e).out('aux', q('femasr_vq_aux_bytes', n_e, d))
    # (which codes besides the first-min a list holds depends on the order in which concurrent waves tighten the row's threshold -
    # include/femasr_hip.h -: guarded, but not required to be the same bits in two runs)
    ops.out('cand', 2 * m * 32, compared=False).out('cnt', 2 * m, compared=False).build()
    _vq_prepare(ops, n_e, d, packed=False, aux=True)
    _lib.check(lib.femasr_vq_candidates(None, ops.p('z'), m, d, ops.p('aux'), ops.p('ee'), n_e, ops.p('cand'), ops.p('cnt')))
    ops.check()
    return ops.get('cand', torch.int16, (m, 32)).cpu().numpy().view('uint16'), ops.get('cnt', torch.int16).cpu().numpy().view('uint16')


def build_net(cfg_name, weights, device='cuda', decoder_math='fp32_strict', linear_math='bf16_split'):
    """decoder_math defaults to 'fp32_strict' HERE (the tests' bit-exact comparisons with the oracle): the product default
    'fp32' runs the SiLU of the Winograd convs on the hardware exp2 / rcp units and is compared with a tolerance instead
    (test_gpu_network.py::test_default_mode_vs_oracle_and_reference)."""
    from femasr_amd.archs import build_network
    from helpers import CONFIGS
    net = build_network(dict(type='FeMaSRNet', **CONFIGS[cfg_name]))
    missing = net.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()}, strict=False)
    assert not missing.unexpected_keys
    net.decoder_math = decoder_math
    net.linear_math = linear_math
    return net.to(device).eval()

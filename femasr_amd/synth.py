"""Deterministic synthetic weights / inputs.

The reference ships no weights (`.gitignore:20`, downloaded at run time in
inference_femasr.py:13-16,33-34) and there is no network here, so goldens and
benchmarks use a counter-based generator that is a pure function of
``(seed, state-dict key, element index)``.  It uses only integer numpy ops and
one float64 affine map, so the same bits come out in the development container
(where the reference is imported to make the goldens) and on the GPU box.
"""
import numpy as np

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _fnv1a64(text: str) -> int:
    h = 0xCBF29CE484222325
    for ch in text.encode('utf-8'):
        h ^= ch
        h = (h * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def _splitmix64(x: np.ndarray) -> np.ndarray:
    with np.errstate(over='ignore'):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def uniform01(seed: int, key: str, n: int) -> np.ndarray:
    """n float64 values in [0,1) with 24 significant bits (exact in fp32)."""
    base = np.uint64((_fnv1a64(key) ^ (seed * 0x9E3779B97F4A7C15)) & 0xFFFFFFFFFFFFFFFF)
    with np.errstate(over='ignore'):
        ctr = base + np.arange(n, dtype=np.uint64) * np.uint64(0xD1342543DE82EF95)
    bits = _splitmix64(ctr) >> np.uint64(40)
    return bits.astype(np.float64) * (1.0 / (1 << 24))


def uniform(seed: int, key: str, shape, lo: float, hi: float) -> np.ndarray:
    n = int(np.prod(shape)) if len(shape) else 1
    u = uniform01(seed, key, n)
    return (lo + (hi - lo) * u).astype(np.float32).reshape(shape)


def synth_tensor(seed: int, key: str, shape, codebook: str = 'init', out_conv_scale: float = 1.0 / 16.0) -> np.ndarray:
    """Value rule per state-dict key.  Chosen so activations stay O(1) through
    the network (variance-preserving conv/linear weights, GN/LN affine near
    identity) — the regime the parity tolerances are stated for.  `out_conv_scale`
    = 1 gives the un-scaled variant (output magnitudes ~16x larger)."""
    shape = tuple(int(s) for s in shape)
    leaf = key.rsplit('.', 1)[-1]
    if key.endswith('embedding.weight'):
        if codebook == 'init':          # reference init: U(+-1/n_e), femasr_arch.py:33
            b = 1.0 / shape[0]
        elif codebook == 'trained':     # codes at the scale of z
            b = 1.0
        else:
            raise ValueError(codebook)
        return uniform(seed, key, shape, -b, b)
    if leaf == 'relative_position_bias_table':
        return uniform(seed, key, shape, -0.2, 0.2)
    if leaf == 'weight' and len(shape) == 1:        # GroupNorm / LayerNorm gamma
        return uniform(seed, key, shape, 0.8, 1.2)
    if leaf == 'bias':
        return uniform(seed, key, shape, -0.1, 0.1)
    if leaf == 'weight' and len(shape) >= 2:        # conv OIHW / linear (out,in)
        fan_in = int(np.prod(shape[1:]))
        b = float(np.sqrt(3.0 / fan_in))
        if key == 'out_conv.weight':    # keep the synthetic image O(1), the regime the 1e-3 bound is stated for
            b *= out_conv_scale
        return uniform(seed, key, shape, -b, b)
    raise KeyError(f'no synthetic rule for {key} {shape}')


def torch_default_tensor(seed: int, key: str, shape, shapes) -> np.ndarray:
    """The distributions torch's default initialisers give each tensor of the architecture (nn.Conv2d / nn.Linear:
    kaiming_uniform(a=sqrt 5) weights and U(+-1/sqrt(fan_in)) biases; GroupNorm / LayerNorm identity affine; Swin
    relative-position tables trunc_normal(std .02), network_swinir.py; codebook U(+-1/n_e), femasr_arch.py:33), drawn from
    a torch CPU generator keyed by (seed, state-dict key) so that both sides regenerate the same values with the same
    torch build.  `shapes` = {key: shape} of the whole state dict (a bias needs its weight's fan-in)."""
    import torch
    shape = tuple(int(s) for s in shape)
    g = torch.Generator().manual_seed((_fnv1a64(key) ^ (seed * 0x9E3779B97F4A7C15)) & 0x7FFFFFFFFFFFFFFF)
    leaf = key.rsplit('.', 1)[-1]
    if key.endswith('embedding.weight'):
        return torch.empty(shape).uniform_(-1.0 / shape[0], 1.0 / shape[0], generator=g).numpy()
    if leaf == 'relative_position_bias_table':
        return torch.nn.init.trunc_normal_(torch.empty(shape), std=.02, generator=g).numpy()
    if len(shape) == 1:
        wkey = key.rsplit('.', 1)[0] + '.weight'
        wshape = shapes.get(wkey, ())
        if leaf == 'weight' or len(wshape) < 2:        # norm layers: weight 1, bias 0
            return (np.ones if leaf == 'weight' else np.zeros)(shape, np.float32)
        b = 1.0 / float(np.sqrt(int(np.prod(wshape[1:]))))
        return torch.empty(shape).uniform_(-b, b, generator=g).numpy()
    b = 1.0 / float(np.sqrt(int(np.prod(shape[1:]))))
    return torch.empty(shape).uniform_(-b, b, generator=g).numpy()


def fill_state_dict(state_dict, seed: int = 0, codebook: str = 'init', variant: str = 'default'):
    """Return {key: np.ndarray} for every floating tensor of a state dict
    (integer / mask buffers such as relative_position_index and attn_mask keep
    their constructed values and are skipped).
    variant: 'default' (synth_tensor), 'unscaled' (out_conv not scaled down), 'torchinit' (torch_default_tensor)."""
    out = {}
    shapes = {k: tuple(v.shape) for k, v in state_dict.items()}
    for key, val in state_dict.items():
        leaf = key.rsplit('.', 1)[-1]
        if leaf in ('relative_position_index', 'attn_mask'):
            continue
        if variant == 'torchinit':
            out[key] = torch_default_tensor(seed, key, tuple(val.shape), shapes)
        else:
            out[key] = synth_tensor(seed, key, tuple(val.shape), codebook, 1.0 if variant == 'unscaled' else 1.0 / 16.0)
    return out


def synth_input(seed: int, shape, tag: str = 'input') -> np.ndarray:
    """Image-like input in [0,1): smooth low-frequency content + noise, NCHW fp32."""
    b, c, h, w = shape
    noise = uniform(seed, f'{tag}.noise', shape, 0.0, 1.0)
    yy = np.arange(h, dtype=np.float64)[:, None] / max(h, 1)
    xx = np.arange(w, dtype=np.float64)[None, :] / max(w, 1)
    ph = uniform(seed, f'{tag}.phase', (b, c, 4), 0.0, 6.283185307179586).astype(np.float64)
    base = np.empty(shape, dtype=np.float64)
    for n in range(b):
        for ch in range(c):
            p = ph[n, ch]
            base[n, ch] = 0.5 + 0.2 * np.sin(6.0 * yy + p[0]) * np.cos(5.0 * xx + p[1]) \
                + 0.1 * np.sin(17.0 * (yy + xx) + p[2])
    img = 0.7 * base + 0.3 * noise
    return np.clip(img, 0.0, 0.999).astype(np.float32)


def lpips_state(shapes, seed: int = 0):
    """Synthetic LPIPS weights for {canonical key: shape} (femasr_amd.lpips.expected_shapes): He-scaled conv weights (uniform with
    variance 2 / fan_in), small positive biases (no tap's features die), non-negative heads in [0, 1) / C_k as the trained heads are."""
    out = {}
    for key, shape in shapes.items():
        if key.startswith('lin'):
            out[key] = (uniform(seed, key, shape, 0.0, 1.0) / shape[1]).astype(np.float32)
        elif key.endswith('.bias'):
            out[key] = uniform(seed, key, shape, 0.01, 0.1)
        else:
            lim = float(np.sqrt(6.0 / (shape[1] * shape[2] * shape[3])))
            out[key] = uniform(seed, key, shape, -lim, lim)
    return out


def dists_state(seed: int = 0, shapes=None):
    """Synthetic DISTS weights for {canonical key: shape} (default: femasr_amd.dists.expected_shapes()): convs N(0, 2 / (9 Cin)), biases
    0.05 N(0, 1), alpha and beta |0.1 + 0.01 N(0, 1)| (positive, as the trained vectors are).  With these the stage outputs stay O(1)
    through all five stages.  Drawn from numpy's PCG64 keyed by (seed, key)."""
    if shapes is None:
        from .dists import expected_shapes
        shapes = expected_shapes()
    out = {}
    for key, shape in shapes.items():
        n = np.random.default_rng([int(seed), _fnv1a64(key) & 0xFFFFFFFF]).standard_normal(tuple(shape))
        if key in ('alpha', 'beta'):
            out[key] = np.abs(0.1 + 0.01 * n).astype(np.float32)
        elif key.endswith('.bias'):
            out[key] = (0.05 * n).astype(np.float32)
        else:
            out[key] = (n * np.sqrt(2.0 / (9.0 * shape[1]))).astype(np.float32)
    return out

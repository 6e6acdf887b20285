"""fp64 restatement of LPIPS v0.1 (inference) in torch.nn.functional, written from the definition alone (not from femasr_amd.lpips):
input scaling, AlexNet / VGG16 `features` with ReLU after every conv, the five taps, the normalise / squared-difference / linear head,
the spatial mean and the sum over taps."""
import numpy as np
import torch
import torch.nn.functional as F

SHIFT = np.float32([-.030, -.088, -.188])
SCALE = np.float32([.458, .448, .450])

# ('conv', torchvision feature index, stride, pad) / ('tap',) / ('pool', kernel)
ALEX = [('conv', 0, 4, 2), ('tap',), ('pool', 3), ('conv', 3, 1, 2), ('tap',), ('pool', 3), ('conv', 6, 1, 1), ('tap',),
        ('conv', 8, 1, 1), ('tap',), ('conv', 10, 1, 1), ('tap',)]
VGG = [('conv', 0, 1, 1), ('conv', 2, 1, 1), ('tap',), ('pool', 2), ('conv', 5, 1, 1), ('conv', 7, 1, 1), ('tap',), ('pool', 2),
       ('conv', 10, 1, 1), ('conv', 12, 1, 1), ('conv', 14, 1, 1), ('tap',), ('pool', 2),
       ('conv', 17, 1, 1), ('conv', 19, 1, 1), ('conv', 21, 1, 1), ('tap',), ('pool', 2),
       ('conv', 24, 1, 1), ('conv', 26, 1, 1), ('conv', 28, 1, 1), ('tap',)]
SLICE_BOUNDS = {'alex': (2, 5, 8, 10, 12), 'vgg': (4, 9, 16, 23, 30)}     # lpips: sliceK = features[prev bound : bound]


def _key(net, idx, what):
    k = next(i + 1 for i, b in enumerate(SLICE_BOUNDS[net]) if idx < b)
    return f'net.slice{k}.{idx}.{what}'


def scale_input(x):
    """x (B,3,H,W) float32 in [0,1] -> fp32 scaled input, the operations in the definition's order."""
    x = torch.as_tensor(np.asarray(x, np.float32))
    t = 2 * x - 1
    return (t - torch.from_numpy(SHIFT).view(1, 3, 1, 1)) / torch.from_numpy(SCALE).view(1, 3, 1, 1)


def _t(v, dtype):
    return (v if torch.is_tensor(v) else torch.from_numpy(np.asarray(v))).to(dtype)


def features(state, net, x, dtype=torch.float64):
    """The five taps of the backbone on the scaled input x (B,3,H,W)."""
    h = torch.as_tensor(x).to(dtype)
    taps = []
    for op in (ALEX if net == 'alex' else VGG):
        if op[0] == 'conv':
            w, b = _t(state[_key(net, op[1], 'weight')], dtype), _t(state[_key(net, op[1], 'bias')], dtype)
            h = F.relu(F.conv2d(h, w, b, stride=op[2], padding=op[3]))
        elif op[0] == 'tap':
            taps.append(h)
        else:
            h = F.max_pool2d(h, op[1], 2)
    return taps


def head(f0, f1, w_lin):
    """Spatial mean of lin((n0 - n1)^2), n = f / (|f| + 1e-10) over channels; f0, f1 (B,C,H,W) -> (B,) in the inputs' dtype."""
    f0, f1 = torch.as_tensor(f0), torch.as_tensor(f1)
    n0 = f0 / (torch.sqrt((f0 ** 2).sum(1, keepdim=True)) + 1e-10)
    n1 = f1 / (torch.sqrt((f1 ** 2).sum(1, keepdim=True)) + 1e-10)
    d = (n0 - n1) ** 2
    w = torch.as_tensor(np.asarray(w_lin)).to(f0.dtype).reshape(1, -1, 1, 1)
    return (d * w).sum(1).mean((1, 2))


def lpips(state, net, x0, x1):
    """(total (B,), terms (B,5)) in fp64 for x0, x1 (B,3,H,W) in [0,1]."""
    t0, t1 = features(state, net, scale_input(x0)), features(state, net, scale_input(x1))
    terms = torch.stack([head(a, b, state[f'lin{k}.model.1.weight']) for k, (a, b) in enumerate(zip(t0, t1))], 1)
    return terms.sum(1).numpy(), terms.numpy()

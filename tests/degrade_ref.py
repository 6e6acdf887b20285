"""float32 restatements of the kernels of csrc/degrade.hip (femasr_amd/degrade.py): the same sums in the same order with every
multiply and every add rounded to float32 on its own (numpy rounds each array operation; the library is built with -ffp-contract=off), so
that the kernels can be compared with them BIT FOR BIT.  The bounds that hold them to the float64 definitions are derived here too.

blur_bound.  The restatement is a recursive float32 sum of n = k^2 products (u = 2^-24 the unit roundoff): term i passes through one rounding
  of its product and at most n roundings of the accumulator, so |f32 - exact| <= ((1 + u)^(n + 1) - 1) sum_i |w_i x_i| (the standard bound of
  recursive summation).  The weights are non-negative and sum to 1, |x| <= X: sum_i |w_i x_i| <= X, and the bound is (k^2 + 1) u X at first
  order: blur_bound = (k^2 + 1) u X.  (The second-order terms are below k^4 u^2 X / 2 < 0.012 u X at k = 25; the float64 accumulation the
  restatement is compared with is within k^2 2^-53 X of the exact sum.)
resize_bound.  Per pass with taps weights w (float32, any sign) and inputs bounded by X: products sum_i |w_i| u X = S u X with S = sum |w_i|
  (1 for bilinear and area, at most about 1.6 for the cubics' negative lobes); every partial sum is bounded by S X, so `taps` adds contribute
  taps S u X.  One pass: (taps + 1) S u X.  The W pass sees inputs bounded by S_h X and carries the H pass's error through weights of
  absolute sum S_w:  total <= S_w (taps_h + 1) S_h u X + (taps_w + 1) S_w S_h u X = S_h S_w (taps_h + taps_w + 2) u X, + 1 u S_h S_w X for
  the definition's own rounding; resize_bound adds one more for second-order terms."""
import numpy as np

from femasr_amd import degrade as D

U = 2.0 ** -24


def blur_f32(img, kernel, stride=1):
    """degrade_blur_kernel: one float32 accumulator per channel from 0, i ascending outside, j inside."""
    img = np.asarray(img, np.float32)
    kernel = D.check_kernel(kernel)
    k = kernel.shape[0]
    r = k // 2
    ys, xs = np.arange(0, img.shape[0], stride), np.arange(0, img.shape[1], stride)
    acc = np.zeros((len(ys), len(xs), 3), np.float32)
    for i in range(k):
        rows = img[D.mirror_index(ys + r - i, img.shape[0])]
        for j in range(k):
            acc = acc + kernel[i, j] * rows[:, D.mirror_index(xs + r - j, img.shape[1])]
    assert acc.dtype == np.float32
    return acc


def blur_bound(k, xmax):
    return (k * k + 1) * U * xmax


def resize_f32(img, tables_h, tables_w):
    """degrade_resize_kernel: H pass, W pass, float32 accumulators from 0 over the taps in ascending order; clip."""
    img = np.asarray(img, np.float32)
    (wh, ih), (ww, iw) = tables_h, tables_w
    out1 = np.zeros((wh.shape[0],) + img.shape[1:], np.float32)
    for k in range(wh.shape[1]):
        out1 = out1 + wh[:, k][:, None, None] * img[ih[:, k]]
    out2 = np.zeros((wh.shape[0], ww.shape[0], 3), np.float32)
    for k in range(ww.shape[1]):
        out2 = out2 + ww[:, k][None, :, None] * out1[:, iw[:, k]]
    assert out2.dtype == np.float32
    return np.clip(out2, np.float32(0), np.float32(1))


def resize_bound(tables_h, tables_w, xmax):
    sh = float(np.abs(tables_h[0].astype(np.float64)).sum(1).max())
    sw = float(np.abs(tables_w[0].astype(np.float64)).sum(1).max())
    return sh * sw * (tables_h[0].shape[1] + tables_w[0].shape[1] + 4) * U * xmax


def op_f32(x, op):
    """One operation of a recipe as the GPU computes it: the float32 restatement where the kernel works in float32, the definition where it
    is exact (integers) or fp64 (noise: equal within 1 float32 ulp, not bit for bit)."""
    if op['op'] == 'blur':
        return blur_f32(x, D.kernel_of(op), op['stride'])
    if op['op'] == 'resize':
        return resize_f32(x, *D.op_tables(op, x.shape[0], x.shape[1]))
    return D.op_ref(x, op)


def ulp_distance(a, b):
    """Distance in float32 ulps between two float32 arrays of finite values (the integer-ordering trick)."""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))

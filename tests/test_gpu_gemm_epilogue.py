"""-m gpu: every instantiation of the three row GEMMs (csrc/gemm_common.h: LDS-DMA fp32, split-bf16 with its 3x3 conv form, one-pass fp16)
on BOTH store paths of the epilogue, at the smallest shapes where it can go wrong.

Rows = block tile + 1 (129; 65 for the 64 x 64 configuration; a 1 x 3 x 43 image = 129 output pixels for the 3x3 form): a second row block
that holds one row.  K = Cin = 64.  N = 40: one ragged column tile on the float4 path, lanes guarded off; N = 130: the scalar path, two or
three column blocks with the last 2 columns wide, and the clamped weight tile.  The fp32 and split cases are bit-exact against the oracle;
the fp16 cases are held to fp16_front_ref.gemm_ref / gemm_bound, GELU bit-exact against the oracle GELU of the plain launch.  Every call
goes through gpu_utils.conv2d, i.e. runs between guard bands at exact operand sizes.  The closing test holds the names that ran against
the library's variant tables.
"""
import numpy as np
import pytest
import torch

import fp16_front_ref as FR
import fp64_ref as R
import gpu_utils as G
from femasr_amd import _lib, synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

K = 64
NS = (40, 130)
RAN = set()         # instantiation names of the cases that ran


def _u(tag, shape, lo=-1.0, hi=1.0):
    return synth.uniform(47, tag, tuple(shape), lo, hi)


def _same(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = got.view(np.uint32) != ref.view(np.uint32)
    assert not bad.any(), f'{what}: not bit-identical in {int(bad.sum())} of {got.size}, first at {tuple(np.argwhere(bad)[0])}'


def _operands(tag, shape, n, nres, ksz=1):
    b, h, w = shape
    x = _u(tag + 'x', (b, h, w, K), -2.0, 2.0)
    wt = _u(tag + 'w', (ksz, ksz, K, n), -0.1, 0.1)
    bias = _u(tag + 'b', (n,), -0.5, 0.5)
    res = [_u(tag + f'r{i}', (b, h, w, n)) for i in range(nres)]
    return (x, wt, bias) + tuple((res + [None, None])[:2])


def _name(shape, n, ksz, pad, act, nres, **flags):
    name = G.conv_variant_name(shape + (K,), n, ksz, 1, pad, act=act, nres=nres, **flags)
    RAN.add(name)
    return name


DMA_CASES = [(cfg, act, nres, n) for cfg in (0, 1, 2) for act in (0, 1) for nres in (0, 1, 2) for n in NS]


@pytest.mark.parametrize('cfg,act,nres,n', DMA_CASES, ids=[f'cfg{c}_act{a}_nres{r}_N{n}' for c, a, r, n in DMA_CASES])
def test_lds_dma_gemm(cuda_device, cfg, act, nres, n):
    lib = _lib.load()
    shape = (1, 1, 65 if cfg == 2 else 129)
    x, wt, bias, r1, r2 = _operands(f'dma{cfg}{act}{nres}{n}', shape, n, nres)
    prev = lib.femasr_gemm_force_config(cfg)
    try:
        name = _name(shape, n, 1, 0, act, nres)
        y = G.conv2d(x, wt, bias, 1, act=act, res1=r1, res2=r2)
    finally:
        lib.femasr_gemm_force_config(prev)
    tile, kb, st = ((2, 4, 2), (2, 2, 3), (1, 4, 2))[cfg]
    assert name == f'gemm_dma<tile=64*{tile},k=8*{kb},stages={st},act={act},nres={nres},vq=false>', name
    _same(y, orc.conv2d(x, wt, bias, 1, 1, 0, False, act=act, res1=r1, res2=r2), name)


S1_CASES = [(act, nres, n) for act in (0, 1) for nres in (0, 1, 2) for n in NS]


@pytest.mark.parametrize('act,nres,n', S1_CASES, ids=[f'act{a}_nres{r}_N{n}' for a, r, n in S1_CASES])
def test_split_gemm(cuda_device, act, nres, n):
    shape = (1, 1, 129)
    x, wt, bias, r1, r2 = _operands(f's1{act}{nres}{n}', shape, n, nres)
    name = _name(shape, n, 1, 0, act, nres, bf16s=True)
    assert name == f'gemm_bf16s<act={act},nres={nres}>', name
    y = G.conv2d(x, wt, bias, 1, act=act, res1=r1, res2=r2, bf16s=True)
    ref = orc.linear_bf16s(x.reshape(-1, K), np.ascontiguousarray(wt.reshape(K, n).T), bias, act,
                           None if r1 is None else r1.reshape(-1, n), None if r2 is None else r2.reshape(-1, n))
    _same(y, ref.reshape(y.shape), name)


S3_CASES = [(nres, n) for nres in (0, 1, 2) for n in NS]


@pytest.mark.parametrize('nres,n', S3_CASES, ids=[f'nres{r}_N{n}' for r, n in S3_CASES])
def test_split_conv3x3(cuda_device, nres, n):
    shape = (1, 3, 43)          # 129 output pixels
    x, wt, bias, r1, r2 = _operands(f's3{nres}{n}', shape, n, nres, ksz=3)
    name = _name(shape, n, 3, 1, 0, nres, bf16s=True)
    assert name == f'conv3x3_bf16s<128px x128,9Cin split GEMM,nres={nres}>', name
    y = G.conv2d(x, wt, bias, 3, 1, 1, res1=r1, res2=r2, bf16s=True)
    _same(y, orc.conv3x3_bf16s(x, wt, bias, r1, r2, stride=1), name)


H_CASES = [(epi, n) for epi in ('plain', 'gelu', 'res') for n in NS]


@pytest.mark.parametrize('epi,n', H_CASES, ids=[f'{e}_N{n}' for e, n in H_CASES])
def test_fp16_gemm(cuda_device, epi, n):
    shape = (1, 1, 129)
    act, nres = int(epi == 'gelu'), int(epi == 'res')
    x, wt, bias, r1, _ = _operands(f'h{epi}{n}', shape, n, nres)
    name = _name(shape, n, 1, 0, act, nres, f16=True)
    assert name == f'gemm_f16<act={act},nres={nres}>', name
    y = G.conv2d(x, wt, bias, 1, act=act, res1=r1, f16=True)
    w_oi = np.ascontiguousarray(wt.reshape(K, n).T)
    ref, mag, rest = FR.gemm_ref(torch.from_numpy(x.reshape(-1, K)), torch.from_numpy(w_oi), torch.from_numpy(bias),
                                 None if r1 is None else torch.from_numpy(r1.reshape(-1, n)))
    if act:     # the GELU epilogue == the oracle's GELU of the same launch without it, bit for bit (as test_gpu_linear_fp16.py)
        plain = G.conv2d(x, wt, bias, 1, act=0, f16=True)
        R.check(plain.reshape(-1, n), ref, FR.gemm_bound(mag, rest), name + ' (plain)')
        _same(y, orc.math_eval('gelu', plain), name)
    else:
        R.check(y.reshape(-1, n), ref, FR.gemm_bound(mag, rest), name)


def test_every_gemm_instantiation_ran(cuda_device):
    """Runs last: the names the cases above launched against the three variant tables as a handle lists them (profile slots), minus the
    VQ epilogue's slots (vq=true; the 64 x 64 configuration's unused VQ slot repeats the name of its first row)."""
    import helpers
    from helpers import synth_weights
    lib = _lib.load()
    cn = sorted(helpers.CONFIGS)[0]
    net = G.build_net(cn, synth_weights(cn, 3, 'trained'))
    _, hnd = net._native(next(net.parameters()).device)
    names = [lib.femasr_profile_name(hnd, i).decode() for i in range(lib.femasr_profile_slots(hnd))]
    listed = {nm for nm in names if nm.startswith(('gemm_dma<', 'gemm_bf16s<', 'conv3x3_bf16s<', 'gemm_f16<')) and 'vq=true' not in nm}
    assert len(listed) == 18 + 9 + 3, sorted(listed)
    ran = set(RAN)          # what this session launched; the tables again, so that a deselected case still counts
    for cfg, act, nres, n in DMA_CASES:
        prev = lib.femasr_gemm_force_config(cfg)
        try:
            _name((1, 1, 65 if cfg == 2 else 129), n, 1, 0, act, nres)
        finally:
            lib.femasr_gemm_force_config(prev)
    for act, nres, n in S1_CASES:
        _name((1, 1, 129), n, 1, 0, act, nres, bf16s=True)
    for nres, n in S3_CASES:
        _name((1, 3, 43), n, 3, 1, 0, nres, bf16s=True)
    for epi, n in H_CASES:
        _name((1, 1, 129), n, 1, 0, int(epi == 'gelu'), int(epi == 'res'), f16=True)
    assert RAN == listed, f'no case for: {sorted(listed - RAN)}; cases under unknown names: {sorted(RAN - listed)}'
    assert ran <= listed, sorted(ran - listed)

"""Host-side logic that needs no GPU: registry semantics, state-dict surface, tile geometry,
rank partition, the deterministic generator, the C-ABI library's exported symbols."""
import math
import os
import re

import numpy as np
import pytest
import torch

from femasr_amd import synth, tiling
from femasr_amd.archs import ARCH_REGISTRY, build_network
from femasr_amd.registry import Registry
from helpers import CONFIGS, key_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_registry_semantics():
    reg = Registry('t')

    @reg.register()
    class A:
        pass

    class B:
        pass
    reg.register(B)
    assert reg.get('A') is A and reg.get('B') is B and 'A' in reg
    with pytest.raises(AssertionError):
        reg.register(A)                      # duplicate name asserts (registry.py:38-41)
    with pytest.raises(KeyError):
        reg.get('missing')
    assert set(reg.keys()) == {'A', 'B'}


@pytest.mark.parametrize('cfg', ['x4', 'x2', 'hq'])
def test_state_dict_surface_matches_reference(cfg):
    """Same keys, order, shapes and dtypes as the reference module (fixture recorded from it)."""
    net = build_network(dict(type='FeMaSRNet', frozen_module_keywords=['quantize'], **CONFIGS[cfg]))
    got = [[k, list(v.shape), str(v.dtype)] for k, v in net.state_dict().items()]
    assert got == key_table(cfg)
    assert 'FeMaSRNet' in ARCH_REGISTRY
    assert net.scale_factor == (CONFIGS[cfg].get('scale_factor', 4) if CONFIGS[cfg]['LQ_stage'] else 1)
    assert net.max_depth == 3 and net.gt_res == 256 and net.use_semantic_loss is False


def test_multi_codebook_keys_and_unsupported_variants():
    """Two codebooks: the state-dict keys / shapes of femasr_arch.py:277-300 (before_quant on 2x channels, CombineQuantBlock
    on e_dim[q-1] + e_dim[q]); the reference's own key table for this config is pinned through the hq2 / x4mc goldens, which
    load synthetic tensors by these keys into the reference with no unexpected key."""
    net = build_network(dict(type='FeMaSRNet', codebook_params=[[32, 1024, 512], [64, 1024, 256]]))
    sd = net.state_dict()
    assert tuple(sd['quantize_group.1.embedding.weight'].shape) == (1024, 256)
    assert tuple(sd['before_quant_group.1.weight'].shape) == (256, 512, 1, 1)
    assert tuple(sd['after_quant_group.1.conv.weight'].shape) == (256, 768, 3, 3)
    with pytest.raises(ValueError):
        build_network(dict(type='FeMaSRNet', codebook_params=[[32, 1024]]))
    with pytest.raises(NotImplementedError):
        build_network(dict(type='FeMaSRNet', codebook_params=[[32, 1024, 512]], norm_type='bn'))


def test_no_cpu_fallback():
    """The product path must fail loudly without a GPU instead of computing on the CPU."""
    from femasr_amd._lib import FemasrError
    net = build_network(dict(type='FeMaSRNet', **CONFIGS['hq']))
    with pytest.raises(FemasrError):
        net.test(torch.zeros(1, 3, 16, 16))


def _reference_tiles(h, w, ts, pad):
    """test_tile's loop restated literally (femasr_arch.py:401-441) as the checker."""
    out = []
    for y in range(math.ceil(h / ts)):
        for x in range(math.ceil(w / ts)):
            ox, oy = x * ts, y * ts
            ex, ey = min(ox + ts, w), min(oy + ts, h)
            out.append((max(oy - pad, 0), min(ey + pad, h), max(ox - pad, 0), min(ex + pad, w), oy, ey, ox, ex))
    return out


@pytest.mark.parametrize('h,w,ts,pad', [(2048, 2048, 240, 16), (2048, 2048, 128, 0), (2048, 2048, 96, 16),
                                         (40, 56, 24, 8), (600, 720, 240, 16), (17, 5, 240, 16)])
def test_tile_enumeration(h, w, ts, pad):
    tiles = tiling.enumerate_tiles(h, w, ts, pad)
    ref = _reference_tiles(h, w, ts, pad)
    assert [(t.y0p, t.y1p, t.x0p, t.x1p, t.y0, t.y1, t.x0, t.x1) for t in tiles] == ref
    cover = np.zeros((h, w), np.int32)
    for t in tiles:
        cover[t.y0:t.y1, t.x0:t.x1] += 1
        ys, ye, xs, xe = t.out_src(4)
        assert ye - ys == (t.y1 - t.y0) * 4 and xe - xs == (t.x1 - t.x0) * 4
        assert ye <= t.in_hw[0] * 4 and xe <= t.in_hw[1] * 4
    assert cover.min() == 1 and cover.max() == 1            # bodies tile the image exactly once


def test_shape_classes_2048():
    """2048^2 at 240/16 -> 81 tiles in 9 classes 49/7/7/7/7/1/1/1/1; at 128/0 -> one class of 256."""
    cl = tiling.shape_classes(tiling.enumerate_tiles(2048, 2048, 240, 16))
    assert sorted((len(v) for v in cl.values()), reverse=True) == [49, 7, 7, 7, 7, 1, 1, 1, 1]
    cl = tiling.shape_classes(tiling.enumerate_tiles(2048, 2048, 128, 0))
    assert list(cl.keys()) == [(128, 128)] and len(cl[(128, 128)]) == 256
    cl = tiling.shape_classes(tiling.enumerate_tiles(2048, 2048, 96, 16))
    assert sum(len(v) for v in cl.values()) == 484


@pytest.mark.parametrize('n,world', [(256, 8), (81, 8), (7, 8), (1, 8), (0, 4), (49, 3)])
def test_rank_partition_is_a_partition(n, world):
    got = []
    for r in range(world):
        lo, hi = tiling.rank_slice(n, r, world)
        assert 0 <= lo <= hi <= n and hi - lo in (n // world, n // world + 1)
        got += list(range(lo, hi))
    assert got == list(range(n))


def test_padded_hw_always_pads():
    assert tiling.padded_hw(128, 128, 4) == (144, 144)      # divisible input still gains one block
    assert tiling.padded_hw(256, 256, 2) == (288, 288)
    assert tiling.padded_hw(20, 28, 4) == (32, 32)
    assert tiling.padded_hw(64, 48, 1) == (128, 64)           # wsz = 64 when scale_factor is 1


def test_synth_is_deterministic_and_keyed():
    a = synth.synth_tensor(0, 'out_conv.bias', (3,))
    b = synth.synth_tensor(0, 'out_conv.bias', (3,))
    c = synth.synth_tensor(1, 'out_conv.bias', (3,))
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    # pinned values: the generator must not drift between the golden container and the GPU box
    u = synth.uniform01(0, 'pin', 4)
    assert [float(v).hex() for v in u] == [float(v).hex() for v in synth.uniform01(0, 'pin', 4)]
    assert np.all((u >= 0) & (u < 1)) and np.all(u * (1 << 24) == np.floor(u * (1 << 24)))
    x = synth.synth_input(3, (1, 3, 8, 8))
    assert x.dtype == np.float32 and x.min() >= 0 and x.max() < 1


def test_cabi_exports_every_declared_symbol():
    """The shared library loads (no GPU needed) and exports every function include/femasr_hip.h declares; the test / measurement hooks
    live in include/femasr_hip_debug.h and are bound separately."""
    from femasr_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'femasr_hip.h')).read()
    declared = set(re.findall(r'\b(femasr_[a-z0-9_]+)\s*\(', hdr))
    declared -= {'femasr_status'}
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    assert not [n for n in declared if 'debug' in n], 'debug hooks belong in include/femasr_hip_debug.h'
    dbg = open(os.path.join(ROOT, 'include', 'femasr_hip_debug.h')).read()
    declared_dbg = set(re.findall(r'^(?:int|size_t)\s+(femasr_[a-z0-9_]+)\s*\(', dbg, re.M))
    assert declared_dbg == set(_lib.DEBUG_SIGNATURES), declared_dbg ^ set(_lib.DEBUG_SIGNATURES)
    lib = _lib.load()
    for name in declared | declared_dbg:
        assert hasattr(lib, name), name
    assert lib.femasr_version() >= 100


def test_counted_waits_of_the_split_gemm():
    """kernels_gemm_bf16.hip feeds its MFMAs from inline-asm loads / LDS-DMA copies behind hand-counted `s_waitcnt vmcnt(N)` waits.  The counts
    hold only if the compiler adds no VMEM instruction of its own to the loop: the build gate disassembles every
    instantiation; here as a test, plus a negative control on a doctored expectation."""
    import sys
    csrc = os.path.join(ROOT, 'femasr_amd', 'csrc')
    if not os.path.exists(os.path.join(csrc, 'kernels_gemm_bf16.o')) or not os.path.exists('/opt/rocm/lib/llvm/bin/llvm-objdump'):
        pytest.skip('no built objects / no llvm-objdump here')
    sys.path.insert(0, csrc)
    import kernel_meta
    assert kernel_meta.check_counted_waits() == []
    keep = dict(kernel_meta.COUNTED)
    try:
        kernel_meta.COUNTED = dict(keep, global_load_lds_dwordx4=11)
        probs = kernel_meta.check_counted_waits()
        assert len(probs) == 9 and all('VMEM instructions in the MFMA loop' in p for p in probs), probs
        kernel_meta.COUNTED = dict(keep, vmcnt={14: 2, 10: 3, 9: 1})
        probs = kernel_meta.check_counted_waits()
        assert len(probs) == 10 and 'update both together' in probs[0], probs
    finally:
        kernel_meta.COUNTED = keep


def test_library_reads_one_environment_variable():
    """libfemasr_hip.so picks no kernel from the caller's environment: the only getenv under femasr_amd/csrc is FEMASR_VQ in
    femasr_finalize_weights (INTEGRATION.md documents it, bench.py labels its output by it).  Test hooks go through include/femasr_hip_debug.h."""
    csrc = os.path.join(ROOT, 'femasr_amd', 'csrc')
    names = []
    for f in sorted(os.listdir(csrc)):
        if f.endswith(('.hip', '.h')):
            names += re.findall(r'getenv\(\s*"?([^")]*)', open(os.path.join(csrc, f)).read())
    assert names == ['FEMASR_VQ'], names


def test_kernel_meta_diff_tells_same_from_differs():
    """kernel_meta.py --diff (how a refactor shows that it left the device code alone): an object against itself is `same` kernel by kernel;
    with one instruction of one kernel changed in memory that kernel, and only that one, `differs`; so does one with another register count.
    A kernel that moved to another object is found there by its symbol: `same` if unchanged, `differs` with one instruction changed."""
    import sys
    csrc = os.path.join(ROOT, 'femasr_amd', 'csrc')
    if not os.path.exists(os.path.join(csrc, 'kernels_layout.o')) or not os.path.exists('/opt/rocm/lib/llvm/bin/llvm-objdump'):
        pytest.skip('no built objects / no llvm-objdump here')
    sys.path.insert(0, csrc)
    import kernel_meta
    held = {'kernels_attn.o': 1, 'kernels_layout.o': 13, 'kernels_norm.o': 10, 'kernels_probe.o': 2}      # the kernels each object holds
    here = kernel_meta.code_of(csrc, objs=list(held))
    assert {f: len(ks) for f, ks in here.items()} == held
    lines = kernel_meta.diff(here, here)
    assert len(lines) == sum(held.values()) and all(what == 'same' for _, _, what in lines), lines
    layout = here['kernels_layout.o']
    victim, other = sorted(layout)[:2]
    insts, meta = layout[victim]
    assert len(insts) > 4
    doctored = dict(layout)
    doctored[victim] = (insts[:3] + [('s_nop', '0')] + insts[4:], meta)
    doctored[other] = (doctored[other][0], ('999',) + doctored[other][1][1:])
    last = sorted(layout)[-1]
    doctored['old_name'] = doctored.pop(last)          # (a kernel whose signature changed: matched only through --rename)
    there = dict(here, **{'kernels_layout.o': doctored})
    got = {n: what for _, n, what in kernel_meta.diff(here, there)}
    assert got.pop(victim) == 'differs' and got.pop(other) == 'differs' and got.pop(last) == 'only here' and got.pop('old_name') == 'only there'
    assert set(got.values()) == {'same'} and len(got) == sum(held.values()) - 3
    got = {n: what for _, n, what in kernel_meta.diff(here, there, rename=[('old_name', last)])}
    assert got[last] == 'same' and 'old_name' not in got and sorted(got.values()).count('differs') == 2
    # one kernel moved from a.o to b.o (b.o exists in this build only), unchanged, then with one instruction changed
    stayed = {n: v for n, v in layout.items() if n != victim}
    for moved, want in ((layout[victim], 'same'), (doctored[victim], 'differs')):
        lines = kernel_meta.diff({'a.o': stayed, 'b.o': {victim: moved}}, {'a.o': layout})
        assert ('b.o < a.o', victim, want) in lines and len(lines) == len(layout), lines
        assert all(f == 'a.o' and what == 'same' for f, n, what in lines if n != victim), lines


def test_kernel_meta_detail_tells_a_moved_loop_instruction():
    """The lines kernel_meta.py --diff prints under a kernel that differs: the MFMA loops of a split-GEMM kernel against themselves are
    `unchanged`; with one LDS read taken out of the loop they are `CHANGED`; one instruction dropped in front of the loop changes nothing."""
    import sys
    csrc = os.path.join(ROOT, 'femasr_amd', 'csrc')
    obj = os.path.join(csrc, 'kernels_gemm_bf16.o')
    if not os.path.exists(obj) or not os.path.exists('/opt/rocm/lib/llvm/bin/llvm-objdump'):
        pytest.skip('no built objects / no llvm-objdump here')
    sys.path.insert(0, csrc)
    import kernel_meta
    name, insts = next((n, i) for n, i in sorted(kernel_meta.disassemble(obj).items()) if 'gemm_bf16s_kernel' in n)
    row = kernel_meta.code_of(csrc, objs=['kernels_gemm_bf16.o'])['kernels_gemm_bf16.o'][name]
    (lo, hi), = kernel_meta.mfma_loops(insts)
    seq = kernel_meta.loop_sequences(insts)
    assert len(seq) == 1 and seq[0].count('s_waitcnt vmcnt(14)') == 2 and 'v_mfma_f32_32x32x16_bf16' in seq[0] and 's_barrier' in seq[0]
    assert kernel_meta.detail(row, row, insts, insts)[-1].endswith('MFMA loops 1 / 1; VMEM, LDS, MFMA, s_waitcnt and s_barrier sequence inside them: unchanged')
    victim = next(i for i in range(lo, hi) if insts[i][1].startswith('ds_read'))
    assert kernel_meta.detail(row, row, insts[:victim] + [(insts[victim][0], 's_nop', '0')] + insts[victim + 1:], insts)[-1].endswith('CHANGED')
    assert kernel_meta.detail(row, row, insts[1:], insts)[-1].endswith('unchanged')


def test_default_schedule_kernels_use_no_scratch():
    """The build gate, as a test: no gfx950 kernel of the default launch schedule touches scratch memory (spilled registers turn into HBM
    traffic: VERDICT r4 found 40 B per thread in the hot Winograd instantiation and 228 B in the codebook search).  Reads the code objects
    the build left next to the sources (llvm-readelf --notes); opt-in / secondary-mode instantiations are named in kernel_meta.ALLOW_SCRATCH."""
    import sys
    csrc = os.path.join(ROOT, 'femasr_amd', 'csrc')
    if not any(f.endswith('.o') for f in os.listdir(csrc)) or not os.path.exists('/opt/rocm/lib/llvm/bin/llvm-readelf'):
        pytest.skip('no built objects / no llvm-readelf here')
    sys.path.insert(0, csrc)
    import kernel_meta
    rows, bad = kernel_meta.check()
    assert len(rows) > 100, len(rows)
    assert not kernel_meta.KNOWN_SCRATCH, 'the default schedule is scratch-free since round 5: do not grow an allow-list again'
    assert not bad, kernel_meta.table(bad)
    hot = [r for r in rows if 'conv3x3_wino4_kernelILi1ELb1ELi1EE' in r['name'] or 'vq_candidates_kernelILi8ELb1E' in r['name']
           or 'gemm_bf16s_kernel' in r['name']]
    assert len(hot) >= 8
    for r in hot:
        assert int(r['vgpr_spill_count']) == 0 and int(r['private_segment_fixed_size']) == 0, r['name']

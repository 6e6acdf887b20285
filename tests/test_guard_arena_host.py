"""The guard-band arena (tests/guard_arena.py) on CPU tensors: its layout rules, one negative control per kind of failure it
exists to catch - each written with plain torch indexing - and a correct operation that passes."""
import re

import numpy as np
import pytest
import torch

import guard_arena as GA


def _arena(poison=GA.POISONS[0], sizes=(1000, 4 * 37, 777)):
    ar = GA.Arena(GA.Arena.room_for(sizes), 'cpu', poison)
    x = np.arange(sizes[0], dtype=np.uint8)
    a = ar.add('x', 'in', sizes[0], x)
    o = ar.add('y', 'out', sizes[1])
    s = ar.add('tmp', 'scratch', sizes[2])
    return ar.arm(), a, o, s


@pytest.mark.parametrize('poison', GA.POISONS)
def test_layout_rules(poison):
    ar, a, o, s = _arena(poison)
    word = np.array([poison], np.uint32).view(np.uint8)
    buf = ar.buf.numpy()
    assert ar.buf.data_ptr() % GA.ALIGN == 0 and buf.size % 4 == 0
    regs = ar.regions
    assert regs[0].off >= 1 << 20 and buf.size - (regs[-1].off + regs[-1].nbytes) >= 1 << 20        # >= 1 MiB margins
    for r in regs:
        assert r.ptr % 256 == 0 and r.ptr == ar.buf.data_ptr() + r.off and r.view.numel() == r.nbytes
        assert r.view.data_ptr() == r.ptr
    for r, n in zip(regs, regs[1:]):
        assert n.off - (r.off + r.nbytes) >= 4096                                                  # >= 4 KiB between regions
    # exact sizes: the byte behind a region, and everything else outside the 'in' data, is the repeating poison word
    mask = np.ones(buf.size, bool)
    mask[a.off:a.off + a.nbytes] = False
    assert np.array_equal(buf[mask], np.tile(word, buf.size // 4)[mask])
    for r in regs:
        end = r.off + r.nbytes
        assert buf[end] == word[end % 4] and buf[r.off - 1] == word[(r.off - 1) % 4]
    assert np.array_equal(a.view.numpy(), np.arange(1000, dtype=np.uint8))
    assert o.as_(torch.int32).numpy().view(np.uint32).tolist() == [poison] * 37
    # the two poisons as numbers
    f = np.array([poison], np.uint32).view(np.float32)[0]
    h = np.array([poison], np.uint32).view(np.float16)
    b = (np.array([poison & 0xFFFF0000, (poison << 16) & 0xFFFFFFFF], np.uint32)).view(np.float32)       # the bf16 halves, widened
    if poison == 0xFFFFFFFF:
        assert np.isnan(f) and np.isnan(h).all() and np.isnan(b).all() and np.array([poison], np.uint32).view(np.int32)[0] == -1
    else:
        # (0x7F7F has fp16's exponent field all ones: as fp16 this poison is a NaN too, with another payload and sign than 0xFFFF)
        assert np.isfinite(f) and f > 3.3e38 and np.isfinite(b).all() and (b > 3e38).all() and np.isnan(h).all()
        assert np.array([poison], np.uint32).view(np.int32)[0] == 2139062143
    with pytest.raises(ValueError):
        ar2 = GA.Arena(GA.Arena.room_for([100]), 'cpu', poison)
        ar2.region(100, 'out')
        ar2.region(1 << 20, 'out')
    with pytest.raises(AssertionError):
        GA.Arena(GA.Arena.room_for([8]), 'cpu', poison).region(8, 'in', np.zeros(9, np.uint8))


def _copy_op(a, o):
    """A correct 'operation': out[i] = int32(in[4i]) for the 37 output words."""
    o.as_(torch.int32)[:] = a.view[0:4 * 37:4].to(torch.int32)


def test_correct_operation_passes():
    ar, a, o, s = _arena()
    _copy_op(a, o)
    s.view[:] = 7
    ar.check('copy')

    def op():
        ar, a, o, s = _arena(GA._POISON[0])
        _copy_op(a, o)
        s.view[:100] = 3          # scratch may keep poison: it is not compared
        ar.check('copy')
        return o.as_(torch.int32).clone()
    got = GA.run_twice(op, 'copy')
    assert got.tolist() == list(range(0, 148, 4))


def _fails(fn, *needles):
    with pytest.raises(GA.GuardError) as e:
        fn()
    msg = str(e.value)
    for n in needles:
        assert re.search(n, msg), (n, msg)
    return msg


def test_control_write_one_byte_after_out():
    ar, a, o, s = _arena()
    _copy_op(a, o)
    ar.buf[o.off + o.nbytes] = 0
    _fails(lambda: ar.check('after'), r"^after: 1 byte", r"after out region 'y'", r'start\+148, end\+0 ')


def test_control_write_one_byte_before_out():
    ar, a, o, s = _arena()
    _copy_op(a, o)
    ar.buf[o.off - 1] = 0
    _fails(lambda: ar.check('before'), r'1 byte', r"before out region 'y'", r'start-1, end-149 ')


def test_control_write_into_in_region():
    ar, a, o, s = _arena()
    _copy_op(a, o)
    a.view[500:503] = 255 - a.view[500:503]
    _fails(lambda: ar.check('in'), r'3 byte', r"inside in region 'x'", r'start\+500, end-500 ')


def test_control_write_100k_away_in_another_regions_separator():
    """A store 100 KiB past `out` lands behind the big scratch region that follows it, inside that region's separator."""
    sizes = (1000, 4 * 37, 98000)
    ar, a, o, s = _arena(sizes=sizes)
    _copy_op(a, o)
    at = o.off + 100 * 1024
    assert s.off + s.nbytes <= at < s.off + s.nbytes + 4096
    ar.buf[at] = 1
    _fails(lambda: ar.check('far'), r'1 byte', r"after scratch region 'tmp'", rf'end\+{at - (s.off + s.nbytes)} ')


def test_control_output_copies_poison_behind_its_input():
    def op():
        ar, a, o, s = _arena(GA._POISON[0])
        _copy_op(a, o)
        behind = ar.buf[_up4(a.off + a.nbytes):][:4].view(torch.int32)         # the first poison word behind the input
        o.as_(torch.int32)[5] = behind[0]
        ar.check('reads past')                                                  # the write side sees nothing
    _fails(lambda: GA.run_twice(op, 'reads past'), r"out region 'y'.* depends on the poison", r'4 byte', r'start\+20, end-128 ')


def _up4(n):
    return (n + 3) // 4 * 4


def test_control_output_element_left_unwritten():
    def op():
        ar, a, o, s = _arena(GA._POISON[0])
        o.as_(torch.int32)[:36] = a.view[0:4 * 36:4].to(torch.int32)             # the last element is never written
        ar.check('unwritten')
    # 0xFFFFFFFF against 0x7F7F7F7F: all four bytes of the word differ
    _fails(lambda: GA.run_twice(op, 'unwritten'), r"out region 'y'.* depends on the poison", r'4 byte', r'start\+144, end-4 ',
           r'\(1 whole word')


def test_run_twice_wants_the_same_regions_and_an_arena():
    with pytest.raises(AssertionError):
        GA.run_twice(lambda: None, 'no arena')
    assert GA._POISON[0] == GA.POISONS[0] and not GA._RECORD                     # state restored after a failure


def test_every_public_size_query_sizes_a_guarded_region():
    """Every size query of the C ABI (femasr_amd/_lib.py SIGNATURES: names ending in _bytes, _floats, _partials, _entries) is asked
    through gpu_utils.q / qp - the helpers that size arena regions and note the name in guard_arena.QUERIED - somewhere in the guarded
    wrappers (tests/gpu_utils.py) or the guard-band cases (tests/test_gpu_guard_band.py)."""
    import os
    from femasr_amd import _lib
    queries = {n for n in _lib.SIGNATURES if n.endswith(('_bytes', '_floats', '_partials', '_entries'))}
    queries.remove('femasr_gn_coeffs_from_partials')            # a kernel entry (the wrapper of the same name guards it), not a query
    assert len(queries) >= 20
    here = os.path.dirname(os.path.abspath(__file__))
    asked = set()
    for f in ('gpu_utils.py', 'test_gpu_guard_band.py'):
        with open(os.path.join(here, f)) as fh:
            asked |= set(re.findall(r"\bqp?\('(femasr_\w+)'", fh.read()))
    assert asked <= queries, f'not size queries of the ABI: {sorted(asked - queries)}'
    assert queries <= asked, f'size queries that size no guarded region: {sorted(queries - asked)}'
    import guard_arena, gpu_utils
    before = set(guard_arena.QUERIED)
    assert gpu_utils.q('femasr_packed_weight_floats', 8, 32, 3, 3) == 9 * 1024 and 'femasr_packed_weight_floats' in guard_arena.QUERIED
    guard_arena.QUERIED.intersection_update(before)

"""-m gpu: one rank of real RCCL in a fresh child process (tests/rccl_one_rank_child.py): the slab path of `TileExchange` and the
serving loop of `StepGather` over `all_gather_into_tensor` of the 'nccl' backend.  What one device cannot show - a second rank, xGMI -
stays uncovered; the per-rank logic of larger worlds is in tests/test_gpu_tile_exchange.py."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

LIMIT = 38          # seconds: five times the measured run, see the test's docstring

EXPECTED = {'backend_is_nccl', 'step_inputs_differ', 'step_0', 'step_1', 'step_2', 'step_3'} | {
    f'tile_{f}_{m}{s}' for f in ('f32', 'u8') for m in ('plain', 'blend') for s in ('', '_through_the_slab')}


def test_one_rank_of_rccl(cuda_device, tmp_path):
    """The child is a fresh process (nothing replaces a running program; two processes hold the GPU while it runs).  No retry; running
    into the time limit is a failure (subprocess.TimeoutExpired).
    Measured once on an MI355X (RCCL 2.26.6): 7.6 s for the child from start to exit - interpreter start, imports, the group's
    initialisation, building the net, fourteen checks -, every boolean true.  LIMIT = 5 x 7.6 s = 38 s: RCCL's start-up varies with the
    load of a shared box."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'rccl_one_rank_child.py')
    p = subprocess.run([sys.executable, child, str(tmp_path)], timeout=LIMIT, capture_output=True)
    out, err = p.stdout.decode(errors='replace'), p.stderr.decode(errors='replace')
    assert p.returncode == 0, f'child exited {p.returncode}\n{out[-2000:]}\n{err[-4000:]}'
    res = json.loads([ln for ln in out.splitlines() if ln.startswith('{')][-1])
    version = res.pop('rccl_version')
    assert set(res) == EXPECTED, (sorted(res), version)
    bad = sorted(k for k, v in res.items() if v is not True)
    assert not bad, f'RCCL {version}: not bit-identical / not true: {bad}'

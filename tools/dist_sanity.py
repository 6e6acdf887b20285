"""RCCL sanity on one GPU box: run under torchrun (any world size); checks that the tile-parallel path (one all_gather
over the NCCL/RCCL backend) reproduces the single-process test_tile output bit for bit.

Without torchrun (world size 1) a one-rank group is made and the call is `test_tile(..., world_size=1, gather=TileExchange())`:
`test_tile_parallel` returns the plain `test_tile` in a world of one, which would compare the call with itself; `_tiled` honours a
gather object it is given, so this leg writes the tiles into the send slab, runs the RCCL all-gather and pastes out of the receive
buffer (tests/test_gpu_rccl_one_rank.py does the same in the suite)."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..'))
from femasr_amd import distributed as fd, synth  # noqa: E402
from femasr_amd.archs.femasr_arch import FeMaSRNet  # noqa: E402


def main():
    rank, world, local = fd.init_from_env()
    torch.cuda.set_device(local)
    if not torch.distributed.is_initialized():       # world size 1: still go through RCCL (one-rank group)
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29555')
        torch.distributed.init_process_group(backend='nccl', rank=0, world_size=1)
    dev = torch.device('cuda', local)
    net = FeMaSRNet(codebook_params=[[32, 1024, 512]], LQ_stage=True, scale_factor=4)
    w = synth.fill_state_dict(net.state_dict(), 5, 'trained')
    net.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    net = net.to(dev).eval()
    x = torch.from_numpy(synth.synth_input(7, (1, 3, 200, 168))).to(dev)
    ref = net.test_tile(x, 96, 16)
    if world == 1:
        got = net.test_tile(x, 96, 16, rank=0, world_size=1, gather=fd.TileExchange())
    else:
        got = fd.test_tile_parallel(net, x, 96, 16)
    same = bool(torch.equal(ref, got))
    print(f'rank {rank}/{world}: tile-parallel == test_tile: {same}; backend {torch.distributed.get_backend()}', flush=True)
    torch.distributed.barrier()
    if not same:
        raise SystemExit(1)


if __name__ == '__main__':
    main()

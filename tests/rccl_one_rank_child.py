"""One rank of real RCCL on one GPU: the child process of tests/test_gpu_rccl_one_rank.py (a script, not collected by pytest).

    python tests/rccl_one_rank_child.py <directory for the rendezvous file>

Initialises a one-rank 'nccl' group (RCCL on ROCm) over a file rendezvous - no TCP port to collide on a shared machine -, then
 1. runs `test_tile` / `test_tile_u8` on (1,3,40,56) at 16/4 with `gather=TileExchange()`, plain and blend=True: the tiles are written
    into the send slab, gathered by `all_gather_into_tensor`, pasted / blended out of the receive buffer; each must be the call without a
    gather, bit for bit;
 2. runs four steps of the weak-scaling serving loop (`StepGather`) with real `net.test(x_k, out=sg.send(k))` forwards on (2,3,24,40)
    inputs that differ per step: result(k-1) is read once launch(k) has returned, the last one after wait_all(); each must be a plain
    `net.test(x_k)` made beforehand - the ordering between the compute stream and the collective's stream.
Prints ONE JSON line of booleans plus the RCCL version, destroys the group, exits 0."""
import json
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from femasr_amd import distributed as fd, synth, tiling  # noqa: E402
from femasr_amd.archs.femasr_arch import FeMaSRNet  # noqa: E402


def main():
    rdv = os.path.join(os.path.abspath(sys.argv[1]), 'rdv')
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    dist.init_process_group(backend='nccl', rank=0, world_size=1, init_method='file://' + rdv)
    res = {'backend_is_nccl': dist.get_backend() == 'nccl' and dist.get_world_size() == 1}
    net = FeMaSRNet(codebook_params=[[32, 1024, 512]], LQ_stage=True, scale_factor=4)
    w = synth.fill_state_dict(net.state_dict(), 5, 'trained')
    net.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    net = net.to(dev).eval()

    x = torch.from_numpy(synth.synth_input(7, (1, 3, 40, 56))).to(dev)
    xu8 = (x[0].permute(1, 2, 0) * 255.0).round().clamp(0, 255).to(torch.uint8).contiguous()
    windows = sum(t.in_hw[0] * t.in_hw[1] for t in tiling.enumerate_tiles(40, 56, 16, 4))         # input pixels of every window, halos included
    for name, fn, img in (('f32', net.test_tile, x), ('u8', net.test_tile_u8, xu8)):
        for blend in (False, True):
            want = fn(img, 16, 4, blend=blend)
            ex = fd.TileExchange()
            got = fn(img, 16, 4, rank=0, world_size=1, gather=ex, blend=blend)
            key = f'tile_{name}_{"blend" if blend else "plain"}'
            res[key] = bool(torch.equal(got, want))
            res[key + '_through_the_slab'] = ex._tg is not None and ex._tg.send.numel() == windows * 16 * 3

    steps = 4
    xs = [torch.from_numpy(synth.synth_input(30 + k, (2, 3, 24, 40))).to(dev) for k in range(steps)]
    wants = [net.test(xk).clone() for xk in xs]
    res['step_inputs_differ'] = not any(torch.equal(wants[0], wk) for wk in wants[1:])
    sg = fd.StepGather(tuple(wants[0].shape), torch.float32, dev)
    for k in range(steps):
        net.test(xs[k], out=sg.send(k))
        sg.launch(k)
        if k >= 1:                                      # launch(k) has waited for step k-1
            res[f'step_{k - 1}'] = bool(torch.equal(sg.result(k - 1)[0], wants[k - 1]))
    sg.wait_all()
    res[f'step_{steps - 1}'] = bool(torch.equal(sg.result(steps - 1)[0], wants[steps - 1]))
    torch.cuda.synchronize()
    res['rccl_version'] = list(torch.cuda.nccl.version())
    print(json.dumps(res), flush=True)
    dist.destroy_process_group()


if __name__ == '__main__':
    main()

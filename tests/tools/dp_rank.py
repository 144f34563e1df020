"""One data-parallel replica of the product's train step (tests/test_gpu_dp.py; launched by dp_spawner.py).

    dp_rank.py OUTDIR [3d] [steps=N] [graph]

Ranks share ONE card and exchange gradients over gloo (RCCL needs one GPU per rank; the product code path --
bucketed all-reduce on the step's streams, grad_scale = 1/world in the Adam kernel, parameter broadcast, per-rank
dropout seed, rank-0 checkpoint -- is the same).  `graph`: use_graph=True (the gradient computation and the update as two
HIP graphs with the all-reduce between them).  Writes OUTDIR/rank{r}.npz: the final state as before and, per step k
under "s{k}.", what the oracle needs to follow this replica step by step -- the state before the step, the losses, the
six generator outputs, grad_all after the exchange, the state after the step and the LeakyReLU branches of the replica's
own forward (util.gate_masks, packed).
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch
import torch.distributed as dist


def main():
    outdir, is3d = sys.argv[1], "3d" in sys.argv[2:]
    nsteps = next((int(a[6:]) for a in sys.argv[2:] if a.startswith("steps=")), 2)
    use_graph = "graph" in sys.argv[2:]
    dist.init_process_group(os.environ.get("TEM_DIST_BACKEND", "gloo"))
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    from oracle import graph                       # test side only: parameter shapes for the shared start state
    from transfer_em_amd.cgan import EM2EM
    from util import DP_OUTPUTS, dp_inputs, gate_masks, pack_masks, scaled_params
    n = 74
    # every rank starts from DIFFERENT weights: the constructor's broadcast must make them rank 0's
    model = EM2EM(n, "dp", is3d=is3d, seed=42, weight_seeds=tuple(100 * rank + i for i in range(4)),
                  checkpoint_root=os.path.join(outdir, f"ckpt{rank}"), use_graph=use_graph)
    init = torch.cat([net.params.theta for net in model._nets]).cpu().numpy()
    if rank == 0:                                  # known start state (the oracle's), then broadcast again
        gs, ds = graph.generator_param_shapes(is3d), graph.discriminator_param_shapes(is3d)
        for net, shapes, seed in zip(model._nets, (gs, gs, ds, ds), (10, 11, 12, 13)):
            net.params.load_dict(scaled_params(shapes, seed))
    model._broadcast_parameters()
    x, y = (torch.from_numpy(a) for a in dp_inputs(rank, is3d, n))

    def state(prefix, out):
        for key, net in zip(("g", "f", "dx", "dy"), model._nets):
            for which in ("theta", "m", "v"):
                out[f"{prefix}{key}.{which}"] = getattr(net.params, which).cpu().numpy()

    out, losses = {}, []
    for k in range(nsteps):
        state(f"s{k}.pre.", out)
        losses.append(model.train_step(x, y).cpu().numpy())
        cs = model._steps[1]
        out[f"s{k}.losses"] = losses[-1]
        out[f"s{k}.grad_all"] = model.grad_all.cpu().numpy()
        for name, plan in DP_OUTPUTS:
            out[f"s{k}.out.{name}"] = cs.fwd[plan].y.float().cpu().numpy()
        out.update(pack_masks(gate_masks(cs), f"s{k}.gate"))
        state(f"s{k}.post.", out)
    ck = model.make_checkpoint(1)
    out.update({"init": init, "losses": np.stack(losses), "grad_all": model.grad_all.cpu().numpy(),
                "seed": np.int64(model.seed), "ckpt": np.array(ck or ""), "step": model.step_dev.cpu().numpy(),
                "nlists": np.int64(len(cs.lists)), "graphs": np.int64(0 if cs.graphs is None else len(cs.graphs))})
    state("", out)
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), **out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

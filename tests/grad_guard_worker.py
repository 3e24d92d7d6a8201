"""Worker of tests/test_hip_grad_guard.py::test_two_ranks_take_the_same_decision (spawned, one process per rank; one rank per
device over RCCL -- with fewer devices than ranks, as tests/diag runs may have it, both on cuda:0 over gloo like
dp_worker): guarded steps with clipping active; on step 2 rank 1 alone writes a NaN into its local gradient before
sync_gradients.  The reduction is not overlapped with backward here, so the NaN written after backward is what gets reduced."""
import os
import sys

import torch


def run(rank, world, port, steps, out_dir):
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for p in (root, os.path.join(root, "gdn-pytorch_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    multi = torch.cuda.device_count() >= world           # (counting devices does not initialise the GPU)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank) if multi else "0",
                      WORLD_SIZE=str(world), GDN_OVERLAP_ALLREDUCE="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    import gdn_amd.AE_model_unet as M
    from gdn_amd import distributed as D
    from gdn_amd import utils as U
    from gdn_amd.optim import Adam
    from oracle import gdn_oracle as O
    D.init(backend="nccl" if multi else "gloo")
    dev = torch.device("cuda", rank if multi else 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    model = M.AutoEncoder_DtoD(input_dim=1, height=32, width=64).to(dev).train()
    model(O.synthetic_batch(2, 32, 64, seed=100 + rank)[0].to(dev), istrain=False)      # builds the arena
    D.broadcast_parameters(model, src=0)
    opt = Adam(model.parameters(), 2e-4, [0.9, 0.999], eps=1e-08, weight_decay=5e-4, max_grad_norm=1e-3, skip_nonfinite=True)
    stats = []
    for s in range(steps):
        depth, _, sparse = [t.to(dev) for t in O.synthetic_batch(2, 32, 64, seed=10 * s + rank)]
        out = model(depth, istrain=False)
        loss, _, _ = U.dtod_loss(out, depth, sparse)
        opt.zero_grad()
        loss.backward()
        if s == 1 and rank == 1:
            model._gdn_param_arena.grad[12345] = float("nan")
        D.sync_gradients(model, opt)
        opt.step()
        stats.append(opt.guard_stats())
    torch.cuda.synchronize()
    torch.save({"stats": stats, "data": model._gdn_param_arena.data.cpu()}, os.path.join(out_dir, "rank%d.pt" % rank))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()

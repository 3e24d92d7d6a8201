"""Worker of tests/test_hip_graph_train.py::test_two_ranks_graph_equals_eager (spawned, one fresh process per rank).  On a box
with one GPU both ranks sit on cuda:0 under GDN_DIST_BACKEND=gloo; with two or more GPUs it is one rank per device over RCCL.
Each rank trains the same start weights on its own shard twice: 6 eager steps (with the overlapped GradReducer), then 2 eager
steps + 4 replays of graph.GraphedDataParallelStep(prewarmed=True), the gradient guard and the weight average on."""
import os
import sys

import torch

STEPS, WARM = 6, 2


def run(rank, world, port, out_dir):
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for p in (root, os.path.join(root, "gdn-pytorch_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    multi = torch.cuda.device_count() >= world           # (counting devices does not initialise the GPU)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank) if multi else "0",
                      WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0")
    if multi:
        os.environ.pop("GDN_DIST_BACKEND", None)
    else:
        os.environ["GDN_DIST_BACKEND"] = "gloo"
    import copy
    import gdn_amd.AE_model_unet as M
    from gdn_amd import distributed as D
    from gdn_amd import utils as U
    from gdn_amd._lib import GdnError
    from gdn_amd.graph import GraphedDataParallelStep, GraphedTrainStep
    from gdn_amd.optim import Adam
    from oracle import gdn_oracle as O
    D.init()
    dev = torch.device("cuda", rank if multi else 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    base = M.AutoEncoder_DtoD(input_dim=1, height=32, width=64)
    batches = [[t.to(dev) for t in O.synthetic_batch(2, 32, 64, seed=10 * s + rank)] for s in range(STEPS)]      # own shard
    out = {"backend": str(torch.distributed.get_backend()), "world": D.world_size()}
    for mode in ("eager", "graph"):
        model = copy.deepcopy(base).to(dev).train()
        model(batches[0][0], istrain=False)              # builds the arena
        D.broadcast_parameters(model, src=0)
        opt = Adam(model.parameters(), 2e-4, [0.9, 0.999], eps=1e-08, weight_decay=5e-4, max_grad_norm=1.0,
                   skip_nonfinite=True, ema_decay=0.9)

        def fwd_bwd(depth, sparse, model=model, opt=opt):
            loss, ol, gl = U.dtod_loss(model(depth, istrain=False), depth, sparse)
            opt.zero_grad()
            U.backward(loss)
            return loss, ol, gl

        def step(depth, sparse, model=model, opt=opt, fwd_bwd=fwd_bwd):
            terms = fwd_bwd(depth, sparse)
            D.sync_gradients(model, opt)
            opt.step()
            return terms

        losses, run_step = [], step
        for s, (depth, _, sparse) in enumerate(batches):
            if mode == "graph" and s == WARM:
                refused = False
                try:
                    GraphedTrainStep(step, (depth, sparse), opt, prewarmed=True)
                except GdnError as e:
                    refused = "single-process" in str(e)
                out["single_graph_refused"] = refused
                w0 = model._gdn_param_arena.data.clone()
                run_step = GraphedDataParallelStep(fwd_bwd, model, opt, (depth, sparse), prewarmed=True)
                out["capture_ran_nothing"] = bool(torch.equal(w0, model._gdn_param_arena.data))
            losses.append("%.4f" % run_step(depth, sparse)[0].item())
        torch.cuda.synchronize()
        red = getattr(model, "_gdn_reducer", None)
        out[mode] = {"sd": {k: v.cpu() for k, v in model.state_dict().items()}, "opt": opt.state_dict(), "losses": losses,
                     "guard": opt.guard_stats(), "reducer": red is not None,
                     "replays": getattr(run_step, "replays", 0)}
    torch.save(out, os.path.join(out_dir, "rank%d.pt" % rank))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()

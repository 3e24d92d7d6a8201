"""Worker of tests/test_resume_cpu.py::test_two_ranks_gather_and_take_back_their_loader_state (spawned, one process per
rank, gloo, no GPU): each rank runs its shard of a loader for a while, the ranks save ONE training state through rank 0,
read it back into fresh objects and must go on with their own batches and draws."""
import os
import sys

import numpy as np
import torch


class _Set:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        a = np.full((4, 6, 1), i, np.uint8)
        return a, np.full((4, 6, 3), i, np.uint8), a


def _seq(loader, epochs, it=None, count=None):
    out = []
    if it is not None:
        for _ in range(count):
            gt = next(it)[0]
            out.append(([int(v) for v in gt[:, 0, 0, 0]], list(loader.last_params)))
        return out
    for _ in range(epochs):
        for gt, _, _ in loader:
            out.append(([int(v) for v in gt[:, 0, 0, 0]], list(loader.last_params)))
    return out


def run(rank, world, port, out_dir, q):
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for p in (root, os.path.join(root, "gdn-pytorch_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank),
                      WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    import torch.distributed as dist
    from gdn_amd import datasets
    from gdn_amd import distributed as D
    from gdn_amd import trainer as T
    from gdn_amd._lib import GdnError
    from gdn_amd.optim import Adam
    try:
        D.init(backend="gloo")
        datasets.ops.kitti_augment = lambda x, params, train: x
        mk = lambda: datasets.GpuAugmentLoader(_Set(16), 2, "cpu", train=True, seed=40 + rank, drop_last=True, rank=rank,
                                               world=world, order_seed=7)
        straight = mk()
        want = _seq(straight, 3)                       # 4 batches per rank and epoch
        first = mk()
        got = _seq(first, 1)
        it = iter(first)
        got += _seq(first, 0, it, 1 + rank)            # the ranks stop at DIFFERENT positions: the entries must not be swapped
        torch.manual_seed(0)
        net = torch.nn.Linear(3, 2)
        path = os.path.join(out_dir, T.STATE_FILE)
        wrote = T.save_training_state(path, net, Adam(net.parameters(), 1e-3), first,
                                      {"epoch": 1, "i": rank, "lr": 1e-3, "model_num": 1, "seen": 20, "step": 5 + rank})
        assert (wrote == path) == (rank == 0), wrote
        dist.barrier()
        state = T.read_training_state(path)
        assert state["world"] == 2 and [s["rank"] for s in state["loader"]] == [0, 1]
        assert [s["pos"] for s in state["loader"]] == [0, 1] and state["loader"][0]["py_rng"] != state["loader"][1]["py_rng"]
        second = mk()
        net2 = torch.nn.Linear(3, 2)
        progress = T.load_training_state(state, net2, Adam(net2.parameters(), 1e-3), second)
        assert progress["epoch"] == 1 and progress["model_num"] == 1
        assert torch.equal(net2.weight, net.weight)
        rest = _seq(second, 2)
        assert got + rest == want, (rank, len(got), len(rest))
        state["world"] = 1
        try:
            T.load_training_state(state, net2, Adam(net2.parameters(), 1e-3), mk())
            raise AssertionError("a state saved by one rank was accepted by two")
        except GdnError:
            pass
        q.put((rank, "ok"))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put((rank, "FAIL: %s\n%s" % (e, traceback.format_exc())))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()

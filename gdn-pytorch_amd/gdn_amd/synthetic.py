"""Synthetic KITTI-shaped batches; the same law as the oracle's recipe."""
import torch


def synthetic_batch(B, H=128, W=416, seed=0, device=None):
    """depth, rgb ~ U(-1,1); sparse = same law where Bernoulli(0.05) else exactly -1 (no LiDAR return)."""
    g = torch.Generator().manual_seed(seed)
    depth = torch.rand(B, 1, H, W, generator=g) * 2 - 1
    rgb = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    sv = torch.rand(B, 1, H, W, generator=g) * 2 - 1
    keep = torch.rand(B, 1, H, W, generator=g) < 0.05
    sparse = torch.where(keep, sv, torch.full_like(sv, -1.0))
    if device is not None:
        depth, rgb, sparse = depth.to(device), rgb.to(device), sparse.to(device)
    return depth, rgb, sparse


class SyntheticLoader:
    """Iterable of `steps` identical-shape batches (gt, rgb, sparse) resident on `device`."""

    def __init__(self, batch_size, steps, H=128, W=416, seed=0, device=None, distinct=1):
        self.steps, self.bs = steps, int(batch_size)
        self._pos, self._resume = -1, None       # the batch last handed out; after load_state_dict(): where to go on
        self.batches = [synthetic_batch(batch_size, H, W, seed + i, device) for i in range(max(1, distinct))]

    def __len__(self):
        return self.steps

    def __iter__(self):
        first, self._resume = self._resume or 0, None
        for i in range(first, self.steps):
            self._pos = i
            yield self.batches[i % len(self.batches)]

    def state_dict(self, epoch_done=False):
        """The position in the epoch (the batches themselves are fixed: there is no random stream to save)."""
        return {"rank": 0, "world": 1, "n": self.steps, "batch_size": self.bs, "pos": -1 if epoch_done else self._pos}

    def load_state_dict(self, state):
        from ._lib import GdnError
        for key, mine, what in (("n", self.steps, "epoch length"), ("batch_size", self.bs, "batch size")):
            if int(state[key]) != mine:
                raise GdnError("loader state was saved with %s %d, this loader has %d" % (what, int(state[key]), mine))
        self._pos = int(state["pos"])
        self._resume = self._pos + 1

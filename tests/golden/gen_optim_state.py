#!/usr/bin/env python3
"""Writes tests/golden/optim_state_v1.pt: what five steps of the fused Adam leave behind on an MI355X, for
tests/test_hip_optim_fixture.py to hold every later revision of gdn_amd/optim.py and of the Adam kernels to, bit for bit.

Public API only (engine.ParamArena, the Adam constructor, step, state_dict, load_state_dict, averaged), so the script runs
unchanged on either side of a change to the optimizer's insides; the test imports it and drives the same steps.  The file
was written by the commit BEFORE the optimizer's state stores became one type.  A pull request that changes the kernels'
arithmetic on purpose regenerates it (python tests/golden/gen_optim_state.py on the GPU box) and says so.

The net is Conv2d(2,3,3), BatchNorm2d(3), ConvTranspose2d(3,2,3) in one arena (384 floats: both tap-major layouts, the
alignment padding) plus one loose Parameter(5).  Gradients come from CPU generators and are copied over.
    step 1  full coverage, norm above max_grad_norm (clipped)
    step 2  full coverage, norm below it
    step 3  the BatchNorm weight has no gradient: per-tensor updates from here on
    step 4  one inf in the gradient: the guarded optimizer skips it (the plain one is not given this step)
    step 5  partial coverage again, the first convolution's gradient a caller-owned tensor instead of its arena slice
Two optimizers, each over a net of its own: Adam(max_grad_norm=1, skip_nonfinite, ema_decay=0.99) and the host-path Adam.
Stored for each: state_dict() and the weights after steps 3 and 5 (and every averaged(p) of the first), and the initial
weights.  Tensors, numbers, strings, lists, tuples and dicts only: read with torch.load(weights_only=True)."""
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent.parent
for _p in (str(ROOT), str(ROOT / "gdn-pytorch_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import torch

PATH = pathlib.Path(__file__).resolve().parent / "optim_state_v1.pt"
HYPER = dict(lr=1e-3, weight_decay=5e-4)
FORMS = {"guarded": dict(max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.99), "plain": {}}
STEPS = {"guarded": (1, 2, 3, 4, 5), "plain": (1, 2, 3, 5)}
NO_GRAD = 2          # index of the BatchNorm weight among the parameters


def make(device, form, weights=None):
    """(parameters, arena, optimizer) of one form; `weights`: logical-shape values to start from instead of the seeded ones."""
    from gdn_amd import engine as E
    from gdn_amd.optim import Adam
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Conv2d(2, 3, 3), torch.nn.BatchNorm2d(3), torch.nn.ConvTranspose2d(3, 2, 3))
    ar = E.ParamArena(net, device)
    net._gdn_param_arena = ar
    loose = torch.nn.Parameter(torch.randn(5, generator=torch.Generator().manual_seed(4)).to(device))
    params = list(net.parameters()) + [loose]
    if weights is not None:
        with torch.no_grad():
            for p, w in zip(params, weights):
                p.copy_(w)
        ar.touch()
    return params, ar, Adam(params, **HYPER, **FORMS[form])


def set_grads(k, params, ar):
    """The gradients of step k = 1..5, the same for both forms."""
    gen = torch.Generator().manual_seed(1000 + k)
    flat, lg, own = torch.randn(ar.numel, generator=gen), torch.randn(5, generator=gen), torch.randn(3, 2, 3, 3, generator=gen)
    if k == 2:
        flat, lg = flat * 0.01, lg * 0.01
    if k == 4:
        flat[7] = float("inf")
    ar.grad.copy_(flat)
    for p in params[:-1]:
        p.grad = ar.grad_view(p)
    params[-1].grad = lg.to(ar.device)
    if k in (3, 5):
        params[NO_GRAD].grad = None
    if k == 5:
        params[0].grad = own.to(ar.device)


def to_cpu(x):
    if torch.is_tensor(x):
        return x.detach().cpu().clone()
    if isinstance(x, dict):
        return {k: to_cpu(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(to_cpu(v) for v in x)
    return x


def snapshot(form, params, opt):
    out = {"state": to_cpu(opt.state_dict()), "weights": [p.detach().cpu().clone() for p in params]}
    if "ema_decay" in FORMS[form]:
        out["avg"] = [opt.averaged(p).detach().cpu().clone(memory_format=torch.contiguous_format) for p in params]
    return out


def run(form, params, ar, opt, steps):
    """Take `steps` (a subset of STEPS[form], in order); {'after3': snapshot, 'after5': snapshot} for those reached."""
    out = {}
    for k in steps:
        set_grads(k, params, ar)
        opt.step()
        if k in (3, 5):
            out["after%d" % k] = snapshot(form, params, opt)
    return out


def generate(device):
    out = {}
    for form in FORMS:
        params, ar, opt = make(device, form)
        out[form] = {"initial": [p.detach().cpu().clone() for p in params]}
        out[form].update(run(form, params, ar, opt, STEPS[form]))
    return out


if __name__ == "__main__":
    torch.save(generate(torch.device("cuda:0")), PATH)
    back = torch.load(PATH, weights_only=True)
    print("wrote", PATH, PATH.stat().st_size, "bytes;", {f: sorted(back[f]) for f in back})

#!/usr/bin/env python3
"""Writes tests/golden/loop_cadence.json: what trainer.train_AE_DtoD / train_AE_RtoD do, and in which order, over runs long
enough to reach every constant of their cadence -- the progress print (50 / 100 batches), the checkpoint (3000 / 700), the
learning-rate decay (epoch > 5 every 1900 / epoch > 2 every 2200), the state file (--save_state, --save_state_every) and the
groups of --accum_steps -- for tests/test_train_loop_cadence_cpu.py to hold every later revision of the loops to.

No GPU and no kernels: the model returns its input, the optimizer and the loader are small objects, and the loops' heavy
seams are replaced for the run (utils.dtod_loss, utils.rtod_pixel_loss, utils.backward, distributed.sync_gradients,
trainer._save_checkpoint, trainer.save_training_state, trainer.validate).  The loops reach all of them through module
globals, so the script runs unchanged on either side of a change to the loops' insides.  The file was written by the commit
BEFORE the two loop bodies became one driver.  A pull request that changes the cadence on purpose regenerates it
(python tests/golden/gen_loop_cadence.py) and says so.

One scenario is one call of a loop.  Recorded for each:
    dense_len, dense_sha256   every event in order: zero_grad, backward, sync, step:<optimizer.micro_batches>, and the sparse ones
    events                    the sparse ones, [position in the dense stream, kind, payload]:
                                  lr        the value written into param_groups[0]['lr']
                                  ckpt      the path given to _save_checkpoint
                                  state     the progress dict given to save_training_state
                                  validate  the epoch given to validate
                                  print     the index of the finished line in `stdout`
    stdout                    the lines, the time-dependent '(%.1f img/s)' figure masked
    returns, micro_batches    what the loop returned (as floats) and optimizer.micro_batches after it
    error                     the exception a refused run raised, [type name, message]"""
import argparse
import contextlib
import hashlib
import json
import pathlib
import re
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent.parent
for _p in (str(ROOT), str(ROOT / "gdn-pytorch_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import torch

PATH = pathlib.Path(__file__).resolve().parent / "loop_cadence.json"
RATE = re.compile(r"\(\S+ img/s\)")
DENSE = ("zero_grad", "backward", "sync", "step")

# name: (loop, n_epochs, loader batches, args of the run, extras)
#   extras: 'sized' False: a loader without __len__; 'guarded': the optimizer has a gradient guard to print;
#           'validate' False: no validation loader; 'progress': the run resumes from it
SCENARIOS = {
    "dtod_cadence": ("DtoD", 8, 3800, dict(save_state=True, save_state_every=1000), {}),
    "rtod_single_accum3": ("RtoD", 4, 4400, dict(accum_steps=3, save_state=True, save_state_every=1000), {}),
    "rtod_single_short": ("RtoD", 2, 5, dict(save_state=True), dict(guarded=True)),
    "rtod_single_short_no_state": ("RtoD", 2, 5, {}, dict(validate=False)),
    "dtod_break_partial_group": ("DtoD", 2, 10, dict(epoch_size=7, accum_steps=3, save_state=True, save_state_every=2),
                                 dict(guarded=True)),
    "dtod_unsized_loader": ("DtoD", 2, 8, dict(epoch_size=100, accum_steps=3, save_state_every=1), dict(sized=False)),
    "dtod_nyu_every_step_state": ("DtoD", 2, 4, dict(dataset="NYU", save_state_every=1), dict(validate=False)),
    "dtod_resume_accum2": ("DtoD", 3, 10, dict(accum_steps=2, save_state=True, save_state_every=3),
                           dict(progress={"epoch": 1, "i": 3, "lr": 1.5e-5, "model_num": 1, "seen": 28, "step": 14,
                                          "accum_steps": 2})),
    "rtod_single_resume_accum2": ("RtoD", 3, 9, dict(accum_steps=2, save_state=True, save_state_every=3),
                                  dict(progress={"epoch": 1, "i": 5, "lr": 1.5e-5, "model_num": 0, "seen": 30, "step": 15,
                                                 "accum_steps": 2})),
    "refuse_graph_with_accum": ("DtoD", 2, 6, dict(graph=True, accum_steps=2), {}),
    "refuse_resume_other_k": ("RtoD", 2, 6, dict(accum_steps=3),
                              dict(progress={"epoch": 0, "i": 1, "lr": 2e-5, "model_num": 0, "seen": 4, "step": 2,
                                             "accum_steps": 2})),
}


class Trace:
    """The dense stream as a running sha256 and a count; the sparse events and the printed lines verbatim."""

    def __init__(self):
        self.sha, self.n, self.events, self.stdout, self._line = hashlib.sha256(), 0, [], [], ""

    def add(self, kind, payload=None):
        self.sha.update(("%s|%s\n" % (kind, json.dumps(payload, sort_keys=True))).encode())
        if kind.split(":")[0] not in DENSE:
            self.events.append([self.n, kind, payload])
        self.n += 1

    def write(self, text):                       # sys.stdout of the run
        self._line += text
        while "\n" in self._line:
            line, self._line = self._line.split("\n", 1)
            self.stdout.append(RATE.sub("(# img/s)", line))
            self.add("print", len(self.stdout) - 1)
        return len(text)

    def flush(self):
        pass


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x, istrain=False):
        return x


class _Group(dict):
    def __init__(self, trace, lr):
        super().__init__(lr=lr)
        self.trace = trace

    def __setitem__(self, k, v):
        if k == "lr":
            self.trace.add("lr", v)
        super().__setitem__(k, v)


class _Optimizer:
    def __init__(self, trace, lr, guarded):
        self.trace, self.param_groups, self.micro_batches, self.guarded, self.steps = trace, [_Group(trace, lr)], 1, guarded, 0

    def zero_grad(self):
        self.trace.add("zero_grad")

    def step(self):
        self.steps += 1
        self.trace.add("step:%d" % self.micro_batches)

    def state_dict(self):
        return {}

    def guard_stats(self):
        return {"norm": 0.5, "coef": 1.0, "clipped": self.steps // 3, "skipped": self.steps // 7, "steps": self.steps}


class _Loader:
    """`n` batches an epoch, the same three CPU tensors each; the first epoch of a resumed run yields what is left of it."""

    def __init__(self, n, done=0):
        self.n, self.done = n, done
        self.batch = (torch.zeros(2, 1, 1, 2), torch.zeros(2, 3, 1, 2), torch.zeros(2, 1, 1, 2))

    def __iter__(self):
        left, self.done = self.n - self.done, 0
        for _ in range(left):
            yield self.batch

    def state_dict(self, epoch_done=False):
        return {"epoch_done": epoch_done}


class _SizedLoader(_Loader):
    def __len__(self):
        return self.n


@contextlib.contextmanager
def _seams(trace):
    from gdn_amd import distributed as D
    from gdn_amd import trainer as T
    from gdn_amd import utils as U
    zero = torch.zeros(())
    new = [(U, "dtod_loss", lambda *a, **k: (zero, zero, zero)),
           (U, "rtod_pixel_loss", lambda *a, **k: (zero, zero, zero)),
           (U, "backward", lambda loss: trace.add("backward")),
           (D, "sync_gradients", lambda model, optimizer: trace.add("sync")),
           (T, "_save_checkpoint", lambda model, path, optimizer=None: trace.add("ckpt", path)),
           (T, "save_training_state", lambda path, model, optimizer, loader, progress: trace.add("state", dict(progress))),
           (T, "validate", lambda args, loader, model, epoch, logger, mode: trace.add("validate", epoch) or ([], [], []))]
    old = [(mod, name, getattr(mod, name)) for mod, name, _ in new]
    stdout = sys.stdout
    try:
        for mod, name, f in new:
            setattr(mod, name, f)
        sys.stdout = trace
        yield T
    finally:
        sys.stdout = stdout
        for mod, name, f in old:
            setattr(mod, name, f)


def run_scenario(name):
    loop, n_epochs, n, flags, extra = SCENARIOS[name]
    trace = Trace()
    progress = extra.get("progress")
    args = argparse.Namespace(**dict(dict(dataset="KITTI", mode="DtoD" if loop == "DtoD" else "RtoD_single"), **flags))
    model, optimizer = _Model(), _Optimizer(trace, 2e-5, extra.get("guarded", False))
    done = 0 if progress is None else progress["i"] + 1
    loader = _SizedLoader(n, done) if extra.get("sized", True) else _Loader(n, done)
    val = ([], object()) if extra.get("validate", True) else (None, None)
    out = {"error": None, "returns": None}
    with _seams(trace) as T:
        try:
            if loop == "DtoD":
                got = T.train_AE_DtoD(args, model, None, None, optimizer, loader, val[0], 2, n_epochs, 2e-5, val[1], None,
                                      progress=progress)
                out["returns"] = None if got is None else float(got)
            else:
                got = T.train_AE_RtoD(args, model, None, None, None, optimizer, loader, val[0], 2, n_epochs, 2e-5, val[1],
                                      None, progress=progress)
                out["returns"] = [None if t is None else float(t) for t in got]
        except Exception as e:  # noqa: BLE001  (a refusal: recorded)
            out["error"] = [type(e).__name__, str(e)]
    out.update(micro_batches=optimizer.micro_batches, dense_len=trace.n, dense_sha256=trace.sha.hexdigest(),
               events=trace.events, stdout=trace.stdout)
    return out


def render(results):
    """The file's text: one event and one printed line per row, so a diff of two recordings reads."""
    def rows(items):
        return "[\n" + ",\n".join("   " + json.dumps(x, sort_keys=True) for x in items) + "\n  ]" if items else "[]"
    parts = []
    for name, r in results.items():
        head = {k: r[k] for k in ("error", "returns", "micro_batches", "dense_len", "dense_sha256")}
        parts.append(' %s: {\n  "head": %s,\n  "events": %s,\n  "stdout": %s\n }' %
                     (json.dumps(name), json.dumps(head, sort_keys=True), rows(r["events"]), rows(r["stdout"])))
    return "{\n" + ",\n".join(parts) + "\n}\n"


def parse(text):
    return {name: dict(r["head"], events=r["events"], stdout=r["stdout"]) for name, r in json.loads(text).items()}


def generate():
    return {name: run_scenario(name) for name in SCENARIOS}


if __name__ == "__main__":
    PATH.write_text(render(generate()))
    back = parse(PATH.read_text())
    print("wrote", PATH, PATH.stat().st_size, "bytes;", {n: (r["dense_len"], len(r["events"])) for n, r in back.items()})

#!/usr/bin/env python3
"""GPU box: what one call of the Eigen-split evaluation (gdn_depth_metrics_std) costs, against the inference
forward of the same batch.  AutoEncoder_DtoD, prediction 128 x 416, B = 8, fp32.

Forms, microseconds per call in a window of 200 back to back on one stream (device events), alternated over `rounds` rounds:
  std-native        ground truth 375 x 1242 uint16 (20 % dense), Garg crop, no median scaling   (1 memset + 3 kernels)
  std-native-med    the same with median scaling                                                (1 memset + 6 kernels)
  std-native-ops, std-native-med-ops   the same two through ops.depth_metrics_std with the boxes already on the device (the
                    forms above upload them per call, pinned)
  std-128-unit      ground truth 128 x 416 in [-1, 1] (kind 2, dense), Garg crop                (1 memset + 3 kernels)
  std-128-unit-med  the same with median scaling
  reference         the existing gdn_depth_metrics at 128 x 416 (unchanged code, for scale)
  flip              gdn_flip_w of the input + gdn_flip_mean of the two outputs
  forward           the inference forward of the same batch (unchanged code: the yardstick)
and the calls into the C ABI one evaluation batch makes under either protocol (tests/libcalls.py).

usage: eval_std_time.py [rounds = 3] [--batch 8] [--out FILE]"""
import json
import pathlib
import statistics
import sys

HERE = pathlib.Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(HERE.parent)); sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "gdn-pytorch_amd"))


def opt_arg(name, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return v
    return default


import numpy as np
import torch
import gdn_amd.AE_model_unet as M
from gdn_amd import ops, trainer
from gdn_amd.calculate_error import compute_errors_device, compute_errors_std_device, eval_boxes
from libcalls import count_library_calls

out = opt_arg("--out", None)
B = int(opt_arg("--batch", "8"))
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
H, W, H0, W0 = 128, 416, 375, 1242
dev = torch.device("cuda:0")


def window(step, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def spread(xs):
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2)}


r = np.random.RandomState(0)
yy = np.linspace(0, 1, H)[:, None]
pred = torch.from_numpy(np.clip(0.7 - 1.5 * yy + r.normal(0, 0.08, (B, 1, H, W)), -1, 1).astype(np.float32)).to(dev)
metres = 5.0 + 75.0 * (1 - np.linspace(0, 1, H0))[:, None] ** 2 + r.normal(0, 1.0, (B, H0, W0))
gt16 = torch.from_numpy(np.where(r.rand(B, H0, W0) < 0.2, np.clip(np.round(metres * 256), 0, 65535), 0).astype(np.uint16)).to(dev)
unit = torch.from_numpy(np.clip(0.6 - 1.4 * yy + r.normal(0, 0.05, (B, 1, H, W)), -1, 1).astype(np.float32)).to(dev)
sizes = [(H0, W0)] * B

torch.manual_seed(0)
model = M.AutoEncoder_DtoD(input_dim=1, height=H, width=W).to(dev).eval()


def forward():
    with torch.no_grad():
        return model(unit, istrain=False)


flipped = torch.empty_like(pred)
boxes = eval_boxes(sizes, "garg").to(dev)
forms = {
    "std-native": lambda: compute_errors_std_device(gt16, sizes, pred, crop="garg"),
    "std-native-med": lambda: compute_errors_std_device(gt16, sizes, pred, crop="garg", median_scaling=True),
    "std-native-ops": lambda: ops.depth_metrics_std(gt16, ops.GT_U16, boxes, pred),          # boxes already on the device
    "std-native-med-ops": lambda: ops.depth_metrics_std(gt16, ops.GT_U16, boxes, pred, median_scaling=True),
    "std-128-unit": lambda: compute_errors_std_device(unit, None, pred, crop="garg"),
    "std-128-unit-med": lambda: compute_errors_std_device(unit, None, pred, crop="garg", median_scaling=True),
    "reference": lambda: compute_errors_device(unit, unit, pred, crop=True),
    "flip": lambda: ops.flip_mean(pred, ops.flip_w(unit), out=flipped),
    "forward": forward,
}
for f in forms.values():
    window(f, 10)
us = {k: [] for k in forms}
for _ in range(rounds):
    for k, f in forms.items():
        us[k].append(window(f, 200 if k != "forward" else 30) * 1e3)
res = {"batch": B, "pred": [H, W], "native": [H0, W0], "rounds": rounds, "us_per_call": {k: spread(v) for k, v in us.items()},
       "rounds_us": {k: [round(x, 2) for x in v] for k, v in us.items()}}
for k, v in res["us_per_call"].items():
    print("%-17s %s us per call" % (k, v))
valid = compute_errors_std_device(gt16, sizes, pred, crop="garg").cpu()[:, 0].tolist()
res["valid_pixels_native"] = valid

# the library calls of one evaluation batch under either protocol (flags off: no call of the new entry points)
import types
loader = [(unit, unit, unit)]
calls = {}
for name, args, fn in (("reference", types.SimpleNamespace(), trainer.validate),
                       ("standard", types.SimpleNamespace(eval_protocol="standard"), trainer.validate_std),
                       ("standard-flip-med", types.SimpleNamespace(eval_protocol="standard", flip_test=True, median_scaling=True),
                        trainer.validate_std)):
    n, _ = count_library_calls(lambda: fn(args, loader, model, 0, None, "DtoD_test"))
    new = {k: v for k, v in n.items() if k in ("gdn_depth_metrics_std", "gdn_flip_w", "gdn_flip_mean", "gdn_depth_metrics")}
    calls[name] = {"total": sum(n.values()), **new}
    print("library calls of one evaluation batch, %-18s %s" % (name, calls[name]))
res["library_calls"] = calls
line = json.dumps(res)
print(line)
if out:
    pathlib.Path(out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(out).write_text(line + "\n")

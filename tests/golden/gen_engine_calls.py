#!/usr/bin/env python3
"""Writes tests/golden/engine_calls.json: every launching call into the C library, with its arguments, that one forward and one
backward of the networks make in each configuration below -- for tests/test_hip_engine_calls.py to hold every later revision
of gdn_amd/engine.py to.  Needs the GPU.  The file was written by the commit BEFORE engine.conv_bn_act was split into its
norm, backward and data-gradient parts.  A pull request that changes the call sequence on purpose regenerates it
(python tests/golden/gen_engine_calls.py) and says so.

A call is recorded as libcalls.canonical_call gives it: the name, integers and floats by value, a geometry by its eleven
fields, every pointer as null / non-null.  The file holds the table of distinct records and, per configuration, the forward's
and the backward's calls as indices into it.

A configuration is a seeded network at batch 2 on oracle.gdn_oracle.synthetic_batch inputs, 16 x 32 unless it says otherwise,
under utils.dtod_loss:
    <net>_<dtype>_train / _freeze_encoder / _freeze_bn / _freeze_bn_affine / _infer
                          AutoEncoder_DtoD (dtod) and AutoEncoder_2 (rtod): plain training, freeze("encoder"), freeze_bn(),
                          freeze_bn() with every gamma and beta frozen too (NULL dgamma / dbeta), eval() under no_grad
    guide_<dtype>         AutoEncoder_DtoD in eval() with nothing trainable and an input that requires a gradient: the eval-mode
                          BatchNorm backward, folded into the epilogue (fp32, and the bf16 layers) and applied separately (the
                          fp32 input layer of the bf16 network)
    legacy_*              the legacy AutoEncoder in fp32: training with BatchNorm; norm='Instance' under freeze_bn() (the network
                          refuses to record a tape through train-mode InstanceNorm layers, so this is how it trains) and in eval()
    convblock_instance, convtblock_instance
                          a standalone ConvBlock / ConvTBlock(norm='Instance') in train mode, the input requiring a gradient
    dtod_<dtype>_no_<switch>
                          AutoEncoder_DtoD, plain training, with one of engine._FUSE_TRAIN_BN, _FUSE_UP2X, _FUSE_UP2X_BF16,
                          _PRUNE_FROZEN set to False.  AutoEncoder_DtoD has no upsampling and plain training nothing frozen, so
                          the switches are also recorded where they act: rtod_fp32_no_FUSE_UP2X, rtod_bf16_no_FUSE_UP2X_BF16
                          and dtod_fp32_freeze_encoder_no_PRUNE_FROZEN.
*_32x64: the same at 32 x 64, the smallest multiple of 16 at which the bf16 direct data gradient of the 64-channel 9x9 layers
emits the producer's BatchNorm-backward partials (gdn_conv_dgrad_bnb_slots is 0 for every layer at 16 x 32 and at 32 x 32);
every other kind of call below is reached at 16 x 32."""
import copy
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent.parent
for _p in (str(ROOT), str(ROOT / "gdn-pytorch_amd"), str(ROOT / "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import torch

PATH = pathlib.Path(__file__).resolve().parent / "engine_calls.json"
NETS = {"dtod": "AutoEncoder_DtoD", "rtod": "AutoEncoder_2"}


def _configs():
    """name -> dict(net=, dtype=, variant=, off=(switches set to False), hw=(H, W))."""
    c = {}
    for net in NETS:
        for dtype in ("fp32", "bf16"):
            for variant in ("train", "freeze_encoder", "freeze_bn", "freeze_bn_affine", "infer"):
                c["%s_%s_%s" % (net, dtype, variant)] = dict(net=net, dtype=dtype, variant=variant)
    for dtype in ("fp32", "bf16"):
        c["guide_%s" % dtype] = dict(net="dtod", dtype=dtype, variant="guide")
    c["legacy_fp32_train"] = dict(net="legacy", dtype="fp32", variant="train")
    c["legacy_instance_fp32_freeze_bn"] = dict(net="legacy_instance", dtype="fp32", variant="freeze_bn")
    c["legacy_instance_fp32_infer"] = dict(net="legacy_instance", dtype="fp32", variant="infer")
    c["convblock_instance"] = dict(net="convblock", dtype="fp32", variant="block")
    c["convtblock_instance"] = dict(net="convtblock", dtype="fp32", variant="block")
    for sw, dtypes in (("_FUSE_TRAIN_BN", ("fp32", "bf16")), ("_FUSE_UP2X", ("fp32",)), ("_FUSE_UP2X_BF16", ("bf16",)),
                       ("_PRUNE_FROZEN", ("fp32",))):
        for dtype in dtypes:
            c["dtod_%s_no%s" % (dtype, sw)] = dict(net="dtod", dtype=dtype, variant="train", off=(sw,))
    c["rtod_fp32_no_FUSE_UP2X"] = dict(net="rtod", dtype="fp32", variant="train", off=("_FUSE_UP2X",))
    c["rtod_bf16_no_FUSE_UP2X_BF16"] = dict(net="rtod", dtype="bf16", variant="train", off=("_FUSE_UP2X_BF16",))
    c["dtod_fp32_freeze_encoder_no_PRUNE_FROZEN"] = dict(net="dtod", dtype="fp32", variant="freeze_encoder", off=("_PRUNE_FROZEN",))
    for name in ("dtod_bf16_train", "dtod_bf16_freeze_bn", "rtod_bf16_train"):
        c[name + "_32x64"] = dict(c[name], hw=(32, 64))
    return c


CONFIGS = _configs()
_BASES = {}


def _base(net, hw):
    """One seeded network of each kind and size on the CPU, never modified (every configuration works on a deep copy)."""
    import gdn_amd.AE_model_unet as M
    key = (net, hw)
    if key not in _BASES:
        torch.manual_seed(11)
        H, W = hw
        if net in NETS:
            m = getattr(M, NETS[net])(input_dim=1 if net == "dtod" else 3, height=H, width=W)
        elif net in ("legacy", "legacy_instance"):
            m = M.AutoEncoder(norm="Instance" if net == "legacy_instance" else "Batch", height=H, width=W)
        elif net == "convblock":
            m = M.ConvBlock(64, 64, kernel_size=3, padding=1, norm="Instance")
        else:
            m = M.ConvTBlock(64, 64, kernel_size=4, padding=1, stride=2, norm="Instance")
        _BASES[key] = m
    return _BASES[key]


def run_config(name, dev):
    """{'fwd': [...], 'bwd': [...]}: the canonical records of the configuration's forward (with its loss) and backward."""
    from gdn_amd import engine as E
    from gdn_amd import utils as U
    from libcalls import record_library_calls
    from oracle import gdn_oracle as O
    cfg = CONFIGS[name]
    net, variant = cfg["net"], cfg["variant"]
    H, W = hw = cfg.get("hw", (16, 32))
    depth, rgb, sparse = [t.to(dev) for t in O.synthetic_batch(2, H, W, seed=70)]
    m = copy.deepcopy(_base(net, hw)).to(dev).compute_dtype(cfg["dtype"]).train()
    if variant == "freeze_encoder":
        m.freeze("encoder")
    elif variant in ("freeze_bn", "freeze_bn_affine"):
        m.freeze_bn()
        if variant == "freeze_bn_affine":
            for p in m.parameters():
                if p.dim() == 1:
                    p.requires_grad_(False)
    elif variant in ("infer", "guide"):
        m.eval()
    saved = {sw: getattr(E, sw) for sw in cfg.get("off", ())}
    state = {}
    try:
        for sw in saved:
            setattr(E, sw, False)
        if variant == "block":
            g = torch.Generator().manual_seed(70)
            x = (torch.rand(2, 64, H, W, generator=g) * 2 - 1).to(dev).requires_grad_()

            def fwd():
                out = m(x)
                state["loss"] = (out * out).mean()
        else:
            x = (depth if net == "dtod" else rgb).clone()
            if variant == "guide":
                for p in m.parameters():
                    p.requires_grad_(False)
                x.requires_grad_()

            def fwd():
                with torch.no_grad() if variant == "infer" else torch.enable_grad():
                    out = m(x, istrain=False)
                    state["loss"] = U.dtod_loss(out, depth, sparse)[0]
        rec = {"fwd": record_library_calls(fwd), "bwd": []}
        if variant != "infer":
            rec["bwd"] = record_library_calls(state["loss"].backward)
        torch.cuda.synchronize()
    finally:
        for sw, v in saved.items():
            setattr(E, sw, v)
    return rec


def check_coverage(runs):
    """Every kind of call the recording is there to pin appears in it; returns the table that is printed."""
    calls = [r for run in runs.values() for part in ("fwd", "bwd") for r in run[part]]

    def n(name, pred=lambda r: True):
        return sum(1 for r in calls if r[0] == name and pred(r))
    want = {
        "path fft (gdn_fftconv_fwd)": n("gdn_fftconv_fwd"),
        "path wino (gdn_winoconv_fwd)": n("gdn_winoconv_fwd"),
        "path wino2 (gdn_wino2conv_fwd)": n("gdn_wino2conv_fwd"),
        "path c1 (gdn_conv_c1_fwd)": n("gdn_conv_c1_fwd"),
        "path direct (gdn_conv_fwd)": n("gdn_conv_fwd"),
        "gdn_bn_bwd": n("gdn_bn_bwd"),
        "gdn_bn_bwd_coeffs": n("gdn_bn_bwd_coeffs"),
        "gdn_bn_eval_bwd, applied separately": n("gdn_bn_eval_bwd", lambda r: r[11] == 1),
        "gdn_bn_eval_bwd, behind a folded epilogue": n("gdn_bn_eval_bwd", lambda r: r[11] == 2),
        "gdn_bn_apply_up2x": n("gdn_bn_apply_up2x"),
        "gdn_bn_frozen_bwd with a dy output": n("gdn_bn_frozen_bwd", lambda r: r[9] == 1),
        "gdn_bn_frozen_bwd without a dy output": n("gdn_bn_frozen_bwd", lambda r: r[9] == 0),
        "gdn_bn_frozen_bwd with NULL dgamma and dbeta": n("gdn_bn_frozen_bwd", lambda r: r[11] == 0 and r[12] == 0),
        "gdn_conv_dgrad with a BatchNorm input": n("gdn_conv_dgrad", lambda r: r[9] == 1),
        "gdn_conv_dgrad with up2x": n("gdn_conv_dgrad", lambda r: r[14] != 0),
        "transform backward with bnb partials": (n("gdn_fftconv_bwd", lambda r: r[20] == 1) + n("gdn_winoconv_bwd", lambda r: r[15] == 1)
                                                 + n("gdn_winoconv_bwd_pair", lambda r: r[15] == 1)),
        "gdn_fftconv_bwd": n("gdn_fftconv_bwd"),
        "gdn_winoconv_bwd / _pair": n("gdn_winoconv_bwd") + n("gdn_winoconv_bwd_pair"),
        "gdn_wino2conv_bwd": n("gdn_wino2conv_bwd"),
        "gdn_conv_c1_wgrad": n("gdn_conv_c1_wgrad"),
    }
    for k, v in want.items():
        print("  %-50s %d" % (k, v))
    missing = [k for k, v in want.items() if v == 0]
    assert not missing, "the recording never reaches: %s" % ", ".join(missing)
    return want


def encode(runs):
    """The file's content: the distinct records once, each configuration as two lists of indices into them."""
    table, index, out = [], {}, {}
    for name, run in runs.items():
        out[name] = {}
        for part in ("fwd", "bwd"):
            ids = []
            for r in run[part]:
                k = json.dumps(r)
                if k not in index:
                    index[k] = len(table)
                    table.append(r)
                ids.append(index[k])
            out[name][part] = ids
    lines = ["{", ' "records": [']
    lines += ["  " + json.dumps(r) + ("," if i + 1 < len(table) else "") for i, r in enumerate(table)]
    lines += [" ],", ' "configs": {']
    names = list(out)
    for i, name in enumerate(names):
        lines.append('  %s: {"fwd": %s,' % (json.dumps(name), json.dumps(out[name]["fwd"], separators=(",", ":"))))
        lines.append('   "bwd": %s}%s' % (json.dumps(out[name]["bwd"], separators=(",", ":")), "," if i + 1 < len(names) else ""))
    lines += [" }", "}"]
    return "\n".join(lines) + "\n"


def decode(text):
    """name -> {'fwd': [records], 'bwd': [records]} of a file encode() wrote."""
    d = json.loads(text)
    return {name: {part: [d["records"][i] for i in ids] for part, ids in run.items()} for name, run in d["configs"].items()}


def main(argv):
    out = pathlib.Path(argv[0]) if argv else PATH
    dev = torch.device("cuda:0")
    runs = {}
    for name in CONFIGS:
        runs[name] = run_config(name, dev)
        print("%-45s %4d forward calls, %4d backward calls" % (name, len(runs[name]["fwd"]), len(runs[name]["bwd"])))
        sys.stdout.flush()
    text = encode(runs)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(text)
    print("%s: %d bytes, %d distinct records" % (out, len(text), len(json.loads(text)["records"])))
    check_coverage(runs)


if __name__ == "__main__":
    main(sys.argv[1:])

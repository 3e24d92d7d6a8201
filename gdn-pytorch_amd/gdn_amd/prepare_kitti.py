"""Write the training, validation and test sets the loaders read from a raw KITTI download.

    python -m gdn_amd.prepare_kitti RAW_ROOT OUT --train_list F [--val_list F] [--test_list F] [--height 128 --width 416]
        [--velo_depth camera|forward] [--depth_scale 80] [--max_depth 100] [--batch 8] [--workers N] [--overwrite]

The lists are in either format kitti_raw.parse_frame_list reads.  Per batch: host threads decode the colour frames and shrink
them with Pillow BILINEAR and read the scans; the scans are projected at the output size (kitti_raw.projection(size=),
ops.velo_project), filled (ops.depth_densify) and both maps encoded as bytes (ops.depth_encode_u8, byte 255 = depth_scale
metres; in the sparse map a return never encodes as 0) on the device; one device-to-host copy; host threads write the files.

    OUT/<DATE>_<DRIVE>_0<C>/<%010d>.jpg            the colour frame, JPEG quality 95
    OUT/<DATE>_<DRIVE>_0<C>/gt/<%010d>.png         the sparse depth
    OUT/<DATE>_<DRIVE>_0<C>/color_gt2/<%010d>.png  the dense depth
    OUT/train.txt, OUT/val.txt                     one scene per line: what datasets.SequenceFolder pairs by sorted name
    OUT/eigen_test/<scene>_<%010d>.png, ..._color_gt.png, ..._gt.png  and OUT/eigen_test_files_{img,color_gt,gt}.txt in list
                                                   order: what datasets.TestFolder reads

Everything that can be refused is refused before anything touches the GPU (a scan file is checked by its size: a non-zero
multiple of 16 bytes), with one line on stderr and exit status 2.  A frame that a list names twice is written once."""
import argparse
import concurrent.futures as cf
import os
import pathlib
import sys

import numpy as np

from ._lib import GdnError
from .kitti_raw import parse_frame_list, projection

SPLITS = ("train", "val", "test")
TEST_DIR = "eigen_test"
TEST_LISTS = {"img": "eigen_test_files_img.txt", "color_gt": "eigen_test_files_color_gt.txt", "gt": "eigen_test_files_gt.txt"}


def build_parser():
    p = argparse.ArgumentParser(prog="python -m gdn_amd.prepare_kitti", description=__doc__.split("\n\n")[0])
    p.add_argument("raw_root", metavar="RAW_ROOT", help="the raw KITTI tree (RAW_ROOT/DATE/calib_*.txt, RAW_ROOT/DATE/DRIVE/...)")
    p.add_argument("out", metavar="OUT", help="the directory to write")
    p.add_argument("--train_list", required=True, metavar="F")
    p.add_argument("--val_list", default=None, metavar="F")
    p.add_argument("--test_list", default=None, metavar="F")
    p.add_argument("--height", type=int, default=128)
    p.add_argument("--width", type=int, default=416)
    p.add_argument("--velo_depth", default="camera", choices=["camera", "forward"])
    p.add_argument("--depth_scale", type=float, default=80.0, help="the depth byte 255 stands for, in metres")
    p.add_argument("--max_depth", type=float, default=100.0, help="the depth the fill inverts at, in metres")
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--workers", type=int, default=0, help="host threads (0: datasets.preload_threads decides)")
    p.add_argument("--overwrite", action="store_true",
                   help="write into an OUT that already holds a train.txt.  Nothing is deleted: files an earlier run with other "
                        "lists left in a scene folder stay there, and SequenceFolder reads every file of a scene it is given")
    return p


def scene_of(frame):
    return "%s_%s_0%d" % (frame["date"], frame["drive"], frame["cam"])


def output_paths(out, split, frame):
    """{'img', 'gt', 'color_gt'} -> the three files of one sample."""
    out, scene, stem = pathlib.Path(out), scene_of(frame), "%010d" % frame["frame"]
    if split == "test":
        base = out / TEST_DIR / ("%s_%s" % (scene, stem))
        return {"img": base.with_name(base.name + ".png"), "gt": base.with_name(base.name + "_gt.png"),
                "color_gt": base.with_name(base.name + "_color_gt.png")}
    return {"img": out / scene / (stem + ".jpg"), "gt": out / scene / "gt" / (stem + ".png"),
            "color_gt": out / scene / "color_gt2" / (stem + ".png")}


def plan(args):
    """Every refusal, on the host -> {split: [frame, ...]} of the lists that were given: the records of parse_frame_list, each
    with 'P', its projection at the output size."""
    if args.height < 1 or args.width < 1:
        raise GdnError("prepare_kitti: a size of %d x %d" % (args.height, args.width))
    if args.batch < 1:
        raise GdnError("prepare_kitti: --batch %d" % args.batch)
    if not (0.0 < args.depth_scale < float("inf")):
        raise GdnError("prepare_kitti: --depth_scale %r is not a finite positive number" % (args.depth_scale,))
    if not (0.2 < args.max_depth < float("inf")):
        raise GdnError("prepare_kitti: --max_depth %r is not a finite number above 0.2" % (args.max_depth,))
    if not os.path.isdir(args.raw_root):
        raise GdnError("prepare_kitti: the raw KITTI tree %r is not a directory" % (args.raw_root,))
    lists = {s: getattr(args, s + "_list") for s in SPLITS}
    for s, f in lists.items():
        if f is not None and not os.path.isfile(f):
            raise GdnError("prepare_kitti: --%s_list %r: no such file" % (s, f))
    if (pathlib.Path(args.out) / "train.txt").exists() and not args.overwrite:
        raise GdnError("prepare_kitti: %s already holds a train.txt (--overwrite writes into it)" % (args.out,))
    frames = {}
    for s, f in lists.items():
        if f is None:
            continue
        seen, frames[s] = set(), []
        for fr in parse_frame_list(f, args.raw_root):           # a frame a list names twice is written once
            key = (fr["date"], fr["drive"], fr["cam"], fr["frame"])
            if key not in seen:
                seen.add(key)
                frames[s].append(fr)
                size = os.path.getsize(fr["scan"])
                if size == 0 or size % 16:
                    raise GdnError("%s holds %d bytes: not one or more points of float32 x, y, z, reflectance (named by %s)"
                                   % (fr["scan"], size, f))
    if not frames["train"]:
        raise GdnError("prepare_kitti: --train_list %r names no frame" % (lists["train"],))
    both = {scene_of(f) for f in frames["train"]} & {scene_of(f) for f in frames.get("val", [])}
    if both:
        raise GdnError("prepare_kitti: scene(s) %s in both the training and the validation list" % ", ".join(sorted(both)))
    calib = {}                              # a calibration file without the fields it needs is refused here, not mid-run
    for fs in frames.values():
        for f in fs:
            key = (f["date_dir"], f["cam"])
            if key not in calib:
                calib[key] = projection(f["date_dir"], f["cam"], size=(args.height, args.width))[0]
            f["P"] = calib[key]
    return frames


def _load(frame, H, W):
    from PIL import Image
    try:
        with Image.open(frame["image"]) as im:
            rgb = np.asarray(im.convert("RGB").resize((W, H), Image.BILINEAR))
    except Exception as e:
        raise GdnError("cannot decode %s: %s" % (frame["image"], e)) from e
    raw = np.fromfile(frame["scan"], dtype=np.float32)
    if raw.size % 4:
        raise GdnError("%s holds %d floats: not x, y, z, reflectance per point" % (frame["scan"], raw.size))
    return rgb, raw.reshape(-1, 4)


def _write(paths, rgb, sparse, dense):
    from PIL import Image
    for p in paths.values():
        p.parent.mkdir(parents=True, exist_ok=True)
    if paths["img"].suffix == ".jpg":
        Image.fromarray(rgb).save(paths["img"], quality=95)
    else:
        Image.fromarray(rgb).save(paths["img"])
    Image.fromarray(sparse).save(paths["gt"])
    Image.fromarray(dense).save(paths["color_gt"])


def run(args, frames, device="cuda"):
    """The batches of every split -> (samples per split, mean share of bytes 0 in the sparse maps, in the dense maps)."""
    import torch
    from . import ops
    from .datasets import assemble_scans, preload_threads
    H, W, out = args.height, args.width, pathlib.Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    empty = np.zeros(2, np.float64)
    total = 0
    with cf.ThreadPoolExecutor(max_workers=preload_threads(args.workers)) as ex:
        writes = []
        for split, fs in frames.items():
            for k in range(0, len(fs), args.batch):
                batch = fs[k:k + args.batch]
                loaded = list(ex.map(lambda f: _load(f, H, W), batch))
                samples = [(pts, f["P"], (H, W)) for f, (_, pts) in zip(batch, loaded)]
                points, offsets, proj, sizes, _, _, _ = assemble_scans(samples, device)
                sparse = ops.velo_project(points, offsets, proj, sizes, H, W, depth=args.velo_depth,
                                          max_points=max(len(s[0]) for s in samples))
                dense = ops.depth_densify(sparse, sizes, max_depth=args.max_depth)
                both = torch.stack([ops.depth_encode_u8(sparse, args.depth_scale, keep_valid=True),
                                    ops.depth_encode_u8(dense, args.depth_scale)]).cpu().numpy()
                empty += (both == 0).reshape(2, -1).mean(axis=1) * len(batch)
                total += len(batch)
                for w in writes:            # the previous batch's files: their errors surface here, and memory stays bounded
                    w.result()
                writes = [ex.submit(_write, output_paths(out, split, f), loaded[i][0], both[0, i], both[1, i])
                          for i, f in enumerate(batch)]
        for w in writes:
            w.result()
    for split in ("train", "val"):
        if split in frames:
            scenes = list(dict.fromkeys(scene_of(f) for f in frames[split]))
            (out / (split + ".txt")).write_text("".join(s + "\n" for s in scenes))
    if "test" in frames:
        for kind, name in TEST_LISTS.items():
            (out / name).write_text("".join("%s\n" % output_paths(out, "test", f)[kind].relative_to(out) for f in frames["test"]))
    return {s: len(fs) for s, fs in frames.items()}, empty[0] / max(total, 1), empty[1] / max(total, 1)


def main(argv=None):
    args = build_parser().parse_args(argv)
    try:
        frames = plan(args)
        counts, sparse_empty, dense_empty = run(args, frames)
    except GdnError as e:
        print(str(e) if str(e).startswith("prepare_kitti: ") else "prepare_kitti: %s" % e, file=sys.stderr)     # one line, no trace
        return 2
    print("=> prepare_kitti: %d samples (%s) at %d x %d in %s; pixels left empty (byte 0) on average: sparse %.2f %%, dense %.2f %%"
          % (sum(counts.values()), ", ".join("%s %d" % kv for kv in counts.items()), args.height, args.width, args.out,
             100.0 * sparse_empty, 100.0 * dense_empty))
    return 0


if __name__ == "__main__":
    sys.exit(main())

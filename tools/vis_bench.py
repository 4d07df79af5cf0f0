#!/usr/bin/env python3
"""The generation CLI (samrs_amd.generate.run) without and with --vis on the same seeded tiles, and what visualize.py does on the
finished files on the host, arms alternating: one JSON line per run.
  plain : generate without --vis
  vis   : generate with --vis (overlays blended and PNG-encoded on the device; the host writes their bytes)
  host  : tool-only -- per image of the `vis` run's output: decode the image and gray/<stem>.png again, paint the class colours,
          PIL Image.blend(image, colours, 0.4), samrs_io_png_write_rgb at zlib level 6.  One thread; thread time per image.
Lines carry images/s of the loop, the host thread ms per image by stage, and for `vis` / `host` the mean overlay file size on the
same pixels (the device encoder has no LZ77 stage, zlib level 6 has).  The synthetic tiles are not photographs: sizes on them are
indicative only.  Thread pools are sized from this process's CPU share.
usage: vis_bench.py [--tiles 320] [--model vit_h] [--reps 2] [--arms plain,vis,host] [--warm 16]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from samrs_amd import generate, tile_io  # noqa: E402
from png_device_bench import make_tiles  # noqa: E402


def run_generate(root, img_dir, ann, n, model, vis):
    boxes = os.path.join(root, f"boxes_{n}.json")
    with open(boxes, "w") as f:
        json.dump({k: ann[k] for k in sorted(ann)[:n]}, f)
    out_dir = os.path.join(root, "out_vis" if vis else "out_plain")
    shutil.rmtree(out_dir, ignore_errors=True)
    ns = argparse.Namespace(images=img_dir, boxes=boxes, out=out_dir, model=model, checkpoint=None, precision="f16", classes=None,
                            n_classes=18, palette=None, box_batch=64, no_rle=False, batch=8, resume=False, timing=True, vis=vis)
    t = generate.run(ns)["timing"]
    stages = {k: round(1e3 * v / t["images"], 2) for k, v in sorted(t["stage_thread_seconds"].items()) if not k.startswith("loop.")}
    r = {"arm": "vis" if vis else "plain", "images": t["images"], "images_per_s": round(t["images"] / t["loop_seconds"], 1),
         "host_ms_per_image": round(sum(stages.values()), 2), "stages_ms_per_image": stages, "cpus": len(os.sched_getaffinity(0))}
    if vis:
        sizes = [os.path.getsize(os.path.join(out_dir, "vis", f)) for f in os.listdir(os.path.join(out_dir, "vis"))]
        r["vis_bytes_mean"] = round(float(np.mean(sizes)), 1)
    return r


def run_host(root, img_dir, n):
    """visualize.py on the `vis` run's finished files; the overlays must equal the device's pixel for pixel."""
    from PIL import Image
    out_dir = os.path.join(root, "out_vis")
    host_dir = os.path.join(root, "out_host")
    shutil.rmtree(host_dir, ignore_errors=True)
    os.makedirs(host_dir)
    lut = tile_io.class_lut(generate.default_palette(18))
    stems = sorted(os.path.splitext(f)[0] for f in os.listdir(os.path.join(out_dir, "gray")))[:n]
    sizes, equal = [], True
    t0, c0 = time.perf_counter(), time.thread_time()
    for stem in stems:
        image = tile_io.read_rgb(os.path.join(img_dir, stem + ".png"))
        seg = tile_io.read_rgb(os.path.join(out_dir, "gray", stem + ".png"))[..., 0]
        colour = np.empty_like(image)
        for c in np.unique(seg):                                          # visualize.py paints class by class
            colour[seg == c] = lut[c]
        over = np.asarray(Image.blend(Image.fromarray(image), Image.fromarray(colour), 0.4))
        path = os.path.join(host_dir, stem + ".png")
        tile_io.write_rgb(path, over, 6)
        sizes.append(os.path.getsize(path))
    wall, cpu = time.perf_counter() - t0, time.thread_time() - c0
    for stem in stems[:8]:                                                # outside the clock: the two arms wrote the same pixels
        equal &= bool(np.array_equal(tile_io.read_rgb(os.path.join(host_dir, stem + ".png")),
                                     tile_io.read_rgb(os.path.join(out_dir, "vis", stem + ".png"))))
    return {"arm": "host", "images": len(stems), "images_per_s": round(len(stems) / wall, 1),
            "host_ms_per_image": round(1e3 * cpu / len(stems), 2), "vis_bytes_mean": round(float(np.mean(sizes)), 1),
            "pixels_equal_device": equal, "cpus": len(os.sched_getaffinity(0))}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=320)
    ap.add_argument("--model", default="vit_h")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--arms", default="plain,vis,host")
    ap.add_argument("--warm", type=int, default=16, help="tiles of an unmeasured first run per generate arm (kernel load, allocator)")
    a = ap.parse_args()
    arms = a.arms.split(",")
    root = tempfile.mkdtemp(prefix="samrs_vis_")
    try:
        img_dir, ann = make_tiles(root, a.tiles)
        if a.warm:
            for arm in arms:
                if arm != "host":
                    run_generate(root, img_dir, ann, a.warm, a.model, arm == "vis")
        for rep in range(a.reps):
            for arm in arms:
                r = run_host(root, img_dir, a.tiles) if arm == "host" else run_generate(root, img_dir, ann, a.tiles, a.model, arm == "vis")
                r["rep"] = rep
                print(json.dumps(r), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()

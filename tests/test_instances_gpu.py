"""GPU: HRSC instance evaluation -- samrs_gt_match (ground-truth intersection / area / masks on the device) against numpy,
InstancePipeline(gt=True) against a gt=False run of the same stream, and the instances CLI end to end against a host
restatement (InstancePrompter masks, numpy ground truths, rle.encode), with --resume and two ranks sharing this GPU.
Integer work on both sides: every comparison is exact."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from samrs_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sam(name="vit_tiny", **kw):
    import samrs_amd
    return samrs_amd.sam_model_registry[name](**kw).to("cuda")


def _gt_numpy(label, colors):
    return (label[None] == colors[:, None, None, :]).all(-1)


def _label_case(h, w, n, seed):
    """Label image of a few palette colours; instance colours that occur, one absent, one duplicated, and one that only
    occurs at the last pixel (the ragged tail when h * w % 16 != 0)."""
    rng = np.random.default_rng(seed)
    palette = rng.integers(0, 256, size=(6, 3), dtype=np.uint8)
    label = palette[rng.integers(0, 6, size=(h, w))]
    tail = np.array([1, 2, 3], dtype=np.uint8)
    label[-1, -1] = tail
    colors = palette[rng.integers(0, 6, size=n)]
    colors[0] = [7, 7, 7]                                  # absent (palette draws never hit it exactly: checked below)
    if n > 2:
        colors[2] = colors[1]                              # duplicated
    if n > 3:
        colors[3] = tail
    colors[0] = colors[0] if not (label == colors[0]).all(-1).any() else [0, 0, 0]
    masks = rng.integers(0, 4, size=(n, h, w), dtype=np.uint8) * rng.integers(0, 2, size=(n, h, w), dtype=np.uint8) * 50
    return label, colors.astype(np.uint8), masks


@pytest.mark.parametrize("h,w", [(1024, 1024), (600, 800), (517, 803), (1, 1), (3, 8192)])
def test_gt_match_equals_numpy(h, w):
    from samrs_amd import engine
    sam = _sam(max_images=1, max_prompts=8)
    eng = sam.engine
    n = 70                                                   # more than one 64-instance counter chunk
    label, colors, masks = _label_case(h, w, n, seed=h * 7 + w)
    gt = _gt_numpy(label, colors)
    mk = torch.from_numpy(masks).cuda()
    lab, col = torch.from_numpy(label).cuda(), torch.from_numpy(colors).cuda()
    gm = torch.full((n, h, w), 9, dtype=torch.uint8, device="cuda")
    inter, gta, gmo = eng.gt_match(mk, lab, col, gt_masks_out=gm)
    torch.cuda.synchronize()
    want_inter = ((masks != 0) & gt).reshape(n, -1).sum(1)
    want_gt = gt.reshape(n, -1).sum(1)
    assert np.array_equal(inter.cpu().numpy(), want_inter)
    assert np.array_equal(gta.cpu().numpy(), want_gt)
    assert np.array_equal(gmo.cpu().numpy(), gt.astype(np.uint8))
    assert want_gt[0] == 0 and (n <= 2 or want_gt[1] == want_gt[2])
    if h * w > 1:
        assert want_gt[3] >= 1                              # the tail colour is found
    # without gt_masks_out, into caller-owned slices of a larger table; the outputs are overwritten, not accumulated
    tab = torch.full((2, n + 3), -5, dtype=torch.int64, device="cuda")
    eng.gt_match(mk, lab, col, inter_out=tab[0, 1:n + 1], gt_area_out=tab[1, 1:n + 1])
    eng.gt_match(mk, lab, col, inter_out=tab[0, 1:n + 1], gt_area_out=tab[1, 1:n + 1])
    t = tab.cpu().numpy()
    assert np.array_equal(t[0, 1:n + 1], want_inter) and np.array_equal(t[1, 1:n + 1], want_gt)
    assert (t[:, 0] == -5).all() and (t[:, n + 1:] == -5).all()
    # argument validation at the C ABI
    lib = eng.lib
    rc = lib.samrs_gt_match(eng.handle, mk.data_ptr(), 0, h, w, lab.data_ptr(), col.data_ptr(), tab.data_ptr(), tab.data_ptr(), None, None)
    assert rc == engine.ERR_BAD_ARG
    rc = lib.samrs_gt_match(eng.handle, mk.data_ptr(), n, h, w, None, col.data_ptr(), tab.data_ptr(), tab.data_ptr(), None, None)
    assert rc == engine.ERR_BAD_ARG


def _paint_labels(h, w, polys, colors):
    """A label image with each object's rotated box painted in its colour (later objects on top), on a grey background."""
    label = np.full((h, w, 3), 128, dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    for p, c in zip(polys, colors):
        inside = np.ones((h, w), dtype=bool)
        sgn = None
        for k in range(4):
            x0, y0 = p[k]
            x1, y1 = p[(k + 1) % 4]
            cross = (x1 - x0) * (yy - y0) - (y1 - y0) * (xx - x0)
            if sgn is None:
                sgn = 1.0 if ((x1 - x0) * (p[(k + 2) % 4][1] - y0) - (y1 - y0) * (p[(k + 2) % 4][0] - x0)) >= 0 else -1.0
            inside &= sgn * cross >= 0
        label[inside] = c
    return label


def _colors(n, seed):
    rng = np.random.default_rng(seed)
    cols = rng.integers(0, 256, size=(n, 3), dtype=np.uint8)
    if n > 2:
        cols[1] = cols[0]                                     # duplicated colour: identical ground truths
    if n > 3:
        cols[3] = [128, 128, 128]                             # the background colour
    return cols


@pytest.mark.parametrize("prompt", ["box", "rbox_mask", "point"])
@pytest.mark.parametrize("multimask", [False, True])
def test_instance_pipeline_gt(prompt, multimask):
    from samrs_amd import driver, rle
    sam = _sam(max_images=4, max_prompts=6)
    sizes = [(1024, 1024), (600, 800), (517, 803)]
    items = []
    for i, (h, w) in enumerate(sizes):
        img = synth.make_image(60 + i, h, w)
        polys, labels = synth.make_rboxes(60 + i, 9, h, w)
        cols = _colors(9, 60 + i)
        if i == 2:
            cols[5] = [1, 2, 3]                               # occurs nowhere
        label = _paint_labels(h, w, polys, cols)
        ann = polys.mean(1).astype(np.float32) if prompt == "point" else polys
        items.append(driver.WorkItem(f"t{i}", img, ann, labels, (label, cols)))

    def collect(pipe):
        got = {}

        def sink(results, release):
            for r in results:
                got[r.key] = r
                r.rles = [r.rle(j) for j in range(len(r.labels))]
                r.gts = [r.gt_rle(j) for j in range(len(r.labels))]
                r.areas, r.quality = r.areas.copy(), r.quality.copy()
                r.masks = None if r.masks is None else r.masks.copy()
            release()

        assert pipe.run(driver.batched(items, 2), sink) == len(items)
        return got

    kw = dict(prompt=prompt, multimask=multimask, batch=2, box_batch=6, max_boxes=16, rle=True, rle_buffer_mb=16)
    with_gt = collect(driver.InstancePipeline(sam, 1, gt=True, **kw))
    ref = collect(driver.InstancePipeline(sam, 1, keep_masks=True, **kw))
    for it in items:
        a, b = with_gt[it.key], ref[it.key]
        assert a.seg_mask is None and b.seg_mask is None and a.size == b.size and a.masks is None
        assert np.array_equal(a.areas, b.areas) and np.array_equal(a.quality, b.quality) and a.rles == b.rles
        assert b.inter is None and b.gt_area is None and b.gts == [None] * len(b.labels)
        label, cols = it.gt
        gt = _gt_numpy(label, cols)
        pm = b.masks.astype(bool)
        assert np.array_equal(a.inter, (pm & gt).reshape(len(cols), -1).sum(1)), it.key
        assert np.array_equal(a.gt_area, gt.reshape(len(cols), -1).sum(1)), it.key
        for j in range(len(cols)):
            assert a.gts[j] == rle.encode(gt[j]), f"{it.key} object {j}: device ground-truth RLE differs"
    # a label image of another size is refused, naming the item
    bad = driver.WorkItem("odd-one", items[0].image, items[0].boxes, items[0].labels, (items[1].gt[0], items[0].gt[1]))
    with pytest.raises(ValueError, match="odd-one"):
        driver.InstancePipeline(sam, 1, gt=True, **kw).run([[bad]], lambda res, rel: rel())


# ------------------------------------------------------------------------------------------------
# the CLI end to end
# ------------------------------------------------------------------------------------------------
def _hrsc_xml(path, objs):
    rows = []
    for o in objs:
        rows.append("<HRSC_Object>" + "".join(f"<{k}>{v}</{k}>" for k, v in o.items()) + "</HRSC_Object>")
    with open(path, "w") as f:
        f.write("<HRSC_Image><HRSC_Objects>" + "".join(rows) + "</HRSC_Objects></HRSC_Image>")


def _write_dataset(root):
    from PIL import Image
    from samrs_amd import tile_io
    img_dir, ann_dir, lab_dir = (os.path.join(root, d) for d in ("images", "ann", "labels"))
    for d in (img_dir, ann_dir, lab_dir):
        os.makedirs(d)
    sizes = {"s2": (600, 800), "s0": (517, 803), "s1": (1024, 1024), "s3": (480, 640)}
    for k, (stem, (h, w)) in enumerate(sizes.items()):
        Image.fromarray(synth.make_image(80 + k, h, w)).save(os.path.join(img_dir, stem + ".bmp"))
        polys, _ = synth.make_rboxes(80 + k, 7, h, w)
        cols = _colors(7, 80 + k)
        objs = []
        for p, c in zip(polys.astype(np.float64), cols):
            cx, cy = p.mean(0)
            bw, bh = np.linalg.norm(p[1] - p[0]), np.linalg.norm(p[3] - p[0])
            ang = math.atan2(p[1][1] - p[0][1], p[1][0] - p[0][0])
            ang = (ang + math.pi / 2) % math.pi - math.pi / 2                  # le90 range
            objs.append({"box_xmin": int(p[:, 0].min()), "box_ymin": int(p[:, 1].min()), "box_xmax": int(p[:, 0].max()),
                         "box_ymax": int(p[:, 1].max()), "mbox_cx": f"{cx:.4f}", "mbox_cy": f"{cy:.4f}", "mbox_w": f"{bw:.4f}",
                         "mbox_h": f"{bh:.4f}", "mbox_ang": f"{ang:.6f}", "seg_color": "{},{},{}".format(*c)})
        if stem == "s3":
            objs[2]["seg_color"] = "12,34"                                       # the reference skips the whole image
        _hrsc_xml(os.path.join(ann_dir, stem + ".xml"), objs)
    return img_dir, ann_dir, lab_dir, sizes


def _paint_dataset_labels(img_dir, ann_dir, lab_dir, sizes):
    from samrs_amd import instances, tile_io
    for stem, (h, w) in sizes.items():
        a = instances.read_hrsc_xml(os.path.join(ann_dir, stem + ".xml"))
        tile_io.write_rgb(os.path.join(lab_dir, stem + ".png"), _paint_labels(h, w, a.rboxes, a.colors))


def _host_restatement(img_dir, ann_dir, lab_dir, prompt, batch, box_batch):
    """What the reference driver computes, from the one-image-at-a-time prompter, numpy ground truths and rle.encode."""
    import samrs_amd
    from samrs_amd import driver, generate, instances, rle, tile_io
    sam = samrs_amd.sam_model_registry["vit_tiny"](options=generate.default_split_options(None), max_images=2 * batch,
                                                    max_prompts=box_batch).to("cuda")
    prm = driver.InstancePrompter(samrs_amd.SamPredictor(sam))
    stems = sorted(s for s in os.listdir(ann_dir))
    stems = [s[:-4] for s in stems if not instances.read_hrsc_xml(os.path.join(ann_dir, s)).skip]
    pred, gts, pms, gms = [], [], [], []
    for stem in stems:
        a = instances.read_hrsc_xml(os.path.join(ann_dir, stem + ".xml"))
        img = np.asarray(__import__("PIL.Image", fromlist=["Image"]).open(os.path.join(img_dir, stem + ".bmp")).convert("RGB"))
        if prompt == "box":
            m, q = prm.predict(img, "box", hboxes=synth.enclosing_hboxes(a.rboxes))
        elif prompt == "rbox_mask":
            m, q = prm.predict(img, "rbox_mask", rboxes=a.rboxes)
        else:
            m, q = prm.predict(img, "point", points=a.points)
        label = tile_io.read_rgb(os.path.join(lab_dir, stem + ".png"))
        pred.append((m.cpu().numpy(), q.cpu().numpy()))
        gts.append(_gt_numpy(label, a.colors))
    sam_json = []
    gt_json = {"images": [], "annotations": [], "categories": [{"id": 0, "name": "ship", "supercategory": "None"}]}
    for n, (stem, g) in enumerate(zip(stems, gts)):
        gt_json["images"].append({"id": n, "width": g.shape[2], "height": g.shape[1], "file_name": f"{stem}.png"})
    for n, ((m, q), g) in enumerate(zip(pred, gts)):
        for c in range(m.shape[0]):
            sam_json.append({"image_id": n, "category_id": 0, "segmentation": rle.encode(m[c]), "score": float(q[c])})
        for c in range(g.shape[0]):
            gt_json["annotations"].append({"id": c, "image_id": n, "category_id": 0, "area": int(g[c].sum()), "iscrowd": 0,
                                           "segmentation": rle.encode(g[c]), "attributes": {}})
    avg, area = driver.mean_iou([m for m, _ in pred], gts)
    return stems, json.dumps(sam_json), json.dumps(gt_json), avg, area


def _cli_args(img_dir, ann_dir, lab_dir, out, prompt, extra=()):
    return ["--images", img_dir, "--annotations", ann_dir, "--gt-labels", lab_dir, "--out", out, "--prompt", prompt,
            "--model", "vit_tiny", "--batch", "2", "--box-batch", "4", *extra]


def _outputs(out, tag):
    return {name: open(os.path.join(out, name), "rb").read() for name in (f"sam_ins_{tag}.json", f"gt_ins_{tag}.json", "miou.json")}


@pytest.mark.parametrize("prompt", ["box", "rbox_mask", "point"])
def test_instances_cli_end_to_end(tmp_path, prompt, capsys):
    from samrs_amd import instances
    img_dir, ann_dir, lab_dir, sizes = _write_dataset(str(tmp_path))
    _paint_dataset_labels(img_dir, ann_dir, lab_dir, sizes)
    tag = instances.TAGS[prompt]
    out = str(tmp_path / "out")
    rec = instances.main(_cli_args(img_dir, ann_dir, lab_dir, out, prompt))
    stems, sam_txt, gt_txt, avg, area = _host_restatement(img_dir, ann_dir, lab_dir, prompt, 2, 4)
    assert stems == ["s0", "s1", "s2"]                                             # sorted; s3 skipped
    files = _outputs(out, tag)
    assert files[f"sam_ins_{tag}.json"].decode() == sam_txt
    assert files[f"gt_ins_{tag}.json"].decode() == gt_txt
    assert rec == json.loads(files["miou.json"]) and rec["average"] == avg and rec["area"] == area
    assert rec["n_instances"] > 0
    assert f"Average mIOU:  {avg} Area mIOU:  {area}" in capsys.readouterr().out
    assert sorted(os.listdir(os.path.join(out, "parts"))) == ["s0.json", "s1.json", "s2.json"]
    # --resume: nothing left to do, the merge gives the same bytes; a lost fragment is recomputed
    instances.main(_cli_args(img_dir, ann_dir, lab_dir, out, prompt, ["--resume"]))
    assert _outputs(out, tag) == files
    os.remove(os.path.join(out, "parts", "s1.json"))
    instances.main(_cli_args(img_dir, ann_dir, lab_dir, out, prompt, ["--resume"]))
    assert _outputs(out, tag) == files
    # without ground truth: only the predictions
    out2 = str(tmp_path / "out_nogt")
    args = _cli_args(img_dir, ann_dir, lab_dir, out2, prompt)
    i = args.index("--gt-labels")
    assert instances.main(args[:i] + args[i + 2:]) is None
    assert open(os.path.join(out2, f"sam_ins_{tag}.json")).read() == sam_txt
    assert not os.path.exists(os.path.join(out2, f"gt_ins_{tag}.json")) and not os.path.exists(os.path.join(out2, "miou.json"))


def test_instances_cli_two_ranks_share_the_gpu(tmp_path):
    """Two ranks on this GPU over gloo (SAMRS_SHARE_GPU=1): the static shards, the barrier and rank 0's merge give the same bytes
    as one rank."""
    from samrs_amd import instances
    img_dir, ann_dir, lab_dir, sizes = _write_dataset(str(tmp_path))
    _paint_dataset_labels(img_dir, ann_dir, lab_dir, sizes)
    one, two = str(tmp_path / "one"), str(tmp_path / "two")
    instances.main(_cli_args(img_dir, ann_dir, lab_dir, one, "box"))
    env = dict(os.environ, SAMRS_SHARE_GPU="1", PYTHONDONTWRITEBYTECODE="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29547", "-m", "samrs_amd.instances", *_cli_args(img_dir, ann_dir, lab_dir, two, "box", ["--batch", "1"])]
    r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert _outputs(two, "rhbox") == _outputs(one, "rhbox")
    assert r.stdout.count("Average mIOU:") == 1                                      # rank 0 merges and prints

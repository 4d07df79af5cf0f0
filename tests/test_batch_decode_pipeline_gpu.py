"""GPU: batch_decode (one Engine.predict_multi per batch instead of one predict per tile and box chunk) in TilePipeline,
InstancePipeline and the two CLIs: every output equals the default run byte for byte."""
import os

import numpy as np
import pytest

from samrs_amd import synth, tile_io

pytestmark = pytest.mark.gpu


def _sam(**kw):
    import samrs_amd
    return samrs_amd.sam_model_registry["vit_tiny"](precision="f16", **kw).to("cuda")


def _tile_items(driver, sizes, counts):
    items = []
    for i, ((h, w), n) in enumerate(zip(sizes, counts)):
        boxes, labels = synth.make_boxes(90 + i, n, h, w)
        items.append(driver.WorkItem(f"img{i}", synth.make_image(90 + i, h, w), boxes, labels))
    return items


@pytest.mark.parametrize("ragged", [False, True])
def test_tile_pipeline_batch_decode_equals_default(ragged):
    from samrs_amd import driver
    sam = _sam(max_images=6, max_prompts=16)
    sizes = [(1024, 1024), (600, 800), (1024, 1024), (517, 803), (1024, 1024), (1024, 1024)] if ragged else [(1024, 1024)] * 6
    counts = [3, 21, 0, 9, 40, 1]
    items = _tile_items(driver, sizes, counts)
    lut = tile_io.class_lut(np.random.default_rng(2).integers(0, 256, (18, 3), dtype=np.uint8))

    def collect(**kw):
        pipe = driver.TilePipeline(sam, 18, batch=3, box_batch=20, max_boxes=64, rle=True, rle_buffer_mb=16, png_lut=lut, **kw)
        got = {}

        def sink(results, release):
            for r in results:
                got[r.key] = (r.seg_mask.copy(), r.areas.copy(), [r.rle(j) for j in range(len(r.labels))],
                              bytes(r.png("gray")), bytes(r.png("color")))
            release()
        assert pipe.run(driver.batched(items, 3), sink) == len(items)
        return got, pipe.class_pixels.cpu(), pipe.class_instances.cpu()

    ref, cp0, ci0 = collect()
    got, cp1, ci1 = collect(batch_decode=True)
    assert sorted(ref) == sorted(got)
    for k in ref:
        a, b = ref[k], got[k]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), k
        assert a[2] == b[2] and a[3] == b[3] and a[4] == b[4], k
    assert (cp0 == cp1).all() and (ci0 == ci1).all()


@pytest.mark.parametrize("prompt", ["box", "rbox_mask", "point"])
def test_instance_pipeline_batch_decode_equals_default(prompt):
    import test_instances_gpu as ti
    from samrs_amd import driver
    sam = _sam(max_images=4, max_prompts=6)
    items = []
    for i, (h, w) in enumerate([(1024, 1024), (600, 800), (517, 803)]):
        polys, labels = synth.make_rboxes(60 + i, 9, h, w)
        cols = ti._colors(9, 60 + i)
        ann = polys.mean(1).astype(np.float32) if prompt == "point" else polys
        items.append(driver.WorkItem(f"t{i}", synth.make_image(60 + i, h, w), ann, labels, (ti._paint_labels(h, w, polys, cols), cols)))

    def collect(**kw):
        pipe = driver.InstancePipeline(sam, 1, prompt=prompt, multimask=prompt != "point", gt=True, batch=2, box_batch=4,
                                       max_boxes=16, rle=True, rle_buffer_mb=16, **kw)
        got = {}

        def sink(results, release):
            for r in results:
                got[r.key] = (r.areas.copy(), r.quality.copy(), r.inter.copy(), r.gt_area.copy(),
                              [r.rle(j) for j in range(len(r.labels))], [r.gt_rle(j) for j in range(len(r.labels))])
            release()
        assert pipe.run(driver.batched(items, 2), sink) == len(items)
        return got

    ref, got = collect(), collect(batch_decode=True)
    for k in ref:
        for a, b in zip(ref[k], got[k]):
            assert (np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b), k


def _tree(d):
    return {os.path.relpath(os.path.join(p, f), d): open(os.path.join(p, f), "rb").read() for p, _, fs in os.walk(d) for f in fs}


def test_generate_cli_batch_decode(tmp_path):
    import test_png_device_gpu as tp
    from samrs_amd import generate
    img_dir, boxes = tp._cli_dataset(tmp_path)
    a, b = tmp_path / "a", tmp_path / "b"
    sa = generate.run(tp._cli_args(img_dir, boxes, a))
    sb = generate.run(tp._cli_args(img_dir, boxes, b, batch_decode=True))
    assert generate.build_parser().parse_args(["--images", "i", "--boxes", "b", "--out", "o", "--batch-decode"]).batch_decode
    assert sa == sb
    ta, tb = _tree(a), _tree(b)
    assert sorted(ta) == sorted(tb) and ta
    for k in ta:
        assert ta[k] == tb[k], k


@pytest.mark.parametrize("prompt", ["box", "rbox_mask"])
def test_instances_cli_batch_decode(tmp_path, prompt):
    import test_instances_gpu as ti
    from samrs_amd import instances
    img_dir, ann_dir, lab_dir, sizes = ti._write_dataset(str(tmp_path))
    ti._paint_dataset_labels(img_dir, ann_dir, lab_dir, sizes)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    ra = instances.main(ti._cli_args(img_dir, ann_dir, lab_dir, a, prompt))
    rb = instances.main(ti._cli_args(img_dir, ann_dir, lab_dir, b, prompt, ["--batch-decode"]))
    assert ra == rb
    ta, tb = _tree(a), _tree(b)
    assert sorted(ta) == sorted(tb) and ta
    for k in ta:
        assert ta[k] == tb[k], k

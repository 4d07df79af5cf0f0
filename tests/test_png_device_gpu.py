"""GPU: the class-map PNG pair encoded on the device (samrs_png_encode_labels / Engine.png_encode) against the host's label-aware
pair writer (tile_io.write_label_pair, libsamrs_io's samrs_io_png_write_label_pair).  The device files must be byte-identical
with the host's, file for file: the same parse, the same Huffman trees, the same bit packing, the same checksums."""
import heapq
import os

import numpy as np
import pytest
import torch

from samrs_amd import tile_io

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import samrs_amd
    sam = samrs_amd.sam_model_registry["vit_tiny"](max_prompts=4, max_points=1).to("cuda")
    return sam.engine


def _host_pair(tmp_path, seg, lut):
    g, c = str(tmp_path / "g.png"), str(tmp_path / "c.png")
    tile_io.write_label_pair(g, c, seg, lut)
    with open(g, "rb") as fg, open(c, "rb") as fc:
        return fg.read(), fc.read()


def _device(eng, maps, lut, cap=None, cursor0=0, out=None, cur=None):
    maps = np.ascontiguousarray(maps if maps.ndim == 3 else maps[None])
    n, h, w = maps.shape
    if out is None:
        cap = cap or int(n * 2 * (h * w * 6 + h * 2 + 8192)) + 4096
        out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    if cur is None:
        cur = torch.full((1,), cursor0, dtype=torch.int64, device="cuda")
    tab = torch.zeros(n, 2, 2, dtype=torch.int64, device="cuda")
    eng.png_encode(torch.from_numpy(maps).cuda(), torch.from_numpy(np.ascontiguousarray(lut)).cuda(), out, cur, tab)
    torch.cuda.synchronize()
    return out, cur, tab.cpu().numpy()


def _files(out, tab):
    o = out.cpu().numpy()
    return [[bytes(o[int(tab[j, k, 0]): int(tab[j, k, 0]) + int(tab[j, k, 1])]) for k in range(2)] for j in range(len(tab))]


def _fib_literals():
    """One row whose every pixel is a literal (no two neighbours equal) and whose label counts are Fibonacci numbers: the plain
    Huffman tree of the literal / length alphabet is deeper than 15 bits, so the encoder must flatten the counts and rebuild."""
    fib = [2, 3]
    while len(fib) < 18:
        fib.append(fib[-1] + fib[-2])
    labels = np.concatenate([np.full(f, i + 1, np.uint8) for i, f in enumerate(fib)])       # labels 1 .. 18, sorted
    row = np.empty_like(labels)
    half = (len(labels) + 1) // 2
    row[0::2], row[1::2] = labels[:half], labels[half:]                                    # max count < half: no equal neighbours
    assert not np.any(row[1:] == row[:-1])
    return row.reshape(1, -1).copy(), fib


def _plain_huffman_depth(counts):
    heap = [(c, i, 0) for i, c in enumerate(counts)]
    heapq.heapify(heap)
    nxt = len(counts)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], nxt, max(a[2], b[2]) + 1))
        nxt += 1
    return heap[0][2]


def _long_runs(rng):
    segs = [1, 2, 3, 85, 86, 87, 172, 173, 257, 258, 259, 300, 517, 1000]
    row = np.concatenate([np.full(n, rng.integers(0, 18), np.uint8) for n in segs])
    seg = np.repeat(row[None], 12, axis=0)
    seg[5] = np.roll(seg[5], 3)
    seg[7, ::97] = 200
    return seg


def _blobs(rng, h, w):
    seg = np.full((h, w), 255, np.uint8)
    for _ in range(40):
        y, x = rng.integers(0, h), rng.integers(0, w)
        r = rng.integers(4, max(5, min(h, w) // 4))
        yy, xx = np.ogrid[:h, :w]
        seg[(yy - y) ** 2 + (xx - x) ** 2 < r * r] = rng.integers(0, 18)
    return seg


def _map(kind, golden_dir):
    rng = np.random.default_rng(11)
    h, w = 256, 384
    if kind == "noise":                      # > 2^20 tokens: two deflate blocks
        return rng.integers(0, 18, (1024, 1100)).astype(np.uint8)
    if kind == "blobs":
        return _blobs(rng, h, w)
    if kind == "constant":
        return np.full((h, w), 255, np.uint8)
    if kind == "one_class":
        return np.full((300, 500), 7, np.uint8)
    if kind == "columns":
        return np.repeat(rng.integers(0, 18, (1, w)).astype(np.uint8), h, axis=0)
    if kind == "rows":
        return np.repeat(rng.integers(0, 18, (h, 1)).astype(np.uint8), w, axis=1)
    if kind == "wide":                       # 12000-pixel rows: no "up" matches in either stream
        return np.repeat(rng.integers(0, 18, (3, 1200)).astype(np.uint8), 10, axis=1)
    if kind == "pairs":                      # nothing but 2-pixel runs: the gray stream's literal path
        return np.repeat(rng.integers(0, 200, (h, w // 2)).astype(np.uint8), 2, axis=1)
    if kind == "long_runs":                  # runs past 258 (one token) and 86 pixels (one colour match)
        return _long_runs(rng)
    if kind == "fixture":
        return np.ascontiguousarray(np.load(os.path.join(golden_dir, "vit_h_c2c4.npz"))["c2_seg"])
    if kind == "fibonacci":
        return _fib_literals()[0]
    hh, ww = (int(v) for v in kind.split("x"))
    seg = _blobs(rng, hh, ww)
    seg[rng.random((hh, ww)) < 0.05] = rng.integers(0, 18)
    return seg


KINDS = ["noise", "blobs", "constant", "one_class", "columns", "rows", "wide", "pairs", "long_runs", "fixture", "fibonacci",
         "1x1", "1x7", "7x1", "753x1166", "800x800"]


@pytest.mark.parametrize("kind", KINDS)
def test_device_pair_is_byte_identical_with_the_host_writer(eng, tmp_path, kind, golden_dir):
    seg = _map(kind, golden_dir)
    lut = tile_io.class_lut(np.random.default_rng(3).integers(0, 256, (200, 3), dtype=np.uint8))
    hg, hc = _host_pair(tmp_path, seg, lut)
    out, cur, tab = _device(eng, seg, lut)
    (dg, dc), = _files(out, tab)
    assert tab[0, 0, 0] == 0 and tab[0, 1, 0] == (len(hg) + 15) // 16 * 16
    assert int(cur.item()) == tab[0, 1, 0] + (len(hc) + 15) // 16 * 16
    assert len(dg) == len(hg) and dg == hg, kind
    assert len(dc) == len(hc) and dc == hc, kind


def test_fibonacci_map_needs_the_length_limit(eng, tmp_path):
    row, fib = _fib_literals()
    # gray literal / length alphabet: labels 1 .. 18 (Fibonacci counts), label 0 once (the filter byte), end-of-block once
    assert _plain_huffman_depth([1, 1] + fib) > 15
    lut = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    hg, hc = _host_pair(tmp_path, row, lut)
    out, _, tab = _device(eng, row, lut)
    assert _files(out, tab) == [[hg, hc]]


def test_one_call_of_eight_maps_equals_eight_calls(eng, golden_dir):
    rng = np.random.default_rng(5)
    maps = [_blobs(rng, 200, 300) for _ in range(4)] + [rng.integers(0, 18, (200, 300)).astype(np.uint8) for _ in range(3)]
    maps.append(np.full((200, 300), 255, np.uint8))
    maps = np.stack(maps)
    lut = tile_io.class_lut(rng.integers(0, 256, (18, 3), dtype=np.uint8))
    out, cur, tab = _device(eng, maps, lut)
    batch = _files(out, tab)
    single = [_files(*_device(eng, maps[j], lut)[::2])[0] for j in range(8)]
    assert batch == single
    offs = tab[:, :, 0].reshape(-1)
    lens = tab[:, :, 1].reshape(-1)
    assert np.all(offs % 16 == 0) and np.all(lens > 0)
    assert np.array_equal(offs[1:], offs[:-1] + (lens[:-1] + 15) // 16 * 16)
    assert int(cur.item()) == offs[-1] + (lens[-1] + 15) // 16 * 16


def test_two_calls_append_behind_the_cursor(eng, tmp_path):
    rng = np.random.default_rng(9)
    a, b = _blobs(rng, 120, 90), rng.integers(0, 5, (64, 64)).astype(np.uint8)
    lut = tile_io.class_lut(rng.integers(0, 256, (18, 3), dtype=np.uint8))
    out = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    cur = torch.full((1,), 37, dtype=torch.int64, device="cuda")
    _, _, ta = _device(eng, a, lut, out=out, cur=cur)
    end_a = int(cur.item())
    _, _, tb = _device(eng, b, lut, out=out, cur=cur)
    assert ta[0, 0, 0] == 48 and tb[0, 0, 0] == end_a
    assert _files(out, ta)[0] == list(_host_pair(tmp_path, a, lut))
    assert _files(out, tb)[0] == list(_host_pair(tmp_path, b, lut))


def test_too_small_buffer_reports_the_size_and_writes_nothing(eng, tmp_path):
    rng = np.random.default_rng(13)
    seg = rng.integers(0, 18, (256, 256)).astype(np.uint8)
    lut = tile_io.class_lut(rng.integers(0, 256, (18, 3), dtype=np.uint8))
    hg, hc = _host_pair(tmp_path, seg, lut)
    out = torch.full((4096,), 0xAB, dtype=torch.uint8, device="cuda")
    out, cur, tab = _device(eng, seg, lut, out=out)
    assert tab[0, 0, 1] == -len(hg) - 1 and tab[0, 1, 1] == -len(hc) - 1
    assert int(cur.item()) == 0
    assert bool((out == 0xAB).all())
    # room for the gray file only: it is written, the colour file is not
    cap = (len(hg) + 15) // 16 * 16 + 16
    out = torch.full((cap,), 0xAB, dtype=torch.uint8, device="cuda")
    out, cur, tab = _device(eng, seg, lut, out=out)
    assert tab[0, 0, 1] == len(hg) and tab[0, 1, 1] == -len(hc) - 1
    assert bytes(out[:len(hg)].cpu().numpy()) == hg and bool((out[(len(hg) + 15) // 16 * 16:] == 0xAB).all())
    assert int(cur.item()) == (len(hg) + 15) // 16 * 16


def test_device_files_decode_to_the_map_and_its_palette(eng, tmp_path):
    rng = np.random.default_rng(17)
    maps = np.stack([_blobs(rng, 160, 224), rng.integers(0, 18, (160, 224)).astype(np.uint8)])
    lut = tile_io.class_lut(rng.integers(0, 256, (18, 3), dtype=np.uint8))
    out, _, tab = _device(eng, maps, lut)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    for j, (g, c) in enumerate(_files(out, tab)):
        pg, pc = str(tmp_path / f"g{j}.png"), str(tmp_path / f"c{j}.png")
        with open(pg, "wb") as f:
            f.write(g)
        with open(pc, "wb") as f:
            f.write(c)
        assert np.array_equal(tile_io.read_rgb(pg)[..., 0], maps[j])
        assert np.array_equal(tile_io.read_rgb(pc), lut[maps[j]])
        if Image is not None:
            assert np.array_equal(np.array(Image.open(pg)), maps[j])
            assert np.array_equal(np.array(Image.open(pc)), lut[maps[j]])


def test_bad_sizes_are_rejected(eng):
    lut = torch.zeros(256, 3, dtype=torch.uint8, device="cuda")
    out = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    cur = torch.zeros(1, dtype=torch.int64, device="cuda")
    tab = torch.zeros(1, 2, 2, dtype=torch.int64, device="cuda")
    with pytest.raises(AssertionError, match="too large"):
        eng.png_encode(torch.zeros(1, 1, 70000, dtype=torch.uint8, device="cuda"), lut, out, cur, tab)


# ---- the pipeline and the CLI ------------------------------------------------------------------------------------------------

def _stream_items(driver, sizes, counts):
    from samrs_amd import synth
    items = []
    for i, ((h, w), n) in enumerate(zip(sizes, counts)):
        img = synth.make_image(40 + i, h, w)
        boxes, labels = synth.make_boxes(40 + i, n, h, w)
        items.append(driver.WorkItem(f"img{i}", img, boxes, labels))
    return items


def test_pipeline_png_files_equal_the_host_encoder(tmp_path):
    """TilePipeline(png_lut=...): every TileResult.png(kind) equals the host encoder's file for that result's own seg_mask, for
    native and odd-sized tiles in one batch; every other field equals a run without png_lut."""
    import samrs_amd
    from samrs_amd import driver
    sam = samrs_amd.sam_model_registry["vit_tiny"](max_images=4, max_prompts=20, precision="f16").to("cuda")
    sizes = [(1024, 1024), (600, 800), (1024, 1024), (517, 803), (1024, 1024)]
    counts = [3, 5, 24, 2, 9]
    items = _stream_items(driver, sizes, counts)
    lut = tile_io.class_lut(np.random.default_rng(1).integers(0, 256, (18, 3), dtype=np.uint8))

    def collect(pipe):
        got = {}

        def sink(results, release):
            for r in results:
                png = (bytes(r.png("gray")), bytes(r.png("color"))) if r.png_table is not None else None
                got[r.key] = (r.seg_mask.copy(), r.areas.copy(), [r.rle(j) for j in range(len(r.labels))], png)
            release()
        assert pipe.run(driver.batched(items, 2), sink) == len(items)
        return got

    plain = collect(driver.TilePipeline(sam, 18, batch=2, box_batch=20, max_boxes=64, rle=True, rle_buffer_mb=16))
    pipe = driver.TilePipeline(sam, 18, batch=2, box_batch=20, max_boxes=64, rle=True, rle_buffer_mb=16, png_lut=lut)
    for rnd in range(2):                                  # a second run through the same pipeline reuses its buffers
        dev = collect(pipe)
        for it in items:
            seg, areas, rles, png = dev[it.key]
            seg0, areas0, rles0, png0 = plain[it.key]
            assert png0 is None and png is not None
            assert np.array_equal(seg, seg0) and np.array_equal(areas, areas0) and rles == rles0
            assert list(png) == list(_host_pair(tmp_path, seg, lut)), f"{it.key} (round {rnd})"
    with pytest.raises(ValueError, match="no device PNG"):
        driver.TileResult("k", plain["img0"][0], plain["img0"][1], None, None).png("gray")
    # a buffer that cannot hold the batch's files fails loudly and names the knob
    small = driver.TilePipeline(sam, 18, batch=2, box_batch=20, max_boxes=64, png_lut=lut, png_buffer_mb=1)
    small.png_dev = [t[:4096] for t in small.png_dev]
    with pytest.raises(RuntimeError, match="png_buffer_mb"):
        small.run(driver.batched(items[:2], 2), lambda res, rel: rel())


def _cli_dataset(root):
    import json
    from samrs_amd import synth
    img_dir = root / "img"
    img_dir.mkdir()
    ann = {}
    for i, (h, w) in enumerate([(1024, 1024), (600, 800), (1024, 1024)]):
        tile_io.write_rgb(str(img_dir / f"P{i:04d}.png"), synth.make_image(70 + i, h, w), 1)
        b, l = synth.make_boxes(70 + i, 23, h, w)
        ann[f"P{i:04d}"] = {"boxes": b.tolist(), "labels": l.tolist()}
    (root / "boxes.json").write_text(json.dumps(ann))
    return img_dir, root / "boxes.json"


def _cli_args(img_dir, boxes, out, **kw):
    from samrs_amd import generate
    a = dict(images=str(img_dir), boxes=str(boxes), out=str(out), model="vit_tiny", checkpoint=None, precision="f16", classes=None,
             n_classes=18, palette=None, box_batch=20, no_rle=False, batch=2)
    a.update(kw)
    return generate.argparse.Namespace(**a)


def _tree(d):
    return {os.path.relpath(os.path.join(p, f), d): open(os.path.join(p, f), "rb").read()
            for p, _, fs in os.walk(d) for f in fs}


def test_cli_png_device_writes_the_same_files(tmp_path):
    """generate with and without --png-device on the same tiles: byte-identical gray/ and color/ trees, equal ins/*.pkl and
    statistic/; a --resume run with the flag re-creates a removed image's files exactly."""
    from samrs_amd import generate
    img_dir, boxes = _cli_dataset(tmp_path)
    host, dev = tmp_path / "host", tmp_path / "dev"
    s_host = generate.run(_cli_args(img_dir, boxes, host))
    s_dev = generate.run(_cli_args(img_dir, boxes, dev, png_device=True))
    assert s_host == s_dev
    th, td = _tree(host), _tree(dev)
    assert sorted(th) == sorted(td) and len([k for k in th if k.startswith("gray")]) == 3
    for k in th:
        assert th[k] == td[k], k
    for sub in ("gray", "color"):
        os.remove(dev / sub / "P0001.png")
    os.remove(dev / "ins" / "P0001.pkl")
    generate.run(_cli_args(img_dir, boxes, dev, png_device=True, resume=True))
    tr = _tree(dev)
    assert sorted(tr) == sorted(th)
    for k in th:                                   # a resumed run lists the old images' mask sizes first: same sizes, other order
        if k.endswith("all_mask_size.npy"):
            assert sorted(np.load(dev / k).tolist()) == sorted(np.load(host / k).tolist())
        else:
            assert tr[k] == th[k], k

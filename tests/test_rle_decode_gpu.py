"""GPU: COCO run-length DEcoding on the device (samrs_rle_decode, the inverse of samrs_rle_encode) against the host restatement
samrs_amd/rle.py:decode.  Byte / integer work: every comparison is exact.  The malformed-string cases pin the validation the
kernels do before any fill: status codes as samrs_hip.h's samrs_rle_status, zero masks, and no byte written outside masks_out."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from samrs_amd import rle

pytestmark = pytest.mark.gpu

OK, ABSENT, RANGE, BAD_CHAR, TRUNCATED, BAD_COUNT, BAD_SUM = range(7)


@pytest.fixture(scope="module")
def eng():
    import samrs_amd
    sam = samrs_amd.sam_model_registry["vit_tiny"](max_prompts=4, max_points=1).to("cuda")
    return sam.engine


def _blobs(rng, h, w, p):
    m = rng.random((h, w)) < p
    if h > 8 and w > 8:
        m[h // 4: h // 2, w // 5: w // 2] = True
        m[h // 3, :] = False
    return m


def _decode(eng, rles, size):
    """(masks, areas, status) as numpy, through pack_strings + Engine.rle_decode"""
    buf, table = rle.pack_strings(rles)
    masks, areas, status = eng.rle_decode(torch.from_numpy(buf).cuda(), torch.from_numpy(table).cuda(), size)
    torch.cuda.synchronize()
    return masks.cpu().numpy(), areas.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("h,w", [(1024, 1024), (600, 800), (517, 803), (37, 91), (1, 1), (33, 1), (1, 70), (32, 64)])
def test_decode_inverts_encode(eng, h, w):
    rng = np.random.default_rng(h * 7 + w)
    masks = [np.zeros((h, w), bool), np.ones((h, w), bool), _blobs(rng, h, w, 0.0), _blobs(rng, h, w, 0.5), _blobs(rng, h, w, 0.02)]
    m = np.zeros((h, w), bool); m[0, 0] = True; masks.append(m)
    m = np.ones((h, w), bool); m[-1, -1] = False; masks.append(m)
    m = (np.add.outer(np.arange(h), np.arange(w)) & 1).astype(bool); masks.append(m)      # checkerboard: one count per pixel
    masks = np.stack(masks)
    rles = [rle.encode(x) for x in masks]
    got, areas, status = _decode(eng, rles, (h, w))
    assert (status == OK).all(), status
    for j in range(len(masks)):
        assert np.array_equal(got[j], masks[j].astype(np.uint8)), f"mask {j} ({h}x{w})"
    assert np.array_equal(areas, masks.reshape(len(masks), -1).sum(1))
    dev = rle.decode_device(eng, rles)
    assert dev.dtype == torch.uint8 and tuple(dev.shape) == masks.shape and np.array_equal(dev.cpu().numpy(), masks.astype(np.uint8))


def test_decode_known_answers(eng, golden_dir):
    vec = json.load(open(os.path.join(golden_dir, "coco_rle_known_answers.json")))["vectors"]
    for v in vec:
        want = rle.decode({"size": v["size"], "counts": v["string"]})
        for counts in (v["string"], v["string"].encode("ascii"), v["counts"]):            # str, bytes, uncompressed list
            got = rle.decode_device(eng, [{"size": v["size"], "counts": counts}]).cpu().numpy()
            assert np.array_equal(got[0], want.astype(np.uint8)), v["name"]


def _padded(head, hw):
    """counts starting with `head`, padded with one more count to sum hw"""
    rest = hw - sum(head)
    assert rest >= 0
    return list(head) + [rest]


def test_decode_hand_built_counts(eng):
    cases = [((5, 7), [0, 35]),                                            # the full mask
             ((4, 4), [3, 0, 2, 5, 6]),                                    # an interior zero
             ((4, 4), [0, 0, 0, 16]),
             ((4, 4), [16, 0, 0]),                                         # trailing zeros
             ((1100, 1000), _padded([0, 5, 0, 3, 1000000, 2, 7, 1, 40000, 3], 1100 * 1000)),   # a long count, then negative deltas
             ((4100, 4100), _padded([0, 5, 0, 3, 16777300, 2, 7, 1, 300, 3], 4100 * 4100)),    # a 6-char count (>= 2^24)
             ((37, 91), _padded([1, 2] * 300 + [0, 0, 5, 0, 1], 37 * 91))]
    for size, counts in cases:
        assert sum(counts) == size[0] * size[1]
        s = rle.counts_to_string(counts)
        assert rle.string_to_counts(s) == counts
        want = rle.decode({"size": list(size), "counts": s})
        got, areas, status = _decode(eng, [{"size": list(size), "counts": s}], size)
        assert status[0] == OK, (size, counts[:8], status)
        assert np.array_equal(got[0], want.astype(np.uint8)), (size, counts[:8])
        assert areas[0] == want.sum()
    assert len(rle.counts_to_string([16777300])) == 6


def test_device_round_trip_without_a_host_step(eng):
    """rle_encode's buffer and table straight into rle_decode: 40 masks (more than one internal pass of 32), the buffer too small
    for the last one, which comes back ABSENT and zero."""
    rng = np.random.default_rng(11)
    b = rng.random((40, 64, 96)) < 0.5
    need = [(len(rle.encode(x)["counts"]) + 15) & ~15 for x in b]
    cap = sum(need[:-1]) + 16                                               # the last string needs more than 16 bytes
    assert need[-1] > 16
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    cur = torch.zeros(1, dtype=torch.int64, device="cuda")
    tab = torch.zeros(40, 3, dtype=torch.int64, device="cuda")
    dev = torch.as_tensor(b).cuda()
    eng.rle_encode(dev, out, cur, tab)
    masks, areas, status = eng.rle_decode(out, tab, (64, 96))
    torch.cuda.synchronize()
    status = status.cpu().numpy()
    assert (status[:-1] == OK).all() and status[-1] == ABSENT, status
    assert torch.equal(masks[:-1], dev[:-1].view(torch.uint8))
    assert int(masks[-1].sum()) == 0 and int(areas[-1]) == 0
    assert torch.equal(areas[:-1], dev[:-1].flatten(1).sum(1))


def test_malformed_strings_are_reported_and_write_nothing_outside(eng):
    h, w = 37, 91
    hw = h * w
    rng = np.random.default_rng(17)
    good = [_blobs(rng, h, w, 0.3), _blobs(rng, h, w, 0.02), (np.add.outer(np.arange(h), np.arange(w)) & 1).astype(bool)]
    gs = [rle.encode(g)["counts"] for g in good]
    c2s = rle.counts_to_string
    eight = "".join(chr(48 + 0x20 + 1) for _ in range(7)) + chr(48 + 1)    # 8 groups in one token
    strings = [
        (gs[0], OK),
        (c2s([10, 20, hw - 40]), BAD_SUM),                                 # sum too small
        (c2s([10, 20, hw - 20]), BAD_SUM),                                 # sum too large
        ("", BAD_SUM),                                                     # the empty string
        (gs[1], OK),
        (gs[1][:-1] + chr(((ord(gs[1][-1]) - 48) | 0x20) + 48), TRUNCATED),    # continuation bit on the last char
        (gs[0][:5] + " " + gs[0][6:], BAD_CHAR),                           # a byte of 0x20
        (c2s([10, 20, 30, 5]) [:-1] + c2s([-25]), BAD_COUNT),              # 4th count = 20 + (-25) < 0
        (eight + c2s([hw]), BAD_COUNT),                                    # an 8-char token
        (gs[2], OK),
    ]
    # ord(last) - 48 with bit 5 set is at most 111: still a legal char, so TRUNCATED is the lowest code that applies
    assert (ord(strings[5][0][-1]) - 48) & 0x20
    assert rle.string_to_counts(strings[7][0])[3] < 0
    rles = [{"size": [h, w], "counts": s} for s, _ in strings]
    buf, table = rle.pack_strings(rles)
    n = len(strings) + 3
    tab = np.zeros((n, 3), np.int64)
    tab[:len(strings)] = table
    tab[len(strings)] = (len(buf) - 8, 16, 0)                               # offset + length past strings_bytes
    tab[len(strings) + 1] = (-16, 8, 0)                                     # offset < 0
    tab[len(strings) + 2] = (0, -100, 0)                                    # the encoder's "did not fit"
    want_status = [st for _, st in strings] + [RANGE, RANGE, ABSENT]
    pad = 4099                                                              # an odd start: masks_out is unaligned
    big = torch.full((pad + n * hw + pad,), 0xAB, dtype=torch.uint8, device="cuda")
    out = big[pad:pad + n * hw].view(n, h, w)
    areas_big = torch.full((n + 2,), -7, dtype=torch.int64, device="cuda")
    status_big = torch.full((n + 2,), -7, dtype=torch.int32, device="cuda")
    masks, areas, status = eng.rle_decode(torch.from_numpy(buf).cuda(), torch.from_numpy(tab).cuda(), (h, w), out=out,
                                          areas_out=areas_big[1:n + 1], status_out=status_big[1:n + 1])
    torch.cuda.synchronize()
    assert status.cpu().tolist() == want_status
    big = big.cpu().numpy()
    assert (big[:pad] == 0xAB).all() and (big[pad + n * hw:] == 0xAB).all()
    assert areas_big[0] == -7 and areas_big[-1] == -7 and status_big[0] == -7 and status_big[-1] == -7
    got = big[pad:pad + n * hw].reshape(n, h, w)
    gi = 0
    for j, st in enumerate(want_status):
        if st == OK:
            assert np.array_equal(got[j], good[gi].astype(np.uint8)) and int(areas[j]) == good[gi].sum(), j
            gi += 1
        else:
            assert not got[j].any() and int(areas[j]) == 0, j
    with pytest.raises(ValueError, match=r"RLE 1 .*BAD_SUM"):
        rle.decode_device(eng, rles[:3])
    with pytest.raises(ValueError, match="mixed sizes"):
        rle.decode_device(eng, [rles[0], {"size": [w, h], "counts": gs[0]}])


def test_arbitrary_bytes_decode_to_a_status_and_nothing_else(eng):
    """random bytes (all 256 values, and random legal chars) as strings: every mask comes back with a status, non-OK ones zero,
    and the bytes around masks_out are untouched"""
    h, w = 33, 65
    rng = np.random.default_rng(23)
    buf = np.concatenate([rng.integers(0, 256, 3000, dtype=np.uint8), rng.integers(48, 112, 3000, dtype=np.uint8),
                          rng.integers(48, 80, 3001, dtype=np.uint8)])
    tab = np.array([[0, 3000, 0], [3000, 3000, 0], [6000, 3001, 0], [1, 8999, 0], [2999, 2, 0], [9000, 1, 0]], np.int64)
    n = len(tab)
    big = torch.full((64 + n * h * w + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    masks, areas, status = eng.rle_decode(torch.from_numpy(buf).cuda(), torch.from_numpy(tab).cuda(), (h, w),
                                          out=big[64:64 + n * h * w].view(n, h, w))
    torch.cuda.synchronize()
    big, status = big.cpu().numpy(), status.cpu().numpy()
    assert (big[:64] == 0xAB).all() and (big[-64:] == 0xAB).all()
    assert ((status >= OK) & (status <= BAD_SUM)).all() and status[0] == BAD_CHAR
    for j in range(n):
        m = big[64 + j * h * w: 64 + (j + 1) * h * w]
        assert m.max() <= 1 and int(areas[j]) == int(m.sum())
        if status[j] != OK:
            assert not m.any()
        else:                                                               # a random string that happens to be valid
            s = buf[tab[j, 0]:tab[j, 0] + tab[j, 1]].tobytes().decode("ascii")
            assert np.array_equal(m.reshape(h, w), rle.decode({"size": [h, w], "counts": s}).astype(np.uint8))


def test_no_masks_is_a_no_op_and_bad_arguments_are_refused(eng):
    empty = torch.zeros(0, dtype=torch.uint8, device="cuda")
    masks, areas, status = eng.rle_decode(empty, torch.zeros(0, 3, dtype=torch.int64, device="cuda"), (5, 5))
    assert tuple(masks.shape) == (0, 5, 5) and areas.numel() == 0 and status.numel() == 0
    assert rle.decode_device(eng, []).shape[0] == 0
    buf, table = rle.pack_strings([{"size": [1, 1], "counts": rle.counts_to_string([1])}])
    s, t = torch.from_numpy(buf).cuda(), torch.from_numpy(table).cuda()
    o = torch.full((4,), 0xAB, dtype=torch.uint8, device="cuda")
    st = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    lib, hnd, vp = eng.lib, eng.handle, ctypes.c_void_p
    BAD_ARG = -3
    assert lib.samrs_rle_decode(hnd, s.data_ptr(), s.numel(), t.data_ptr(), 1, 1 << 15, 1 << 15, o.data_ptr(), None, st.data_ptr(), None) == BAD_ARG
    assert lib.samrs_rle_decode(hnd, s.data_ptr(), s.numel(), t.data_ptr(), 1, 0, 1, o.data_ptr(), None, st.data_ptr(), None) == BAD_ARG
    assert lib.samrs_rle_decode(hnd, s.data_ptr(), s.numel(), t.data_ptr(), -1, 1, 1, o.data_ptr(), None, st.data_ptr(), None) == BAD_ARG
    assert lib.samrs_rle_decode(hnd, None, s.numel(), t.data_ptr(), 1, 1, 1, o.data_ptr(), None, st.data_ptr(), None) == BAD_ARG
    assert lib.samrs_rle_decode(hnd, s.data_ptr(), s.numel(), None, 1, 1, 1, o.data_ptr(), None, st.data_ptr(), None) == BAD_ARG
    assert lib.samrs_rle_decode(hnd, s.data_ptr(), s.numel(), t.data_ptr(), 1, 1, 1, None, None, st.data_ptr(), None) == BAD_ARG
    assert lib.samrs_rle_decode(hnd, s.data_ptr(), s.numel(), t.data_ptr(), 1, 1, 1, o.data_ptr(), None, None, None) == BAD_ARG
    assert lib.samrs_rle_decode(None, s.data_ptr(), s.numel(), t.data_ptr(), 1, 1, 1, o.data_ptr(), None, st.data_ptr(), None) == BAD_ARG
    torch.cuda.synchronize()
    assert (o.cpu().numpy() == 0xAB).all() and int(st[0]) == -7             # nothing was launched
    assert lib.samrs_rle_decode(hnd, s.data_ptr(), s.numel(), t.data_ptr(), 0, 1, 1, None, None, None, None) == 0
    assert lib.samrs_rle_decode(hnd, s.data_ptr(), s.numel(), t.data_ptr(), 1, 1, 1, o.data_ptr(), None, st.data_ptr(),
                                vp(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    assert o.cpu().tolist() == [0, 0xAB, 0xAB, 0xAB] and int(st[0]) == OK   # counts [1]: one unset pixel


def test_evaluate_files_matches_host_decoded_masks(eng, tmp_path):
    from samrs_amd import coco_ap
    rng = np.random.default_rng(29)
    h, w = 96, 128
    images, anns, dts = [], [], []
    for i in range(3):
        images.append({"id": i + 1, "height": h, "width": w, "file_name": f"{i}.png"})
        for k in range(4):
            g = np.zeros((h, w), bool)
            y, x = int(rng.integers(0, h - 40)), int(rng.integers(0, w - 40))
            g[y:y + int(rng.integers(8, 40)), x:x + int(rng.integers(8, 40))] = True
            anns.append({"id": len(anns) + 1, "image_id": i + 1, "category_id": 1, "iscrowd": 0, "area": int(g.sum()),
                         "segmentation": rle.encode(g)})
            d = g.copy()
            d[rng.random((h, w)) < 0.1 * k] = False
            d |= np.roll(g, 3 * k, axis=1) & (rng.random((h, w)) < 0.5)
            if i == 2 and k == 3:
                continue                                                    # a missed ground truth
            dts.append({"image_id": i + 1, "category_id": 1, "score": float(rng.random()), "segmentation": rle.encode(d)})
    dt_path, gt_path = str(tmp_path / "dt.json"), str(tmp_path / "gt.json")
    json.dump(dts, open(dt_path, "w"))
    json.dump({"images": images, "annotations": anns, "categories": [{"id": 1, "name": "x"}]}, open(gt_path, "w"))
    numbers, tables = coco_ap.evaluate_files(eng, dt_path, gt_path)
    ids, by_dt, by_gt = coco_ap.load_coco_files(dt_path, gt_path)
    host = [(np.stack([rle.decode(s) for _, s in by_dt[i]]), np.array([sc for sc, _ in by_dt[i]], np.float32),
             np.stack([rle.decode(s) for s in by_gt[i]])) for i in ids]
    want_numbers, want_tables = coco_ap.evaluate_masks(eng, host)
    assert len(numbers) == 12 and numbers == want_numbers
    assert len(tables) == len(want_tables)
    for a, b in zip(tables, want_tables):
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k

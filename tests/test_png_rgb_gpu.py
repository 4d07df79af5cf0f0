"""GPU: samrs_png_encode_rgb / Engine.png_encode_rgb.  The yardsticks are two decoders that did not write the files: Pillow (checks
every CRC, the zlib stream and its Adler-32) and libsamrs_io's samrs_io_png_decode_rgb.  Both must return the input pixels exactly."""
import heapq
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlay_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

FILTERS = [-1, 0, 1, 2, 3, 4]


@pytest.fixture(scope="module")
def eng():
    import samrs_amd
    sam = samrs_amd.sam_model_registry["vit_tiny"](max_prompts=4, max_points=1).to("cuda")
    return sam.engine


def _encode(eng, imgs, filt, cap=None, out=None, cur=None):
    """imgs: uint8 [n, h, w, 3] or [h, w, 3] (numpy or a device tensor) -> (out, cursor, table on the host)."""
    from samrs_amd import engine
    x = imgs if isinstance(imgs, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    x = x.reshape(-1, *x.shape[-3:])
    n, h, w, _ = x.shape
    if out is None:
        out = torch.zeros(cap or n * engine.png_rgb_bound(h, w) + 64, dtype=torch.uint8, device="cuda")
    if cur is None:
        cur = torch.zeros(1, dtype=torch.int64, device="cuda")
    tab = torch.zeros(n, 2, dtype=torch.int64, device="cuda")
    eng.png_encode_rgb(x, out, cur, tab, filt)
    torch.cuda.synchronize()
    return out, cur, tab.cpu().numpy()


def _files(out, tab):
    o = out.cpu().numpy()
    return [bytes(o[int(t[0]): int(t[0]) + int(t[1])]) for t in tab]


def _check_decodes(data, img):
    assert np.array_equal(ref.decode_pillow(data), img)
    assert np.array_equal(ref.decode_native(data), img)


def _content(kind, h, w, eng=None):
    rng = np.random.default_rng(h * 7919 + w)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "constant":
        return np.ascontiguousarray(np.broadcast_to(np.array([17, 17, 17], np.uint8), (h, w, 3)))
    if kind == "hgrad":
        return np.ascontiguousarray(np.broadcast_to(((np.arange(w) * 3) % 256).astype(np.uint8)[None, :, None], (h, w, 3)))
    if kind == "vgrad":
        return np.ascontiguousarray(np.broadcast_to(((np.arange(h) * 5) % 256).astype(np.uint8)[:, None, None], (h, w, 3)))
    assert kind == "overlay"
    yy, xx = np.mgrid[:h, :w]
    image = np.stack([(xx * 2 + yy) % 256, (yy * 3) % 256, (xx ^ yy) % 256], axis=-1).astype(np.uint8)
    image = (image.astype(np.int32) + rng.integers(-6, 7, image.shape)).clip(0, 255).astype(np.uint8)
    seg = np.full((h, w), 255, np.uint8)
    seg[h // 4: h // 4 * 3 + 1, w // 3: w // 3 * 2 + 1] = 3
    seg[: h // 3 + 1, : w // 4 + 1] = 11
    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    out = eng.blend_labels(torch.from_numpy(image).cuda(), torch.from_numpy(seg).cuda(), torch.from_numpy(lut).cuda(), 0.4)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("hw", [(1, 1), (1, 5), (7, 1), (64, 64), (517, 803)])
def test_every_content_decodes_to_its_pixels(eng, hw, filt):
    h, w = hw
    imgs = np.stack([_content(k, h, w, eng) for k in ("noise", "constant", "hgrad", "vgrad", "overlay")])
    out, cur, tab = _encode(eng, imgs, filt)
    assert np.all(tab[:, 1] > 0) and np.all(tab[:, 0] % 16 == 0)
    for data, img in zip(_files(out, tab), imgs):
        assert data[25] == 2 and data[24] == 8 and data[28] == 0               # colour type 2, 8 bits, not interlaced
        assert data.count(b"IDAT") == 1 and data[41:43] == b"\x78\x9c"
        _check_decodes(data, img)
        if filt >= 0:
            assert np.all(ref.filter_bytes_of(data) == filt)


def test_two_deflate_blocks_and_one_byte(eng):
    """The smallest image whose filtered bytes are two deflate blocks and one byte: (3 w + 1) h = 2 B + 1."""
    from samrs_amd import engine
    B = engine.PNG_RGB_BLOCK_BYTES
    target = 2 * B + 1
    best = None
    for w in range(1, 70000):                        # the smallest image (fewest pixels) with exactly that many filtered bytes
        L = 3 * w + 1
        if target % L == 0 and target // L <= 65536:
            h = target // L
            if best is None or h * w < best[0] * best[1]:
                best = (h, w)
    h, w = best
    assert (3 * w + 1) * h == target
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img[h // 2:] //= 8                                # the blocks get different codes
    out, _, tab = _encode(eng, img, 1)
    data, = _files(out, tab)
    _check_decodes(data, img)


def _plain_huffman_depth(counts):
    heap = [(c, i, 0) for i, c in enumerate(counts)]
    heapq.heapify(heap)
    nxt = len(counts)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], nxt, max(a[2], b[2]) + 1))
        nxt += 1
    return heap[0][2]


def _fibonacci_image(first, side):
    """uint8 [side, side, 3] whose filter-0 stream (the pixels' bytes and one zero per row) holds 24 byte values with the counts
    F(first) .. F(first + 23), shuffled; the few bytes left over join the most frequent value.  Value 0 carries the first count
    that is >= side, the number of filter bytes."""
    fib = [1, 1]
    while len(fib) < first + 23:
        fib.append(fib[-1] + fib[-2])
    fib = fib[first - 1:]
    h = w = side
    k = next(i for i, f in enumerate(fib) if f >= h)
    values = list(range(1, 25))
    values[k] = 0
    per_value = {v: f for v, f in zip(values, fib)}
    per_value[0] -= h
    n = 3 * h * w
    assert sum(per_value.values()) <= n
    per_value[24] += n - sum(per_value.values())
    vals = np.concatenate([np.full(c, v, np.uint8) for v, c in per_value.items()])
    np.random.default_rng(8).shuffle(vals)
    return vals.reshape(h, w, 3), fib


@pytest.mark.parametrize("first,side,deep", [(1, 202, False), (2, 256, True)])
def test_fibonacci_counts_and_the_length_limit(eng, first, side, deep):
    """Byte values with Fibonacci counts under filter 0.  F(1) .. F(24) (121 392 bytes in 202 x 202): the end-of-block symbol's
    count of 1 stands beside F(1) = F(2) = 1, and under the (weight, node index) order the plain Huffman tree then grows as two
    interleaved chains, 13 deep -- that image decodes exactly but does not reach the limit.  F(2) .. F(25) (196 416 bytes in
    256 x 256), where the end-of-block symbol takes F(1)'s place, gives the single chain: an unlimited code is 24 bits deep and the
    encoder has to flatten the counts and rebuild."""
    img, fib = _fibonacci_image(first, side)
    counts = np.bincount(img.reshape(-1), minlength=256)
    counts[0] += side                                 # the rows' filter bytes
    assert sorted(counts[counts > 0].tolist())[:-1] == fib[:-1]
    depth = _plain_huffman_depth(counts[counts > 0].tolist() + [1])          # + the end-of-block symbol
    assert (depth > 15) == deep, depth
    out, _, tab = _encode(eng, img, 0)
    data, = _files(out, tab)
    _check_decodes(data, img)


@pytest.mark.parametrize("filt", [0, -1])
def test_noise_stays_under_the_documented_bound(eng, filt):
    from samrs_amd import engine
    h, w = 300, 411
    img = np.random.default_rng(6).integers(0, 256, (h, w, 3), dtype=np.uint8)
    out, _, tab = _encode(eng, img, filt, cap=4 * h * w * 3)
    n = (3 * w + 1) * h
    blocks = -(-n // engine.PNG_RGB_BLOCK_BYTES)
    bound = 63 + -(-(9 * n + blocks * (4498 + 9)) // 8)                       # samrs_hip.h
    assert 0 < tab[0, 1] <= bound
    assert engine.png_rgb_bound(h, w) == (bound + 15) // 16 * 16
    _check_decodes(_files(out, tab)[0], img)


def test_one_call_of_eight_images_equals_eight_calls(eng):
    rng = np.random.default_rng(5)
    h, w = 90, 130
    imgs = np.stack([_content(k, h, w, eng) for k in ("noise", "constant", "hgrad", "vgrad", "overlay")]
                    + [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(3)])
    out, cur, tab = _encode(eng, imgs, -1)
    batch = _files(out, tab)
    single = [_files(*_encode(eng, imgs[j], -1)[::2])[0] for j in range(8)]
    assert batch == single
    offs, lens = tab[:, 0], tab[:, 1]
    assert np.all(offs % 16 == 0) and np.all(lens > 0) and offs[0] == 0
    assert np.array_equal(offs[1:], offs[:-1] + (lens[:-1] + 15) // 16 * 16)
    assert int(cur.item()) == offs[-1] + (lens[-1] + 15) // 16 * 16
    # more than one pass of eight, and the same input again: the same bytes
    twelve = np.concatenate([imgs, imgs[:4]])
    o2, _, t2 = _encode(eng, twelve, -1)
    assert _files(o2, t2) == batch + batch[:4]
    o3, _, t3 = _encode(eng, imgs, -1)
    assert _files(o3, t3) == batch and np.array_equal(t3, tab)


def test_two_calls_append_behind_the_cursor(eng):
    rng = np.random.default_rng(9)
    a, b = rng.integers(0, 256, (40, 30, 3), dtype=np.uint8), _content("hgrad", 64, 64)
    out = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    cur = torch.full((1,), 37, dtype=torch.int64, device="cuda")
    _, _, ta = _encode(eng, a, -1, out=out, cur=cur)
    end_a = int(cur.item())
    _, _, tb = _encode(eng, b, -1, out=out, cur=cur)
    assert ta[0, 0] == 48 and end_a == 48 + (ta[0, 1] + 15) // 16 * 16 and tb[0, 0] == end_a
    _check_decodes(_files(out, ta)[0], a)
    _check_decodes(_files(out, tb)[0], b)


def test_too_small_buffer_reports_the_size_and_writes_nothing(eng):
    rng = np.random.default_rng(13)
    imgs = rng.integers(0, 256, (2, 64, 64, 3), dtype=np.uint8)
    imgs[0] //= 64                                    # a small file, then a large one
    _, _, full = _encode(eng, imgs, 0)
    l0, l1 = int(full[0, 1]), int(full[1, 1])
    out = torch.full((32,), 0xAB, dtype=torch.uint8, device="cuda")
    out, cur, tab = _encode(eng, imgs, 0, out=out)
    assert tab[0, 1] == -l0 - 1 and tab[1, 1] == -l1 - 1 and int(cur.item()) == 0
    assert bool((out == 0xAB).all())
    cap = (l0 + 15) // 16 * 16 + 16                   # room for the first file only
    out = torch.full((cap,), 0xAB, dtype=torch.uint8, device="cuda")
    out, cur, tab = _encode(eng, imgs, 0, out=out)
    assert tab[0, 1] == l0 and tab[1, 1] == -l1 - 1
    assert int(cur.item()) == (l0 + 15) // 16 * 16
    assert bool((out[(l0 + 15) // 16 * 16:] == 0xAB).all())
    _check_decodes(bytes(out[:l0].cpu().numpy()), imgs[0])


def test_adaptive_choice_is_the_minimum_sum_rule(eng):
    img = np.random.default_rng(21).integers(0, 256, (33, 67, 3), dtype=np.uint8)
    img[5] = img[4]                                   # "up" costs 0 there
    img[9] = 0                                        # every filter costs 0: the tie goes to filter 0
    img[12, :, :] = img[12, :1, :]                    # "sub" costs next to nothing
    out, _, tab = _encode(eng, img, -1)
    data, = _files(out, tab)
    want = ref.adaptive_filters(img)
    assert want[5] == 2 and want[9] == 0 and len(set(want.tolist())) >= 3
    assert np.array_equal(ref.filter_bytes_of(data), want)
    _check_decodes(data, img)


def test_bad_arguments_are_refused(eng):
    out = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    cur = torch.zeros(1, dtype=torch.int64, device="cuda")
    tab = torch.zeros(1, 2, dtype=torch.int64, device="cuda")
    img = torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device="cuda")
    for filt in (-2, 5):
        with pytest.raises(AssertionError):
            eng.png_encode_rgb(img, out, cur, tab, filt)
    with pytest.raises(AssertionError, match="too large"):
        eng.png_encode_rgb(torch.zeros(1, 1, 70000, 3, dtype=torch.uint8, device="cuda"), out, cur, tab)

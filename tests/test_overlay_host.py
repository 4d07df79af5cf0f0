"""No GPU: the overlay contract as far as it can be seen from the host -- Pillow's blend equals the float32 two-rounding formula the
kernel states, the CLI's and the pipelines' validation of the --vis options, the C ABI declarations and their ctypes binding."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlay_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("alpha", [0.4, 0.0, 1.0, 1 / 3, 0.999, 0.3, 0.5, 0.7])
def test_pillow_blend_is_the_float32_two_rounding_formula(alpha):
    """All 256 x 256 byte pairs: (uint8)(a + alpha * (b - a)) with the product and the sum each rounded to float32, truncated."""
    i = np.arange(256, dtype=np.uint8)
    image = np.ascontiguousarray(np.broadcast_to(i[:, None, None], (256, 256, 3)))
    seg = np.ascontiguousarray(np.broadcast_to(i[None, :], (256, 256)))
    lut = np.ascontiguousarray(np.repeat(i[:, None], 3, axis=1))
    got = ref.overlay_ref(image, seg, lut, alpha)
    assert got.dtype == np.uint8 and got.shape == (256, 256, 3)
    assert np.array_equal(got, ref.blend_f32(image, lut[seg], alpha))


def test_filter_restatement_round_trips_through_two_decoders():
    """tests/overlay_ref.py's numpy filters, put through zlib and framed by hand, decode to the pixels: the restatement the GPU
    test holds the encoder's adaptive choice to is a correct statement of the five PNG filters."""
    import struct
    import zlib
    img = np.random.default_rng(3).integers(0, 256, (9, 11, 3), dtype=np.uint8)
    img[4] = img[3]
    f, ft = ref.filter_rows(img), ref.adaptive_filters(img)
    assert ft[4] == 2
    for choice in (ft, np.arange(9) % 5):
        raw = b"".join(bytes([int(choice[y])]) + f[choice[y], y].tobytes() for y in range(9))

        def chunk(tag, data):
            return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data))
        png = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", 11, 9, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw))
               + chunk(b"IEND", b""))
        assert np.array_equal(ref.decode_pillow(png), img) and np.array_equal(ref.decode_native(png), img)
        assert np.array_equal(ref.filter_bytes_of(png), choice)


def test_cli_refuses_vis_with_scene_window_and_bad_alpha(capsys):
    from samrs_amd import generate
    base = ["--images", "i", "--boxes", "b", "--out", "o"]
    ap = generate.build_parser()
    ns = ap.parse_args(base + ["--vis"])
    assert ns.vis and ns.vis_alpha == 0.4 and ns.vis_palette is None
    assert not ap.parse_args(base).vis
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--vis", "--scene-window", "512"])
    assert "--vis does not apply with --scene-window" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--vis", "--vis-alpha", "1.5"])
    assert "--vis-alpha" in capsys.readouterr().err
    for line in ("always a png", "vis/<stem>.png"):
        assert line in re.sub(r"\s+", " ", ap.format_help()).lower()


def test_vis_options_of_a_namespace():
    """run() is also called with a hand-made namespace (the tests, the benches): the same rules hold there."""
    import argparse
    from samrs_amd import generate, tile_io
    pal = np.arange(54, dtype=np.uint8).reshape(18, 3)
    assert generate.vis_options(argparse.Namespace(), pal) == (None, 0.4)
    lut, alpha = generate.vis_options(argparse.Namespace(vis=True), pal)
    assert alpha == 0.4 and np.array_equal(lut, tile_io.class_lut(pal)) and lut[255].tolist() == [255, 255, 255]
    with pytest.raises(ValueError, match="scene-window"):
        generate.vis_options(argparse.Namespace(vis=True, scene_window=512), pal)
    with pytest.raises(ValueError, match="vis-alpha"):
        generate.vis_options(argparse.Namespace(vis=True, vis_alpha=1.5), pal)


def test_vis_palette_replaces_the_overlay_colours(tmp_path):
    import argparse
    from samrs_amd import generate
    other = (np.arange(54, dtype=np.uint8).reshape(18, 3) * 3)
    np.save(tmp_path / "p.npy", other)
    lut, _ = generate.vis_options(argparse.Namespace(vis=True, vis_palette=str(tmp_path / "p.npy")), np.zeros((18, 3), np.uint8))
    assert np.array_equal(lut[:18], other) and lut[18:].min() == 255


def test_resume_asks_for_the_vis_file_only_under_vis(tmp_path):
    from samrs_amd import generate
    for sub, ext in (("gray", ".png"), ("color", ".png"), ("ins", ".pkl")):
        (tmp_path / sub).mkdir()
        (tmp_path / sub / ("a" + ext)).write_bytes(b"x")
    assert generate.outputs_exist(str(tmp_path), "a")
    assert not generate.outputs_exist(str(tmp_path), "a", vis=True)
    (tmp_path / "vis").mkdir()
    (tmp_path / "vis" / "a.png").write_bytes(b"x")
    assert generate.outputs_exist(str(tmp_path), "a", vis=True)
    os.remove(tmp_path / "gray" / "a.png")
    assert not generate.outputs_exist(str(tmp_path), "a", vis=True)


def test_tile_result_png_vis_raises_without_the_option():
    from samrs_amd import driver
    r = driver.TileResult("k", np.zeros((2, 2), np.uint8), np.zeros(0, np.int64), None, None)
    with pytest.raises(ValueError, match="without vis_lut"):
        r.png("vis")
    r.vis_table, r.vis_data = np.array([16, 3]), np.arange(32, dtype=np.uint8)
    assert bytes(r.png("vis")) == bytes([16, 17, 18])


def test_pipeline_options_are_validated_without_a_device():
    from samrs_amd import driver, scene
    lut = np.zeros((256, 3), np.uint8)
    assert driver.validate_vis_options(None) == (None, 0.4)
    got, alpha = driver.validate_vis_options(lut.tolist(), 0.25)
    assert got.dtype == np.uint8 and got.shape == (256, 3) and alpha == 0.25
    with pytest.raises(ValueError, match="vis_lut must be"):
        driver.validate_vis_options(np.zeros((18, 3), np.uint8))
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="vis_alpha"):
            driver.validate_vis_options(lut, bad)
    with pytest.raises(ValueError, match="vis_buffer_mb"):
        driver.validate_vis_options(lut, 0.4, 0)
    with pytest.raises(ValueError, match="InstancePipeline writes no overlays.*vis_lut is a TilePipeline option"):
        driver.InstancePipeline(None, 18, vis_lut=lut)
    with pytest.raises(ValueError, match="ScenePipeline writes no overlays.*vis_lut is a TilePipeline option"):
        scene.ScenePipeline(None, 18, vis_lut=lut)


def test_documented_bound_and_block_size():
    from samrs_amd import engine
    text = open(os.path.join(ROOT, "include", "samrs_hip.h")).read()
    assert int(re.search(r"#define SAMRS_PNG_RGB_BLOCK_BYTES (\d+)", text).group(1)) == engine.PNG_RGB_BLOCK_BYTES
    n = (3 * 1024 + 1) * 1024
    assert engine.png_rgb_bound(1024, 1024) == (63 + -(-(9 * n + 4 * 4507) // 8) + 15) // 16 * 16
    assert engine.png_rgb_bound(1, 1) == (63 + -(-(9 * 4 + 4507) // 8) + 15) // 16 * 16


def test_header_declares_the_entry_points_and_the_binding_matches():
    import __graft_entry__ as ge
    ge.build_library()
    from samrs_amd import engine
    lib = engine.load_library()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "samrs_hip.h")).read(), flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(samrs_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}
    for name in ("samrs_blend_labels", "samrs_png_encode_rgb"):
        assert name in protos and hasattr(lib, name)
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(protos[name].split(",")), name
    import ctypes
    assert lib.samrs_blend_labels.argtypes[4] is ctypes.c_float
    assert lib.samrs_png_encode_rgb.argtypes[7] is ctypes.c_int64

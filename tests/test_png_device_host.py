"""CPU: the host side of --png-device (the PNG files are encoded on the device, tests/test_png_device_gpu.py): write_outputs writes
the given bytes as they are, atomically, with the pickle last; the flag parses; the host-budget warning and the thread split use
the device path's cost per image."""
import os
import pickle

import numpy as np

from samrs_amd import generate


def test_write_outputs_writes_the_given_png_bytes_via_tmp_and_rename_pickle_last(tmp_path, monkeypatch):
    gray, color = b"\x89PNG gray bytes" * 7, memoryview(b"\x89PNG colour bytes" * 11)
    order = []
    real_replace = os.replace

    def replace(src, dst):
        assert ".tmp." in os.path.basename(src) and not os.path.exists(dst)
        order.append(os.path.relpath(dst, tmp_path))
        real_replace(src, dst)
    monkeypatch.setattr(generate.os, "replace", replace)
    seg = np.zeros((4, 4), np.uint8)                      # not encoded: the files come as bytes
    boxes, labels, areas = np.zeros((2, 4), np.float32), np.array([1, 3]), np.array([5, 0])
    generate.write_outputs(str(tmp_path), "T0", seg, None, boxes, labels, areas, generate.default_palette(18),
                           [str(i) for i in range(18)], rles=[{"size": [4, 4], "counts": "0"}] * 2, png_files=(gray, color))
    assert order == [os.path.join("gray", "T0.png"), os.path.join("color", "T0.png"), os.path.join("ins", "T0.pkl")]
    assert open(tmp_path / "gray" / "T0.png", "rb").read() == gray
    assert open(tmp_path / "color" / "T0.png", "rb").read() == bytes(color)
    info = pickle.load(open(tmp_path / "ins" / "T0.pkl", "rb"))
    assert [d["label"] for d in info] == [1, 3] and [d["size"] for d in info] == [5, 0]
    assert not [f for _, _, fs in os.walk(tmp_path) for f in fs if ".tmp." in f]


def test_png_device_flag_parses():
    ap = generate.build_parser()
    base = ["--images", "i", "--boxes", "b.json", "--out", "o"]
    a = ap.parse_args(base)
    assert a.png_device is False and a.png_buffer_mb is None
    a = ap.parse_args(base + ["--png-device", "--png-buffer-mb", "96"])
    assert a.png_device is True and a.png_buffer_mb == 96


def test_host_budget_uses_the_device_path_cost(monkeypatch):
    assert generate.HOST_MS_PER_IMAGE_PNG_DEVICE < generate.HOST_MS_PER_IMAGE
    monkeypatch.setattr(generate, "host_cpu_budget", lambda local_world=None: 2.0)
    host = generate.host_bound_warning(2, 2, gpu_images_per_s=400.0)
    dev = generate.host_bound_warning(2, 2, gpu_images_per_s=400.0, png_device=True)
    assert f"{generate.HOST_MS_PER_IMAGE:.1f} ms" in host
    assert f"{generate.HOST_MS_PER_IMAGE_PNG_DEVICE:.1f} ms" in dev
    # a rate the device path's budget covers and the host path's does not
    rate = 0.9 * 2.0 / (generate.HOST_MS_PER_IMAGE_PNG_DEVICE * 1e-3)
    assert generate.host_bound_warning(1, 1, gpu_images_per_s=rate) is not None
    assert generate.host_bound_warning(1, 1, gpu_images_per_s=rate, png_device=True) is None
    # the thread split: with the PNG work on the device, decode is the larger share of what is left on the host
    monkeypatch.setattr(generate, "host_cpu_budget", lambda local_world=None: 16.0)
    assert generate.io_threads() == (5, 11)
    r, w = generate.io_threads(png_device=True)
    assert r + w == 16 and r > 5

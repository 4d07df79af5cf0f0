"""CPU, world_size 2, gloo: the downstream consumer check (SURVEY.md 8f N4 / BASELINE.json configs[4]) -- files written by the
generation driver's writers (samrs_amd.generate.write_outputs: gray/*.png, color/*.png, ins/*.pkl) go through the reference's
training read path (oracle/consumer_check.py: datasets.py:185-273, DistributedSampler, CrossEntropyLoss(ignore_index=255)) under
DDP.  The GPU suite runs the same consumer on real `generate.run` output (tests/test_parity_gpu.py::test_generation_driver_end_to_end)."""
import os
import socket

import numpy as np
import torch
import torch.multiprocessing as mp

from samrs_amd import generate, tile_io

from oracle import consumer_check as _cc

N_CLASSES, N_IMAGES, SIDE = _cc.SAMPLE_CLASSES, _cc.SAMPLE_IMAGES, _cc.SAMPLE_SIDE
_make_dataset = _cc.make_sample_dataset


def test_generated_labels_train_under_ddp(tmp_path):
    root = str(tmp_path)
    _make_dataset(root)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_cc.ddp_worker, args=(2, port, root, out), nprocs=2, join=True)
    (l0, w0, d0, h0), (l1, w1, d1, h1) = out[0], out[1]
    assert sorted(d0 + d1) == [0, 1, 2, 3]                          # the sampler's shards partition the train list
    assert all(np.isfinite(l0 + l1)) and l0[1] < l0[0] + 1.0
    assert np.allclose(w0, w1)                                      # DDP: both ranks hold the same weights after the steps
    hist = h0 + h1
    assert hist[N_CLASSES:255].sum() == 0 and hist[255] > 0 and hist[:N_CLASSES].sum() > 0   # class ids or the ignore label, nothing else
    # the serial loop (world 1) sees the same files and the same label values
    from oracle import consumer_check as cc
    ds = cc.SegmentationDataset(root, os.path.join(root, "images"), os.path.join(root, "hbox_segs_init", "gray"), flag="tes")
    assert len(ds) == 2
    x, y = ds[0]
    assert x.shape == (3, SIDE, SIDE) and y.shape == (SIDE, SIDE) and y.dtype == torch.uint8
    # a label map that breaks the contract is refused by the consumer (16-bit / colour / wrong size)
    tile_io.write_rgb(os.path.join(root, "hbox_segs_init", "gray", "P0004.png"), np.zeros((SIDE, SIDE, 3), np.uint8))
    try:
        ds[0]
        raise AssertionError("an RGB label map must be refused")
    except ValueError:
        pass


def test_restated_reader_equals_the_reference_dataset_fixture(tmp_path):
    """Round 6: the reader of oracle/consumer_check.py is pinned to the reference's OWN SegmentationDataset --
    tests/golden/consumer_ref.npz holds what `Pretraining and Finetuning/End_to_End/datasets.py:182-273` (imported in the authoring
    container by oracle/ref_import.import_reference_consumer) returned for every item of the sample dataset the product's writers
    produce: file lists per flag (train.txt / valid.txt, the val[-500:] rule), image tensors and label tensors.  The restated
    reader must build the same lists and return the same tensors from freshly written files (the writers are deterministic)."""
    root = str(tmp_path)
    _make_dataset(root)
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "consumer_ref.npz"))
    for flag in ("trn", "val", "tes"):
        ds = _cc.SegmentationDataset(root, os.path.join(root, "images"), os.path.join(root, "hbox_segs_init", "gray"), flag=flag)
        assert [os.path.relpath(f, root) for f in ds.files] == list(gold[f"{flag}_files"])
        assert [os.path.relpath(f, root) for f in ds.targets] == list(gold[f"{flag}_targets"])
        for i in range(len(ds)):
            x, y = ds[i]
            assert np.array_equal(y.numpy(), gold[f"{flag}_y"][i])                      # labels: bit for bit
            assert np.allclose(x.numpy(), gold[f"{flag}_x"][i], rtol=0, atol=1e-6)      # images: fp32 (x / 255 - mean) / std


def test_reference_dataset_class_trains_on_generated_files_under_ddp(tmp_path):
    """Two DDP-gloo iterations over the files the product's writers wrote must retrace the run of the REFERENCE's own
    SegmentationDataset class: tests/golden/consumer_ref_ddp.npz holds what `train_steps` returned per rank with that class
    (imported in the authoring container by oracle/ref_import.import_reference_consumer; `python -m oracle.consumer_check --ddp`):
    the drawn indices, the label histogram, the losses and the weights after the steps.  The restated reader (pinned item by item
    to the same class by test_restated_reader_equals_the_reference_dataset_fixture) replays it here.  (UperNet-ViT-B needs
    mmseg / mmengine / timm, which cannot be installed: the model stays the one-layer stand-in.)"""
    root = str(tmp_path)
    _make_dataset(root)
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "consumer_ref_ddp.npz"))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_cc.ddp_worker, args=(2, port, root, out), nprocs=2, join=True)
    (l0, w0, d0, h0), (l1, w1, d1, h1) = out[0], out[1]
    assert sorted(d0 + d1) == [0, 1, 2, 3] and all(np.isfinite(l0 + l1)) and np.allclose(w0, w1)
    hist = h0 + h1
    assert hist[N_CLASSES:255].sum() == 0 and hist[255] > 0 and hist[:N_CLASSES].sum() > 0
    for r, (losses, w, drawn, h) in enumerate([out[0], out[1]]):
        assert list(drawn) == gold[f"rank{r}_drawn"].tolist()
        assert np.array_equal(h, gold[f"rank{r}_hist"])
        assert np.allclose(losses, gold[f"rank{r}_losses"], rtol=1e-5, atol=0)
        assert np.allclose(w, gold[f"rank{r}_w"], rtol=1e-5, atol=1e-6)

"""CPU: the host side of samrs_predict_multi / Sam.forward -- the exported symbol and its argtypes, the prompt-signature
grouping, and the argument checks that run before anything touches the device."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_exported_with_the_declared_argtypes():
    from samrs_amd import engine
    lib = engine.load_library()
    assert lib.samrs_predict_multi.argtypes == engine.PREDICT_MULTI_ARGTYPES
    assert lib.samrs_predict_multi.restype == ctypes.c_int
    with open(os.path.join(ROOT, "include", "samrs_hip.h")) as f:
        decl = re.search(r"int samrs_predict_multi\(([^;]*)\);", f.read())
    assert decl is not None
    assert len(decl.group(1).split(",")) == len(engine.PREDICT_MULTI_ARGTYPES) == 17


def _rec(boxes=None, pts=None, mask=None):
    r = {"image": None, "original_size": (1024, 1024)}
    if boxes is not None:
        r["boxes"] = torch.zeros(boxes, 4)
    if pts is not None:
        r["point_coords"] = torch.zeros(2, pts, 2)
        r["point_labels"] = torch.ones(2, pts, dtype=torch.int32)
    if mask is not None:
        r["mask_inputs"] = torch.zeros(mask, 1, 256, 256)
    return r


def test_prompt_signature_grouping():
    from samrs_amd.build_sam import group_by_signature, prompt_signature
    recs = [_rec(boxes=3), _rec(pts=1), _rec(boxes=1), _rec(pts=3), _rec(boxes=2, mask=2), _rec(pts=1), _rec(mask=1),
            _rec(boxes=2, pts=1), _rec(boxes=5)]
    assert prompt_signature(recs[0]) == (False, 0, True, False)
    assert prompt_signature(recs[3]) == (True, 3, False, False)
    assert prompt_signature(recs[7]) == (True, 1, True, False)
    assert group_by_signature(recs) == [
        ((False, 0, True, False), [0, 2, 8]), ((True, 1, False, False), [1, 5]), ((True, 3, False, False), [3]),
        ((False, 0, True, True), [4]), ((False, 0, False, True), [6]), ((True, 1, True, False), [7])]
    assert group_by_signature([]) == []


def test_multi_call_args():
    from samrs_amd.engine import multi_call_args
    assert multi_call_args([2, 0, 2], [1, 0, 3], [(1024, 1024), (600, 1024), (1024, 800)], [(5, 6), (7, 8), (9, 10)], 4) == \
        ([2, 0, 2], [0, 1, 1, 4], [1024, 1024, 600, 1024, 1024, 800], [5, 6, 7, 8, 9, 10])
    with pytest.raises(ValueError, match="at least one image"):
        multi_call_args([], [], [], [], 0)
    with pytest.raises(ValueError, match="2 slots but 3 prompt counts"):
        multi_call_args([0, 1], [1, 1, 1], [(1, 1)] * 2, [(1, 1)] * 2, 3)
    with pytest.raises(ValueError, match="negative"):
        multi_call_args([0, 1], [2, -1], [(1, 1)] * 2, [(1, 1)] * 2, 1)
    with pytest.raises(ValueError, match="sum to 3 but the prompt tensors have 4"):
        multi_call_args([0, 1], [1, 2], [(1, 1)] * 2, [(1, 1)] * 2, 4)
    with pytest.raises(ValueError, match=r"\(h, w\)"):
        multi_call_args([0], [1], [(1, 1, 1)], [(1, 1)], 1)


def test_argument_errors_before_the_device():
    """Engine.predict_multi and Sam.forward refuse bad arguments before they touch the library or the device: the objects
    here have neither."""
    from samrs_amd.build_sam import Sam
    from samrs_amd.engine import Engine
    from samrs_amd.synth import CONFIGS
    eng = Engine.__new__(Engine)                     # no handle, no library, no device
    b = torch.zeros(5, 4)
    with pytest.raises(ValueError, match="sum to 4"):
        eng.predict_multi([0, 1], [1, 3], b, None, None, None, False, False, [(1024, 1024)] * 2, [(1024, 1024)] * 2)
    with pytest.raises(ValueError, match="1 input sizes"):
        eng.predict_multi([0, 1], [2, 3], b, None, None, None, False, False, [(1024, 1024)], [(1024, 1024)] * 2)
    sam = Sam(CONFIGS["vit_tiny"], {}, max_images=1)
    with pytest.raises(RuntimeError, match="HIP device"):
        sam([_rec(boxes=1)], False)
    sam.engine = SimpleNamespace()                   # "on a device", but no free slot besides SamPredictor's
    with pytest.raises(RuntimeError, match="max_images=1"):
        sam([_rec(boxes=1)], False)

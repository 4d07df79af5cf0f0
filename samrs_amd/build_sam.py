"""``sam_model_registry`` -- same names / call shape as the reference
(Generate Dataset/segment_anything/build_sam.py:14-107), returning a ``Sam`` handle whose compute
lives in ``libsamrs_hip.so``.

    sam = sam_model_registry["vit_h"](checkpoint="sam_vit_h_4b8939.pth")   # or checkpoint=None
    sam = sam.to(device="cuda")
    predictor = SamPredictor(sam)

``checkpoint=None`` gives seeded random weights (the reference gives unseeded random weights);
``state_dict=`` lets a caller pass tensors directly.
"""
from __future__ import annotations

import os
from types import SimpleNamespace
from typing import Any, Dict, List, Optional, Sequence, Tuple

import torch

from .engine import Engine
from .synth import CONFIGS, SamConfig, make_state_dict


def prompt_signature(record: Dict[str, Any]) -> Tuple[bool, int, bool, bool]:
    """(points?, points per prompt, boxes?, mask_inputs?) of one ``Sam.forward`` record: the prompt kind that one
    samrs_predict_multi call must share."""
    pts = record.get("point_coords")
    return (pts is not None, int(pts.shape[1]) if pts is not None and pts.dim() == 3 else 0,
            record.get("boxes") is not None, record.get("mask_inputs") is not None)


def group_by_signature(records: Sequence[Dict[str, Any]]) -> List[Tuple[Tuple[bool, int, bool, bool], List[int]]]:
    """Record indices grouped by prompt signature, groups in order of first appearance, indices ascending."""
    groups: Dict[Tuple[bool, int, bool, bool], List[int]] = {}
    for i, r in enumerate(records):
        groups.setdefault(prompt_signature(r), []).append(i)
    return list(groups.items())


class Sam:
    """Weights + (after ``.to('cuda')``) an engine handle.  Mirrors the attributes SAMRS's drivers
    touch: ``image_encoder.img_size`` (main_sam_rbox_mask_instance.py:135), ``device``,
    ``mask_threshold``, ``image_format`` (modeling/sam.py:19-20)."""

    mask_threshold: float = 0.0
    image_format: str = "RGB"

    def __init__(self, cfg: SamConfig, state_dict: Dict[str, torch.Tensor], precision: str = "f16",
                 max_images: int = 1, max_prompts: int = 64, max_points: int = 4, options: Optional[Dict[str, int]] = None,
                 audit_passes: int = 0):
        """``options``: per-engine options applied BEFORE the weights are loaded (include/samrs_hip.h samrs_set_option:
        "split", "decoder_fusion", "ln_fold", "gemm_variant").  ``audit_passes`` = N > 0: the first N encoder passes are profiled
        (samrs_amd/audit.py); when the engine has switched the profile off, ``audit_report`` is filled in and an
        ``OperandRangeWarning`` names the worst sites if there is a finding.  0: nothing is launched or read."""
        self.audit_passes = int(audit_passes)
        self.audit_report: Optional[Dict[str, Any]] = None
        self.cfg = cfg
        self.options = dict(options or {})
        self._state_dict = state_dict
        self.precision = precision
        self.max_images, self.max_prompts, self.max_points = max_images, max_prompts, max_points
        self.image_encoder = SimpleNamespace(img_size=cfg.img_size)
        self.engine: Optional[Engine] = None
        self._device = torch.device("cpu")

    @property
    def device(self) -> torch.device:
        return self._device

    def to(self, device=None, **kwargs) -> "Sam":
        device = torch.device(device if device is not None else kwargs.get("device", "cuda"))
        if device.type != "cuda":
            raise RuntimeError("samrs_amd.Sam can only live on a HIP device ('cuda'); there is no CPU path")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self.engine is not None and self.engine.device == device:
            return self
        self.engine = Engine(self.cfg, device, self.precision, self.max_images, self.max_prompts, self.max_points)
        for k, v in self.options.items():
            self.engine.set_option(k, v)
        # an explicit operand-split mode for the whole engine is the caller's decision, multimask outputs included (otherwise
        # the engine refuses multimask predicts on embeddings encoded below its multimask grade: samrs_get_slot_info)
        if "split" in self.options and "allow_reduced" not in self.options:
            self.engine.set_option("allow_reduced", 1)
        self.engine.load_state_dict(self._state_dict)
        # what this model runs in when nobody says otherwise (ViT-H: 79, else 15): the multimask-safe mode; the pipelines of
        # driver.py run THEIR OWN calls in it or in the 1x-rate mode by output contract (TilePipeline precision="auto") and leave
        # the engine's option as it is
        self.default_split = self.engine.get_option("split")
        self._device = device
        if self.audit_passes > 0:
            self.engine.start_audit(self.audit_passes, self._audit_finished)
        return self

    def finish_audit(self) -> Optional[Dict[str, Any]]:
        """The audit report of a model built with ``audit_passes``; a run that ended before the N-th encoder pass stops the audit
        here and reports the passes it did profile (None when there was none)."""
        eng = self.engine
        if self.audit_report is None and eng is not None and eng._audit_done is not None:
            left = eng.get_option("audit_passes")
            eng.start_audit(0)
            if left < self.audit_passes:
                self.audit_passes -= left
                self._audit_finished(eng)
        return self.audit_report

    def _audit_finished(self, engine: Engine) -> None:
        import warnings
        from . import audit
        self.audit_report = audit.collect(engine, self._state_dict, self.cfg, self.audit_passes)
        text = audit.warning_text(self.audit_report)
        if text:
            warnings.warn(text, audit.OperandRangeWarning, stacklevel=4)

    @torch.no_grad()
    def forward(self, batched_input: List[Dict[str, Any]], multimask_output: bool) -> List[Dict[str, torch.Tensor]]:
        """The reference's batched entry point (modeling/sam.py:53-131): per record an ``image`` (3xHxW, long side img_size,
        integer values 0..255), its ``original_size`` and optional ``point_coords`` / ``point_labels``, ``boxes``,
        ``mask_inputs`` in the input frame -> per record {"masks" bool [B, C, H, W], "iou_predictions" [B, C],
        "low_res_logits" [B, C, 256, 256]}, in input order.

        Images are encoded in chunks that fit embedding slots 1 .. max_images - 1 (slot 0 belongs to ``SamPredictor``, whose
        answers do not change across this call); the records of a chunk that share a prompt kind are decoded in one
        ``Engine.predict_multi`` call."""
        if self.engine is None:
            raise RuntimeError("move the model to a HIP device first: sam.to(device='cuda'); samrs_amd has no CPU path")
        slots = self.max_images - 1
        if slots < 1:
            raise RuntimeError(f"Sam.forward encodes into embedding slots 1 .. max_images - 1, and this model was built with "
                               f"max_images={self.max_images}; pass max_images >= 2 to sam_model_registry[...]")
        s = self.image_encoder.img_size
        tiles = []
        for i, r in enumerate(batched_input):
            img = r["image"]
            assert img.dim() == 3 and img.shape[0] == 3 and max(*img.shape[1:]) == s, \
                f"batched_input[{i}]['image'] must be 3xHxW with long side {s}, got {tuple(img.shape)}"
            t = img.to(self.device)
            if t.is_floating_point():
                assert bool((t == t.round()).all()) and float(t.min()) >= 0 and float(t.max()) <= 255, \
                    "Sam.forward needs integer pixel values in 0..255 (the engine takes uint8 tiles)"
            tiles.append(t.permute(1, 2, 0).round().clamp(0, 255).to(torch.uint8).contiguous())
            if "point_coords" in r and r.get("point_labels") is None:
                raise AssertionError("point_labels must be supplied if point_coords is supplied.")
            if prompt_signature(r) == (False, 0, False, False):
                raise AssertionError(f"batched_input[{i}]: at least one prompt (points, boxes or mask_inputs) is required")
        eng = self.engine
        outputs: List[Optional[Dict[str, torch.Tensor]]] = [None] * len(batched_input)
        for c0 in range(0, len(batched_input), slots):
            idx = list(range(c0, min(c0 + slots, len(batched_input))))
            eng.set_images_ragged([tiles[i] for i in idx], slot0=1)
            for _, members in group_by_signature([batched_input[i] for i in idx]):
                recs = [batched_input[idx[j]] for j in members]
                cat = lambda key: None if recs[0].get(key) is None else torch.cat([r[key].to(self.device) for r in recs])
                boxes = None if recs[0].get("boxes") is None else cat("boxes").reshape(-1, 4)
                counts = [int(r["boxes"].numel() // 4) if r.get("boxes") is not None else
                          int(r["point_coords"].shape[0]) if r.get("point_coords") is not None else int(r["mask_inputs"].shape[0])
                          for r in recs]
                masks, iou, low = eng.predict_multi(
                    [1 + j for j in members], counts, boxes, cat("point_coords"), cat("point_labels"), cat("mask_inputs"),
                    multimask_output, False,
                    [tuple(tiles[idx[j]].shape[:2]) for j in members], [tuple(int(v) for v in r["original_size"]) for r in recs])
                for k, j in enumerate(members):
                    outputs[idx[j]] = {"masks": masks[k], "iou_predictions": iou[k], "low_res_logits": low[k]}
        return outputs

    __call__ = forward

    def cuda(self, index: Optional[int] = None) -> "Sam":
        return self.to(torch.device("cuda", index) if index is not None else "cuda")

    def eval(self) -> "Sam":
        return self

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return self._state_dict


def _build_sam(cfg_name: str, checkpoint: Optional[str] = None, state_dict: Optional[Dict[str, torch.Tensor]] = None,
               **engine_kwargs) -> Sam:
    cfg = CONFIGS[cfg_name]
    if state_dict is None:
        if checkpoint is not None:
            with open(checkpoint, "rb") as f:
                state_dict = torch.load(f, map_location="cpu")
        else:
            state_dict = make_state_dict(cfg, int(os.environ.get("SAMRS_SEED", "0")))
    return Sam(cfg, state_dict, **engine_kwargs)


def build_sam_vit_h(checkpoint=None, **kw):
    return _build_sam("vit_h", checkpoint, **kw)


def build_sam_vit_l(checkpoint=None, **kw):
    return _build_sam("vit_l", checkpoint, **kw)


def build_sam_vit_b(checkpoint=None, **kw):
    return _build_sam("vit_b", checkpoint, **kw)


def build_sam_vit_tiny(checkpoint=None, **kw):      # test-only geometry, not in the reference registry
    return _build_sam("vit_tiny", checkpoint, **kw)


def build_sam_vit_tiny80(checkpoint=None, **kw):
    return _build_sam("vit_tiny80", checkpoint, **kw)


def build_sam_vit_tiny1280(checkpoint=None, **kw):
    return _build_sam("vit_tiny1280", checkpoint, **kw)


build_sam = build_sam_vit_h

sam_model_registry = {
    "default": build_sam_vit_h,
    "vit_h": build_sam_vit_h,
    "vit_l": build_sam_vit_l,
    "vit_b": build_sam_vit_b,
    "vit_tiny": build_sam_vit_tiny,
    "vit_tiny80": build_sam_vit_tiny80,
    "vit_tiny1280": build_sam_vit_tiny1280,
}

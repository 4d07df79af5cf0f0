"""Checkpoint audit: is this checkpoint safe on f16 operands, and does the outlier treatment cover the columns that are really hot?

    python -m samrs_amd.audit --model vit_h --checkpoint sam_vit_h_4b8939.pth [--images DIR | --synthetic N] [--passes 4]
                              [--precision f16] [--split S] [--json OUT]

encodes a few batches of images with the engine option ``audit_passes`` on and prints, per operand tensor of the encoder (the engine's
audit SITES, ``include/samrs_hip.h``), how much of the operand type's range it uses -- saturated values, the largest magnitude and the
headroom in bits, the share of subnormals -- and, per block GEMM, the K-columns whose MEASURED operand magnitude x weight column norm
stands out, next to the columns the engine picked from the weights alone (``samrs_amd.outliers``).  Exit status 0: clean, 2: some tensor
saturated (run the checkpoint with ``--precision bf16``) -- a job script can gate a dataset run on it.

The numbers come from two HIP kernels (``samrs_amd/csrc/audit_kernels.hip``); this module holds their host-side statement
(:func:`profile_of`, the kernels' test reference) and turns rows into a report.  Everything above :func:`collect` runs without a GPU.
"""
from __future__ import annotations

import json
import math
import os
import sys
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import outliers

PROFILE_WORDS = 48
BIN0, N_BINS, MIN_LOG2 = 8, 40, -24          # row[BIN0 + b] counts floor(log2 |x|) == b + MIN_LOG2, clamped into the 40 bins
# operand formats: mantissa bits, exponent bias, the all-ones exponent, the largest finite magnitude pattern
FORMATS = {"f16": (10, 15, 31, 0x7BFF), "bf16": (7, 127, 255, 0x7F7F)}
FORMATS["fp16"] = FORMATS["f16"]
GEMM_SITE = {"qkv": "qkv_in", "lin1": "lin1_in", "lin2": "lin2_in", "proj": "proj_in"}
GEMM_WEIGHT = {"qkv": ".attn.qkv.weight", "lin1": ".mlp.lin1.weight", "lin2": ".mlp.lin2.weight", "proj": ".attn.proj.weight"}
TIGHT_BITS = 1.0
# SUBNORMAL: more than HALF of a site's non-zero elements below the smallest normal number.  The tail of every tensor reaches into the
# subnormals harmlessly (GELU of a pre-activation below -4.2 is a negative number under 2^-14; such elements add nothing a dot product
# can see), so a small share says nothing.  Past one half it is the MEDIAN magnitude that sits under the normal range: the bulk of the
# operand, not its tail, has lost mantissa bits, and the GEMM's relative operand error is no longer the 2^-11 the parity figures assume.
SUBNORMAL_FRACTION = 0.5


class OperandRangeWarning(UserWarning):
    """The profiled encoder passes of a model built with ``audit_passes=N`` found operand tensors at or near the end of the operand
    type's range, or hot columns the outlier treatment does not cover (``Sam.audit_report`` has the details)."""


def pattern_value(pattern: int, prec: str) -> float:
    """The magnitude a 15-bit pattern ``bits & 0x7fff`` of the operand type stands for."""
    mant, bias, exp_all, _ = FORMATS[prec]
    ex, m = int(pattern) >> mant, int(pattern) & ((1 << mant) - 1)
    if ex == exp_all:
        return math.inf if m == 0 else math.nan
    if ex == 0:
        return m * 2.0 ** (1 - bias - mant)
    return (1.0 + m * 2.0 ** -mant) * 2.0 ** (ex - bias)


def profile_of(bits: np.ndarray, prec: str) -> np.ndarray:
    """The profile row (int64 [48]) of a tensor given as uint16 bit patterns: the numpy statement of ``range_profile_kernel``, in
    integer arithmetic on the patterns.  [0] elements, [1] zeros, [2] subnormals, [3] elements at the largest finite magnitude, [4] inf /
    nan, [5] the largest finite magnitude's pattern, [8 + b] finite non-zero elements with floor(log2 |x|) == b - 24 (clamped)."""
    mant, bias, exp_all, max_finite = FORMATS[prec]
    m = (np.asarray(bits).astype(np.uint16).ravel() & 0x7FFF).astype(np.int64)
    ex = m >> mant
    row = np.zeros(PROFILE_WORDS, dtype=np.int64)
    row[0] = m.size
    row[1] = int((m == 0).sum())
    infnan = ex == exp_all
    row[4] = int(infnan.sum())
    live = (m != 0) & ~infnan
    sub = live & (ex == 0)
    row[2] = int(sub.sum())
    row[3] = int((m == max_finite).sum())
    row[5] = int(m[live].max()) if live.any() else 0
    # floor(log2): normals from the exponent field; subnormals m * 2^(1 - bias - mant) from the position of m's leading bit
    lead = np.zeros_like(m)
    ms = m[sub]
    for k in range(1, mant):
        lead[sub] += (ms >> k) > 0
    lg = np.where(ex > 0, ex - bias, lead + 1 - bias - mant)
    b = np.clip(lg[live] - MIN_LOG2, 0, N_BINS - 1)
    row[BIN0:BIN0 + N_BINS] = np.bincount(b, minlength=N_BINS)
    return row


def site_report(names: Sequence[str], rows: np.ndarray, prec: str) -> List[Dict]:
    """One dict per site: elements, saturated (at the largest finite magnitude), inf_nan, largest (magnitude), headroom_bits =
    log2(max finite / largest) (None while nothing non-zero was seen), top_log2 (the highest occupied bin's exponent),
    subnormal_fraction (of the non-zero finite elements), zero_fraction."""
    max_val = pattern_value(FORMATS[prec][3], prec)
    rows = np.asarray(rows, dtype=np.int64).reshape(len(names), PROFILE_WORDS)
    out = []
    for name, r in zip(names, rows):
        n, zeros, sub, at_max, infnan, top = (int(v) for v in r[:6])
        bins = r[BIN0:BIN0 + N_BINS]
        nonzero = int(bins.sum())
        largest = pattern_value(top, prec)
        occupied = np.nonzero(bins)[0]
        out.append({"site": name, "elements": n, "saturated": at_max, "inf_nan": infnan, "largest": largest,
                    "headroom_bits": math.log2(max_val / largest) if largest > 0 else None,
                    "top_log2": int(occupied[-1]) + MIN_LOG2 if len(occupied) else None,
                    "subnormal_fraction": sub / nonzero if nonzero else 0.0, "zero_fraction": zeros / n if n else 0.0,
                    "consistent": zeros + infnan + nonzero == n})
    return out


def column_report(sd, cfg, block: int, gemm: str, sumsq, n_rows: int, engine_picks: Sequence[int], ratio: float = 4.0) -> Dict:
    """Measured outlier columns of one block GEMM: score_c = rms_c x ||W[:, c]|| with rms_c = sqrt(sumsq_c / n_rows) from the engine's
    column statistics, picked by the rule of ``outliers.pick`` (above ``ratio`` x the median score, at most 32, the largest).
    ``engine_picks`` are the columns the engine treats (``Engine.outlier_columns``: read from the engine, whose median differs from the
    host rule's on even lengths).  -> measured_picks, engine_picks, uncovered (measured, not treated) and the share of the measured
    squared-score mass they carry, measured_share, unmeasured (treated, not measured)."""
    import torch
    gemm = outliers.GEMMS[gemm] if isinstance(gemm, int) else gemm
    w = sd[f"image_encoder.blocks.{block}{GEMM_WEIGHT[gemm]}"].detach().to(torch.float64)
    rms = torch.as_tensor(np.sqrt(np.asarray(sumsq, dtype=np.float64) / max(int(n_rows), 1)))
    if rms.numel() != w.shape[1]:
        raise ValueError(f"block {block} {gemm}: {rms.numel()} column statistics for a weight with K = {w.shape[1]}")
    score = rms * w.norm(dim=0)
    idx, share = outliers.pick(score, ratio)
    measured = [int(i) for i in idx]
    treated = sorted(int(i) for i in engine_picks)
    uncovered = [c for c in measured if c not in set(treated)]
    total = float(score.square().sum().clamp(min=1e-300))
    return {"block": int(block), "gemm": gemm, "measured_picks": measured, "engine_picks": treated, "uncovered": uncovered,
            "uncovered_share": float(score[uncovered].square().sum()) / total if uncovered else 0.0, "measured_share": share,
            "unmeasured": [c for c in treated if c not in set(measured)],
            "score_ratio_max": float(score.max() / score.median().clamp(min=1e-300))}


def verdict(report: Dict) -> List[Dict]:
    """Findings of a report {"precision", "sites": site_report(...), "gemms": [column_report(...)]}:
    SATURATED (sites with elements at the largest finite magnitude or inf / nan, first in data-flow order first; remedy: bf16),
    TIGHT (less than one bit of headroom, not saturated), UNCOVERED_OUTLIERS (one per block GEMM with measured outlier columns the engine
    does not treat), SUBNORMAL (more than SUBNORMAL_FRACTION of a site's non-zero elements below the smallest normal number)."""
    out: List[Dict] = []
    sites = report.get("sites", [])
    sat = [(s["site"], s["saturated"] + s["inf_nan"]) for s in sites if s["saturated"] + s["inf_nan"] > 0]
    if sat:
        out.append({"kind": "SATURATED", "sites": sat,
                    "remedy": 'build the model with precision="bf16" (fp32 exponent range; include/samrs_hip.h option "range_check")'})
    tight = [(s["site"], s["headroom_bits"]) for s in sites
             if s["saturated"] + s["inf_nan"] == 0 and s["headroom_bits"] is not None and s["headroom_bits"] < TIGHT_BITS]
    if tight:
        out.append({"kind": "TIGHT", "sites": tight})
    for g in report.get("gemms", []):
        if g["uncovered"]:
            out.append({"kind": "UNCOVERED_OUTLIERS", "block": g["block"], "gemm": g["gemm"], "columns": g["uncovered"],
                        "mass_share": g["uncovered_share"]})
    subn = [(s["site"], s["subnormal_fraction"]) for s in sites if s["subnormal_fraction"] > SUBNORMAL_FRACTION]
    if subn:
        out.append({"kind": "SUBNORMAL", "sites": subn})
    return out


def exit_code(report: Dict) -> int:
    """0 = clean enough to run, 2 = some operand tensor saturated."""
    return 2 if any(f["kind"] == "SATURATED" for f in report.get("findings", verdict(report))) else 0


def format_report(report: Dict) -> str:
    lines = [f"operand type {report['precision']}, {report.get('passes', '?')} encoder pass(es) profiled",
             f"{'site':24s} {'elements':>12s} {'saturated':>10s} {'inf/nan':>8s} {'largest':>11s} {'headroom':>9s} {'subnormal':>10s} {'zero':>8s}"]
    for s in report["sites"]:
        head = "-" if s["headroom_bits"] is None else f"{s['headroom_bits']:.2f} b"
        lines.append(f"{s['site']:24s} {s['elements']:12d} {s['saturated']:10d} {s['inf_nan']:8d} {s['largest']:11.4g} {head:>9s} "
                     f"{s['subnormal_fraction']:10.2e} {s['zero_fraction']:8.2e}")
    if report.get("gemms"):
        lines.append(f"{'block':>5s} {'gemm':5s} {'measured':>9s} {'treated':>8s} {'uncovered':>10s} {'their mass':>11s} {'max / median':>13s}")
        for g in report["gemms"]:
            lines.append(f"{g['block']:5d} {g['gemm']:5s} {len(g['measured_picks']):9d} {len(g['engine_picks']):8d} {len(g['uncovered']):10d} "
                         f"{g['uncovered_share']:11.3f} {g['score_ratio_max']:13.1f}")
    findings = report.get("findings", [])
    for f in findings:
        if f["kind"] == "SATURATED":
            lines.append("SATURATED: " + ", ".join(f"{n} ({c})" for n, c in f["sites"][:8]) + (" ..." if len(f["sites"]) > 8 else "")
                         + " -- " + f["remedy"])
        elif f["kind"] == "TIGHT":
            lines.append("TIGHT (< 1 bit of headroom): " + ", ".join(f"{n} ({h:.2f})" for n, h in f["sites"][:8]))
        elif f["kind"] == "UNCOVERED_OUTLIERS":
            lines.append(f"UNCOVERED_OUTLIERS: block {f['block']} {f['gemm']}: columns {f['columns']} carry {f['mass_share']:.3f} of the "
                         "measured squared-score mass and take no hi + lo terms")
        elif f["kind"] == "SUBNORMAL":
            lines.append("SUBNORMAL (more than half of the non-zero elements): " + ", ".join(f"{n} ({v:.2f})" for n, v in f["sites"][:8]))
    if not findings:
        lines.append("no findings: every operand tensor fits the operand type with at least one bit to spare, and the outlier treatment "
                     "covers the measured hot columns")
    return "\n".join(lines)


def warning_text(report: Dict) -> Optional[str]:
    """One sentence naming the worst sites, or None.  The warning is about the operand RANGE: it is raised by a SATURATED, TIGHT or
    SUBNORMAL finding (and then also mentions untreated outlier columns).  Untreated columns alone do not warn -- they cost accuracy by
    degrees, not a wrong mask, and seeded-normal weights already show a few at 4 - 5x the median; they are in the report."""
    parts, tail = [], []
    for f in report.get("findings", []):
        if f["kind"] == "SATURATED":
            parts.append(f"{len(f['sites'])} operand tensor(s) saturated the {report['precision']} range, first " +
                         ", ".join(f"{n} ({c} values)" for n, c in f["sites"][:4]) + ": " + f["remedy"])
        elif f["kind"] == "TIGHT":
            parts.append("less than one bit of headroom at " + ", ".join(f"{n} ({h:.2f} bit)" for n, h in f["sites"][:4]))
        elif f["kind"] == "SUBNORMAL":
            parts.append("mostly subnormal operands at " + ", ".join(n for n, _ in f["sites"][:4]))
        elif f["kind"] == "UNCOVERED_OUTLIERS":
            tail.append(f"block {f['block']} {f['gemm']}: {len(f['columns'])} measured outlier column(s) untreated "
                        f"({f['mass_share']:.2f} of the score mass)")
    return "checkpoint audit: " + "; ".join(parts + tail[:3]) if parts else None


# ---- GPU side ------------------------------------------------------------------------------------------------------------------------
def collect(engine, sd, cfg, passes: Optional[int] = None) -> Dict:
    """Read the engine's audit state into a report with findings (synchronises the device)."""
    sites = engine.audit_sites()
    names = [n for n, _ in sites]
    prec = "bf16" if engine.precision == "bf16" else "f16"
    report = {"precision": prec, "passes": passes, "sites": site_report(names, engine.range_profile(), prec), "gemms": []}
    ratio = engine.get_option("outlier_ratio_pct") / 100.0
    for i in range(cfg.depth):
        for gi, g in enumerate(outliers.GEMMS):
            site = names.index(f"blocks.{i}.{GEMM_SITE[g]}")
            try:
                st = engine.column_stats(site)
            except AssertionError:              # profiled with "range_profile" = 1: no column statistics
                continue
            report["gemms"].append(column_report(sd, cfg, i, g, st["sumsq"], st["n_rows"], engine.outlier_columns(i, gi), ratio))
    report["findings"] = verdict(report)
    return report


def run_audit(sam, images, passes: int = 4) -> Dict:
    """Encode ``images`` (uint8 HWC arrays of any size) on ``sam`` in batches of ``sam.max_images``, at most ``passes`` of them, with the
    engine option ``audit_passes`` on, and return the report.  Leaves the engine's audit switched off."""
    import torch
    from .transforms import ResizeLongestSide
    eng = sam.engine
    if eng is None:
        raise RuntimeError("move the model to a HIP device first: sam.to(device='cuda')")
    tr = ResizeLongestSide(sam.image_encoder.img_size)
    batches = [images[i:i + sam.max_images] for i in range(0, len(images), sam.max_images)][:max(int(passes), 1)]
    if not batches:
        raise ValueError("run_audit needs at least one image")
    eng.start_audit(len(batches))
    for b in batches:
        tiles = [tr.apply_image_device(torch.as_tensor(np.ascontiguousarray(im), device=eng.device)).contiguous() for im in b]
        eng.set_images_ragged(tiles, slot0=0)
    assert eng.get_option("audit_passes") == 0 and eng.get_option("range_profile") == 0
    for s in range(min(len(batches[-1]), sam.max_images)):
        eng.reset_image(s)
    return collect(eng, sam.state_dict(), sam.cfg, len(batches))


def write_json(report: Dict, path: str) -> None:
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(report, f, indent=1)


def build_parser():
    import argparse
    from .synth import CONFIGS
    ap = argparse.ArgumentParser(prog="python -m samrs_amd.audit", description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", default="vit_h", choices=sorted(CONFIGS))
    ap.add_argument("--checkpoint", default=None, help="a SAM state_dict saved with torch.save (default: the seeded test weights)")
    src = ap.add_mutually_exclusive_group()
    src.add_argument("--images", default=None, help="directory of image files to encode")
    src.add_argument("--synthetic", type=int, default=None, metavar="N", help="N synthetic tiles (synth.make_image) instead of files")
    ap.add_argument("--passes", type=int, default=4, help="encoder passes to profile")
    ap.add_argument("--batch", type=int, default=0, help="tiles per encoder pass (default: 8 at ViT-H scale, else 1)")
    ap.add_argument("--precision", default="f16", choices=["f16", "bf16"])
    ap.add_argument("--split", type=int, default=None, help='engine operand-split mode (option "split"; default: the model\'s own)')
    ap.add_argument("--json", default=None, metavar="OUT", help="also write the report as JSON")
    ap.add_argument("--device", default="cuda:0")
    return ap


def load_images(args, batch: int) -> List[np.ndarray]:
    from . import synth
    want = max(args.passes, 1) * batch
    if args.images:
        from . import tile_io
        exts = (".png", ".jpg", ".jpeg", ".tif", ".bmp")
        files = sorted(f for f in os.listdir(args.images) if f.lower().endswith(exts))[:want]
        if not files:
            raise SystemExit(f"no image files in {args.images}")
        out = []
        for f in files:
            path = os.path.join(args.images, f)
            if f.lower().endswith(".png"):
                out.append(tile_io.read_rgb(path))
            else:
                from PIL import Image
                out.append(np.asarray(Image.open(path).convert("RGB")))
        return out
    n = args.synthetic if args.synthetic else want
    return [synth.make_image(i) for i in range(n)]


def main(argv=None) -> int:
    import torch
    import samrs_amd
    from .synth import CONFIGS
    args = build_parser().parse_args(argv)
    cfg = CONFIGS[args.model]
    batch = args.batch if args.batch > 0 else (8 if cfg.embed_dim >= 1024 else 1)
    opts = {} if args.split is None else {"split": args.split}
    sam = samrs_amd.sam_model_registry[args.model](checkpoint=args.checkpoint, precision=args.precision, options=opts,
                                                   max_images=batch)
    print(f"== load-time outlier columns (samrs_amd.outliers: from the weights alone) ==", flush=True)
    oc = outliers.outlier_columns(sam.state_dict(), cfg)
    total = sum(len(idx) for idx, _ in oc.values())
    per_gemm = {g: sum(len(oc[(i, g)][0]) for i in range(cfg.depth)) for g in outliers.GEMMS}
    print(f"{total} outlier columns over {cfg.depth} blocks: " + ", ".join(f"{g} {n}" for g, n in per_gemm.items()), flush=True)
    sam = sam.to(args.device)
    report = run_audit(sam, load_images(args, batch), args.passes)
    torch.cuda.synchronize()
    print("== measured ==")
    print(format_report(report))
    if args.json:
        write_json(report, args.json)
    return exit_code(report)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

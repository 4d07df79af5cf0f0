"""CPU: the checkpoint audit's host side (samrs_amd/audit.py) and its C ABI surface -- no GPU is touched.

The profile row's numpy statement (``audit.profile_of``, the GPU tests' reference for ``range_profile_kernel``) is checked here against
an INDEPENDENT statement on every 16-bit pattern: the pattern's value as a float, then ``np.frexp``."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from samrs_amd import audit, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC = ("samrs_audit_site_count", "samrs_audit_site_name", "samrs_audit_read_profile", "samrs_audit_read_columns")
KERNEL = ("samrs_k_range_profile", "samrs_k_column_stats")


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(samrs_[a-z0-9_]+)\s*\(", text))


def test_headers_declare_and_the_library_exports_the_audit_entry_points():
    import __graft_entry__ as ge
    ge.build_library()
    from samrs_amd import engine
    assert set(PUBLIC) <= _declared("samrs_hip.h")
    assert set(KERNEL) <= _declared("samrs_hip_internal.h") and not set(KERNEL) & _declared("samrs_hip.h")
    raw = ctypes.CDLL(engine.LIB_PATH)
    for name in PUBLIC + KERNEL:
        assert hasattr(raw, name), name
    lib = engine.load_library()
    assert lib.samrs_abi_version() == 5                    # additive: the ABI version does not move
    for name in PUBLIC + KERNEL:
        assert getattr(lib, name).argtypes is not None, name
    # the constant the column statistics' error bound is derived from is readable from the library and equals kernels.h
    text = open(os.path.join(ROOT, "samrs_amd", "csrc", "kernels.h")).read()
    r = int(re.search(r"constexpr int AUDIT_ROWS_PER_PARTIAL = (\d+);", text).group(1))
    assert lib.samrs_k_audit_rows_per_partial() == r and 1 < r <= 256


def _independent_profile(prec):
    """Every 16-bit pattern once: the pattern -> its value as a float -> frexp."""
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    if prec == "f16":
        val = np.frombuffer(bits.tobytes(), dtype=np.float16).astype(np.float64)
        tiny, top = 2.0 ** -14, 65504.0
    else:
        with np.errstate(invalid="ignore"):                  # signalling-NaN patterns widen to quiet NaNs
            val = np.frombuffer((bits.astype(np.uint32) << 16).tobytes(), dtype=np.float32).astype(np.float64)
        tiny, top = 2.0 ** -126, float(np.frombuffer(np.uint32(0x7F7F0000).tobytes(), dtype=np.float32)[0])
    mag = np.abs(val)
    finite = np.isfinite(val)
    live = finite & (mag > 0)
    row = np.zeros(48, dtype=np.int64)
    row[0] = bits.size
    row[1] = int((mag == 0).sum())
    row[2] = int((live & (mag < tiny)).sum())
    row[3] = int((mag == top).sum())
    row[4] = int((~finite).sum())
    _, e = np.frexp(mag[live])                             # mag = f * 2^e with 0.5 <= f < 1: floor(log2 mag) = e - 1
    b = np.clip(e - 1 + 24, 0, 39)
    row[8:] = np.bincount(b, minlength=40)
    largest = mag[live].max()
    return bits, row, largest


@pytest.mark.parametrize("prec", ["f16", "bf16"])
def test_profile_of_on_all_65536_patterns(prec):
    bits, want, largest = _independent_profile(prec)
    got = audit.profile_of(bits, prec)
    assert got.dtype == np.int64 and got.shape == (48,)
    assert audit.pattern_value(int(got[5]), prec) == largest
    want[5] = got[5]
    assert np.array_equal(got, want), (got, want)
    assert got[1] + got[4] + got[8:].sum() == got[0] and got[6] == 0 and got[7] == 0        # the invariant
    assert got[1] == 2 and got[3] == 2                                                      # +-0, +-max
    if prec == "f16":
        # f16 covers the 40 bins exactly: 2 * 2^b subnormal patterns (both signs) in bins b = 0 .. 9, 2048 per normal binade
        assert got[8:18].tolist() == [2 << k for k in range(10)] and set(got[18:].tolist()) == {2048}
        assert got[2] == 2 * 1023 and got[4] == 2 * 1024
    else:
        # bf16 clamps at both ends: everything below 2^-24 (subnormals included) in bin 0, everything from 2^15 up in bin 39
        assert set(got[9:47].tolist()) == {256} and got[8] == 256 * (127 - 24) + 254 and got[47] == 256 * (127 - 15 + 1)
        assert got[2] == 2 * 127 and got[4] == 2 * 128
    # shuffled and repeated patterns give the same counts times the repetition
    rng = np.random.default_rng(0)
    many = rng.permutation(np.tile(bits, 3))
    got3 = audit.profile_of(many, prec)
    want3 = want * 3
    want3[5] = want[5]
    assert np.array_equal(got3, want3)


def _row(prec, values=(), zeros=0):
    """A profile row of hand-made content: `values` are magnitudes representable in the operand type."""
    dt = torch.float16 if prec == "f16" else torch.bfloat16
    t = torch.tensor(list(values) + [0.0] * zeros, dtype=torch.float32).to(dt)
    return audit.profile_of(t.view(torch.int16).numpy().view(np.uint16), prec)


def test_site_report_and_verdict_name_saturated_and_tight_sites():
    names = ["blocks.0.qkv_in", "blocks.0.v", "blocks.0.proj_in", "blocks.0.lin2_in", "neck.conv1_in"]
    rows = np.stack([
        _row("f16", [1.0, -2.5, 96.0], zeros=1),                   # comfortable
        _row("f16", [65504.0, -65504.0, 3.0, 12.0]),               # saturated twice
        _row("f16", [40000.0, 1.0]),                               # log2(65504 / 40000) = 0.71 bit: TIGHT
        _row("f16", [30000.0, -1.0]),                              # 1.13 bit: not tight
        _row("f16", [3e-6, -2e-5, 5e-5, 0.5]),                     # 3 of 4 non-zero elements subnormal
    ])
    rep = audit.site_report(names, rows, "f16")
    by = {s["site"]: s for s in rep}
    assert all(s["consistent"] for s in rep)
    assert by["blocks.0.qkv_in"]["elements"] == 4 and by["blocks.0.qkv_in"]["zero_fraction"] == 0.25
    assert by["blocks.0.qkv_in"]["largest"] == 96.0 and by["blocks.0.qkv_in"]["top_log2"] == 6
    assert by["blocks.0.v"]["saturated"] == 2 and by["blocks.0.v"]["headroom_bits"] == 0.0
    assert by["blocks.0.proj_in"]["headroom_bits"] == pytest.approx(math.log2(65504 / 40000)) and round(by["blocks.0.proj_in"]["headroom_bits"], 2) == 0.71
    assert round(by["blocks.0.lin2_in"]["headroom_bits"], 2) == 1.13
    assert by["neck.conv1_in"]["subnormal_fraction"] == 0.75
    findings = audit.verdict({"precision": "f16", "sites": rep, "gemms": []})
    kinds = {f["kind"]: f for f in findings}
    assert set(kinds) == {"SATURATED", "TIGHT", "SUBNORMAL"}
    assert kinds["SATURATED"]["sites"] == [("blocks.0.v", 2)] and "bf16" in kinds["SATURATED"]["remedy"]
    assert [n for n, _ in kinds["TIGHT"]["sites"]] == ["blocks.0.proj_in"]
    assert [n for n, _ in kinds["SUBNORMAL"]["sites"]] == ["neck.conv1_in"]
    text = audit.warning_text({"precision": "f16", "sites": rep, "gemms": [], "findings": findings})
    assert "blocks.0.v" in text and "bf16" in text
    assert audit.warning_text({"precision": "f16", "sites": rep[:1], "gemms": [], "findings": []}) is None
    # bf16: inf / nan is the only way to saturate
    r = audit.site_report(["x"], _row("bf16", [float("inf"), 1e30, 1.0])[None], "bf16")
    assert r[0]["inf_nan"] == 1 and r[0]["saturated"] == 0 and r[0]["headroom_bits"] > 20
    assert audit.verdict({"precision": "bf16", "sites": r, "gemms": []})[0]["sites"] == [("x", 1)]


def test_column_report_finds_an_uncovered_measured_outlier_with_its_mass_share():
    cfg = synth.CONFIGS["vit_tiny"]
    D = cfg.embed_dim
    w = torch.ones(3 * D, D)                                       # every column norm = sqrt(3 D)
    w[:, 7] *= 2.0
    sd = {"image_encoder.blocks.1.attn.qkv.weight": w}
    n_rows = 100
    rms = np.ones(D)
    rms[3], rms[7], rms[11] = 10.0, 3.0, 5.0                       # scores / sqrt(3 D): 10, 6, 5 against a median of 1 -> all above 4 x
    sumsq = rms ** 2 * n_rows
    rep = audit.column_report(sd, cfg, 1, "qkv", sumsq, n_rows, engine_picks=[3, 11])
    assert rep["measured_picks"] == [3, 7, 11] and rep["engine_picks"] == [3, 11] and rep["uncovered"] == [7] and rep["unmeasured"] == []
    total = (D - 3) * 1.0 + 100.0 + 36.0 + 25.0                    # squared scores / (3 D), by hand
    assert rep["uncovered_share"] == pytest.approx(36.0 / total, rel=1e-12)
    assert rep["measured_share"] == pytest.approx(161.0 / total, rel=1e-6)
    same = audit.column_report(sd, cfg, 1, 0, sumsq, n_rows, engine_picks=[3, 7, 11])      # GEMM by index, everything treated
    assert same["uncovered"] == [] and same["uncovered_share"] == 0.0
    extra = audit.column_report(sd, cfg, 1, "qkv", sumsq, n_rows, engine_picks=[3, 7, 11, 20])
    assert extra["uncovered"] == [] and extra["unmeasured"] == [20]
    findings = audit.verdict({"precision": "f16", "sites": [], "gemms": [rep, same]})
    assert findings == [{"kind": "UNCOVERED_OUTLIERS", "block": 1, "gemm": "qkv", "columns": [7], "mass_share": rep["uncovered_share"]}]
    with pytest.raises(ValueError):
        audit.column_report(sd, cfg, 1, "qkv", sumsq[:-1], n_rows, engine_picks=[])
    # untreated columns are reported, but the RANGE warning is not raised for them alone
    assert audit.warning_text({"precision": "f16", "sites": [], "gemms": [rep], "findings": findings}) is None


def test_cli_arguments_and_the_exit_code_rule():
    a = audit.build_parser().parse_args(["--model", "vit_tiny", "--checkpoint", "w.pth", "--synthetic", "2", "--passes", "1", "--json", "f.json"])
    assert (a.model, a.checkpoint, a.synthetic, a.images, a.passes, a.json, a.precision, a.split) == ("vit_tiny", "w.pth", 2, None, 1, "f.json", "f16", None)
    d = audit.build_parser().parse_args([])
    assert (d.model, d.passes, d.precision, d.synthetic, d.images) == ("vit_h", 4, "f16", None, None)
    with pytest.raises(SystemExit):
        audit.build_parser().parse_args(["--images", "dir", "--synthetic", "2"])       # one source of images
    with pytest.raises(SystemExit):
        audit.build_parser().parse_args(["--precision", "fp8"])
    sat = {"precision": "f16", "passes": 1, "gemms": [],
           "sites": audit.site_report(["blocks.0.v", "blocks.0.q"], np.stack([_row("f16", [65504.0, 1.0]), _row("f16", [2.0])]), "f16")}
    sat["findings"] = audit.verdict(sat)
    assert audit.exit_code(sat) == 2
    tight = {"precision": "f16", "passes": 1, "gemms": [], "sites": audit.site_report(["blocks.0.v"], _row("f16", [40000.0])[None], "f16")}
    tight["findings"] = audit.verdict(tight)
    assert [f["kind"] for f in tight["findings"]] == ["TIGHT"] and audit.exit_code(tight) == 0      # only SATURATED gates a run
    clean = {"precision": "f16", "passes": 1, "gemms": [], "sites": audit.site_report(["blocks.0.v"], _row("f16", [2.0])[None], "f16")}
    assert audit.verdict(clean) == [] and audit.exit_code(clean) == 0
    out = audit.format_report(sat)
    assert "blocks.0.v" in out and "SATURATED" in out and "no findings" in audit.format_report({**clean, "findings": []})
    for cli in ("generate", "instances"):
        src = open(os.path.join(ROOT, "samrs_amd", cli + ".py")).read()
        assert '"--audit-passes"' in src
    from samrs_amd import generate
    assert generate.build_parser().parse_args(["--images", "i", "--boxes", "b", "--out", "o"]).audit_passes == 0
    assert generate.build_parser().parse_args(["--images", "i", "--boxes", "b", "--out", "o", "--audit-passes", "4"]).audit_passes == 4

"""GPU: the checkpoint audit -- the two kernels alone against their numpy statements (exact integers; a derived bound for the one
fp32 chain), the engine's audit sites against the unchanged "saturated" counter and against the fp32 oracle's tensors, "audit_passes",
the warning, the CLIs, and one ViT-H pass (the shape the feature exists for)."""
import json
import math
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from samrs_amd import audit, outliers, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREC = {"bf16": 0, "f16": 1}
OUTSIDE = dict(hidden_scale=1e5, v_scale=1e5, gamma_scale=30.0)        # GELU(lin1) and v beyond 65504 in the planted blocks
INSIDE = dict(hidden_scale=3e3, v_scale=3e3, gamma_scale=30.0)


def _lib():
    from samrs_amd import engine
    return engine.load_library()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev_bits(bits_u16: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(bits_u16.view(np.int16)).cuda()


def _profile(prec, t, n, cols, ld, row=None):
    row = torch.zeros(48, dtype=torch.int64, device="cuda") if row is None else row
    assert _lib().samrs_k_range_profile(PREC[prec], t.data_ptr(), n, cols, ld, row.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    return row


@pytest.mark.parametrize("prec", ["f16", "bf16"])
def test_range_profile_kernel_is_exact(prec):
    rng = np.random.default_rng(5)
    # (a) every 16-bit pattern 8 times, shuffled
    bits = rng.permutation(np.tile(np.arange(65536, dtype=np.uint32).astype(np.uint16), 8))
    t = _dev_bits(bits)
    r1 = _profile(prec, t, bits.size, 0, 0).cpu().numpy()
    r2 = _profile(prec, t, bits.size, 0, 0).cpu().numpy()
    want = audit.profile_of(bits, prec)
    print(f"{prec} all patterns x 8: {r1[:6].tolist()}")
    assert np.array_equal(r1, want) and np.array_equal(r1, r2)
    assert r1[1] + r1[4] + r1[8:].sum() == r1[0]
    acc = _profile(prec, t, bits.size, 0, 0)                     # a second call on the same row ADDS (the maximum stays a maximum)
    acc = _profile(prec, t, bits.size, 0, 0, acc).cpu().numpy()
    want2 = 2 * want
    want2[5] = want[5]
    assert np.array_equal(acc, want2)
    # (b) rows of 1280 live columns at a stride of 1408 whose pad columns hold the saturation pattern: the pad is never read
    rows = 512
    full = np.full((rows, 1408), 0x7BFF if prec == "f16" else 0x7F7F, dtype=np.uint16)
    live = rng.integers(0, 65536, size=(rows, 1280), dtype=np.uint32).astype(np.uint16)
    if prec == "f16":
        live[(live & 0x7FFF) == 0x7BFF] = 0x3C00
    else:
        live[(live & 0x7FFF) == 0x7F7F] = 0x3F80
    full[:, :1280] = live
    got = _profile(prec, _dev_bits(full.ravel()), rows * 1280, 1280, 1408).cpu().numpy()
    assert np.array_equal(got, audit.profile_of(live, prec)) and got[3] == 0 and got[0] == rows * 1280
    # (c) 2^24 elements of ONE exponent (every lane counts into the same bin): exact, and reproducible
    n = 1 << 24
    mant_bits, one = (10, 0x3C00) if prec == "f16" else (7, 0x3F80)
    same = (one | rng.integers(0, 1 << mant_bits, size=n, dtype=np.uint32)).astype(np.uint16)
    same[::2] |= 0x8000
    t = _dev_bits(same)
    c1, c2 = _profile(prec, t, n, 0, 0).cpu().numpy(), _profile(prec, t, n, 0, 0).cpu().numpy()
    want = audit.profile_of(same, prec)
    assert want[8 + 24] == n and np.array_equal(c1, want) and np.array_equal(c1, c2)


@pytest.mark.parametrize("M,K,ld", [(4096, 1280, 1408), (4096, 5120, 5120)])
def test_column_stats_kernel(M, K, ld):
    lib = _lib()
    R = lib.samrs_k_audit_rows_per_partial()
    assert 1 < R <= 256
    gen = torch.Generator().manual_seed(11)
    # f16 values log-uniform over 2^-20 .. 2^15, random signs; pad columns (never read) hold the saturation pattern
    mag = torch.exp2(torch.rand(M, K, generator=gen, dtype=torch.float64) * 35.0 - 20.0)
    sign = torch.where(torch.rand(M, K, generator=gen) < 0.5, -1.0, 1.0).double()
    x = (mag * sign).to(torch.float16)
    full = torch.full((M, ld), 65504.0, dtype=torch.float16)
    full[:, :K] = x
    dev = full.cuda()
    n_slabs = (M + R - 1) // R

    def run(sumsq=None, maxbits=None):
        partials = torch.full((n_slabs, K), float("nan"), dtype=torch.float32, device="cuda")
        sumsq = torch.zeros(K, dtype=torch.float64, device="cuda") if sumsq is None else sumsq
        maxbits = torch.zeros(K, dtype=torch.int32, device="cuda") if maxbits is None else maxbits
        rc = lib.samrs_k_column_stats(PREC["f16"], dev.data_ptr(), M, K, ld, partials.data_ptr(), sumsq.data_ptr(), maxbits.data_ptr(), _stream())
        assert rc == 0
        torch.cuda.synchronize()
        return sumsq, maxbits

    s1, m1 = run()
    s2, m2 = run()
    ref = x.double().square().sum(0)
    want_max = (x.view(torch.int16).to(torch.int32) & 0x7FFF).amax(0)
    assert torch.equal(m1.cpu(), want_max)                                       # the largest magnitude: exact
    rel = ((s1.cpu() - ref).abs() / ref).max().item()
    bound = (R - 1) * 2.0 ** -24          # exact non-negative addends; the one rounding chain is R - 1 sequential fp32 adds per slab
    print(f"column_stats [{M}][{K}] ld {ld}: max relative error of the sum of squares {rel:.3e} (bound {bound:.3e}, R = {R})")
    assert rel <= bound
    assert torch.equal(s1.view(torch.int64), s2.view(torch.int64)) and torch.equal(m1, m2)   # two runs: the same bits
    s3, m3 = run(s1.clone(), m1.clone())                                         # a second call accumulates
    drel = ((s3 - 2 * s1).abs() / s1).max().item()
    assert drel <= n_slabs * 2.0 ** -52 and torch.equal(m3, m1)                   # n_slabs fp64 adds of half an ulp each


# ---- engine --------------------------------------------------------------------------------------------------------------------------
def _sam(sd, precision="f16", options=None, name="vit_tiny", **kw):
    import samrs_amd
    kw.setdefault("max_prompts", 8)
    kw.setdefault("max_points", 1)
    return samrs_amd.sam_model_registry[name](state_dict=sd, precision=precision, options=options, **kw).to("cuda")


def _tile(i):
    return torch.as_tensor(synth.make_image(i), device="cuda")[None].contiguous()


def _site_sizes(cfg, n_img=1):
    D, t = cfg.embed_dim, 4096 * n_img
    per_block = [t * D] * 6 + [t * 4 * D]
    return per_block * cfg.depth + [t * D, t * 256, t * 256]


def _check_rows(rows, cfg, passes=1, n_img=1):
    assert rows.shape == (7 * cfg.depth + 3, 48)
    assert rows[:, 0].tolist() == [passes * s for s in _site_sizes(cfg, n_img)]
    assert np.array_equal(rows[:, 1] + rows[:, 4] + rows[:, 8:].sum(1), rows[:, 0])          # the invariant, every site
    assert not rows[:, 6:8].any()


def test_profile_agrees_with_the_saturation_counter_and_changes_no_output():
    import samrs_amd
    cfg = synth.CONFIGS["vit_tiny"]
    sd = synth.make_state_dict(cfg, 0)
    sam = _sam(sd, options={"outlier_cols": 0, "range_check": 1, "range_profile": 1})
    plain = _sam(sd, options={"outlier_cols": 0})
    eng = sam.engine
    sites = eng.audit_sites()
    assert len(sites) == 7 * cfg.depth + 3
    assert [n for n, _ in sites[:7]] == [f"blocks.0.{s}" for s in ("qkv_in", "q", "k", "v", "proj_in", "lin1_in", "lin2_in")]
    assert [n for n, _ in sites[-3:]] == ["neck.conv1_in", "neck.conv2_in", "decoder.keys0"]
    D = cfg.embed_dim
    assert [k for _, k in sites[:7]] == [D, 0, 0, 0, D, D, 4 * D] and [k for _, k in sites[-3:]] == [0, 0, 0]
    assert not eng.range_profile().any()                                          # nothing profiled yet
    with pytest.raises(AssertionError, match="range_profile"):
        eng.column_stats("blocks.0.qkv_in")                                       # mode 1 keeps no column statistics
    with pytest.raises(AssertionError, match="no column statistics"):
        eng.column_stats("blocks.0.q")
    img = synth.make_image(0)
    boxes = torch.from_numpy(synth.C1_BOXES).cuda()
    out = []
    for s in (sam, plain):
        pred = samrs_amd.SamPredictor(s)
        pred.set_image(img)
        tb = pred.transform.apply_boxes_torch(boxes, img.shape[:2])
        m, iou, low = pred.predict_torch(None, None, tb, None, multimask_output=False)
        out.append((pred.get_image_embedding().clone(), m.clone(), low.clone()))
    rows = eng.range_profile()
    _check_rows(rows, cfg)
    assert int((rows[:, 3] + rows[:, 4]).sum()) == eng.get_option("saturated")    # the unchanged counter is the yardstick
    for a, b in zip(out[0], out[1]):
        assert torch.equal(a, b)
    again = eng.range_profile(reset=True)
    assert np.array_equal(again, rows) and not eng.range_profile().any()
    assert plain.engine.get_option("range_profile") == 0 and not plain.engine.range_profile().any()
    eng.close()
    plain.engine.close()


def test_saturation_is_located():
    cfg = synth.CONFIGS["vit_tiny"]
    sd = synth.heavy_tailed(synth.make_state_dict(cfg, 0), cfg, 0, **OUTSIDE)
    sam = _sam(sd, options={"outlier_cols": 0, "range_check": 1, "range_profile": 1})
    eng = sam.engine
    eng.set_images(_tile(0))
    rows = eng.range_profile()
    _check_rows(rows, cfg)
    names = [n for n, _ in eng.audit_sites()]
    sat = [n for n, r in zip(names, rows) if r[3] + r[4] > 0]
    print("saturated sites:", {n: int(rows[names.index(n)][3] + rows[names.index(n)][4]) for n in sat})
    print(audit.format_report({"precision": "f16", "passes": 1, "sites": audit.site_report(names, rows, "f16"), "gemms": [], "findings": []}))
    assert "blocks.0.v" in sat and "blocks.0.lin2_in" in sat and sat[0] == "blocks.0.v"
    allowed = {f"blocks.{b}.{s}" for b in (0, 1) for s in ("v", "proj_in", "lin2_in")}
    assert set(sat) <= allowed, sat
    total = int((rows[:, 3] + rows[:, 4]).sum())
    assert total > 0 and total == eng.get_option("saturated")
    findings = audit.verdict({"precision": "f16", "sites": audit.site_report(names, rows, "f16"), "gemms": []})
    assert findings[0]["kind"] == "SATURATED" and findings[0]["sites"][0][0] == "blocks.0.v"
    eng.close()
    # the same weights on bf16 operands: nothing saturates (the documented remedy)
    sam = _sam(sd, precision="bf16", options={"range_profile": 1})
    sam.engine.set_images(_tile(0))
    rows = sam.engine.range_profile()
    _check_rows(rows, cfg)
    assert not (rows[:, 3] + rows[:, 4]).any()
    sam.engine.close()


def _planted(cfg, seed=0, n_channels=4):
    """The channels synth.heavy_tailed plants, per block: its generator replayed."""
    gen = torch.Generator().manual_seed(424242 + seed)
    D, H = cfg.embed_dim, cfg.mlp_ratio * cfg.embed_dim
    out = {}
    for i in sorted({0, cfg.depth // 2, cfg.depth - 1}):
        hid = torch.randperm(H, generator=gen)[:n_channels]
        vch = torch.randperm(D, generator=gen)[:n_channels]
        gch = torch.randperm(D, generator=gen)[:n_channels]
        out[i] = {"qkv": sorted(gch.tolist()), "lin1": sorted(gch.tolist()), "lin2": sorted(hid.tolist()), "proj": sorted(vch.tolist())}
    return out


@pytest.fixture(scope="module")
def inside_run():
    """vit_tiny, heavy-tailed weights inside the f16 range, tile 0: one encoder pass with "range_profile" = 2 (outlier treatment on, and
    off at build time), and the fp32 oracle's operand tensors of the global block (block 1) through Rounding taps."""
    from oracle import sam_oracle as so
    cfg = synth.CONFIGS["vit_tiny"]
    sd = synth.heavy_tailed(synth.make_state_dict(cfg, 0), cfg, 0, **INSIDE)
    runs = {}
    for label, opts in (("on", {"range_profile": 2}), ("off", {"range_profile": 2, "outlier_cols": 0})):
        sam = _sam(sd, options=opts)
        sam.engine.set_images(_tile(0))
        runs[label] = audit.collect(sam.engine, sd, cfg, 1)
        runs[label]["rows"] = sam.engine.range_profile()
        runs[label]["cols"] = {g: sam.engine.column_stats(f"blocks.1.{audit.GEMM_SITE[g]}") for g in outliers.GEMMS}
        sam.engine.close()
    seen = []

    def tap(name):
        def f(x):
            seen.append((rd.cur_block, name, x.detach()))
            return x
        return f
    rd = so.Rounding(points={p: tap(p) for p in ("enc.qkv_in", "enc.qkv_out", "enc.proj_in", "enc.lin1_in", "enc.lin2_in")}, block_points={})
    with torch.no_grad():
        so.image_encoder(sd, cfg, so.preprocess(synth.make_image(0)), rd)
    blk = [(n, x) for b, n, x in seen if b == 1]
    acts = {n: [x for m, x in blk if m == n and x.dim() > 2] for n in ("enc.qkv_in", "enc.proj_in", "enc.lin1_in", "enc.lin2_in")}
    assert all(len(v) == 1 for v in acts.values())           # a point sees its GEMM's weight (2-D) and its activation
    qkv_out = [x for m, x in blk if m == "enc.qkv_out"]
    assert len(qkv_out) == 3                                 # q, k, v in that order
    oracle = {"qkv_in": acts["enc.qkv_in"][0], "v": qkv_out[2], "proj_in": acts["enc.proj_in"][0], "lin1_in": acts["enc.lin1_in"][0],
              "lin2_in": acts["enc.lin2_in"][0]}
    return cfg, sd, runs, oracle


def test_headroom_matches_the_oracle(inside_run):
    cfg, sd, runs, oracle = inside_run
    rep = {s["site"]: s for s in runs["on"]["sites"]}
    _check_rows(runs["on"]["rows"], cfg)
    left_out = []
    for site, t in oracle.items():
        mx = t.abs().max().item()
        want = math.floor(math.log2(mx))
        frac = mx / 2.0 ** round(math.log2(mx))
        got = rep[f"blocks.1.{site}"]
        print(f"blocks.1.{site}: oracle max {mx:.5g} (floor log2 {want}), engine top bin {got['top_log2']}, largest {got['largest']:.5g}, "
              f"headroom {got['headroom_bits']:.2f} bit")
        if abs(frac - 1.0) < 0.005:
            left_out.append(site)
            continue
        assert got["top_log2"] == want, (site, mx, got)
    assert len(left_out) <= 1, left_out
    assert not any(s["saturated"] + s["inf_nan"] for s in runs["on"]["sites"])


def test_measured_columns_match_the_oracle_and_the_engine_picks(inside_run):
    cfg, sd, runs, oracle = inside_run
    planted = _planted(cfg)
    by = {(g["block"], g["gemm"]): g for g in runs["on"]["gemms"]}
    assert len(by) == 4 * cfg.depth
    for g in outliers.GEMMS:
        t = oracle[audit.GEMM_SITE[g]]
        a = t.reshape(-1, t.shape[-1]).double()
        rms_o = a.square().mean(0).sqrt()
        w = sd[f"image_encoder.blocks.1{audit.GEMM_WEIGHT[g]}"].double()
        picks_o, _ = outliers.pick(rms_o * w.norm(dim=0))
        st = runs["on"]["cols"][g]
        assert st["n_rows"] == 4096
        rms_e = torch.from_numpy(np.sqrt(st["sumsq"] / st["n_rows"]))
        rel = ((rms_e[picks_o] - rms_o[picks_o]).abs() / rms_o[picks_o]).max().item()
        mx_rel = abs(float(st["max_abs"].max()) - a.abs().max().item()) / a.abs().max().item()
        print(f"block 1 {g}: oracle-measured picks {picks_o.tolist()}, engine-measured {by[(1, g)]['measured_picks']}, engine picks "
              f"{by[(1, g)]['engine_picks']}; per-column rms vs oracle on the picks: max rel {rel:.2e}; largest magnitude rel {mx_rel:.2e}")
        assert rel <= 0.01
        assert by[(1, g)]["measured_picks"] == by[(1, g)]["engine_picks"] == planted[1][g] == picks_o.tolist()
    for i in range(cfg.depth):
        for g in outliers.GEMMS:
            assert by[(i, g)]["measured_picks"] == by[(i, g)]["engine_picks"] == planted[i][g], (i, g, by[(i, g)])
    assert not [f for f in runs["on"]["findings"] if f["kind"] == "UNCOVERED_OUTLIERS"]
    # built with the outlier treatment off, the same columns are measured, none is treated: all reported
    unc = {(f["block"], f["gemm"]): f for f in runs["off"]["findings"] if f["kind"] == "UNCOVERED_OUTLIERS"}
    for i in range(cfg.depth):
        for g in outliers.GEMMS:
            assert unc[(i, g)]["columns"] == planted[i][g] and unc[(i, g)]["mass_share"] > 0.5, (i, g)


def test_audit_passes_switch_themselves_off():
    import samrs_amd
    cfg = synth.CONFIGS["vit_tiny"]
    sd = synth.make_state_dict(cfg, 0)
    sam, never = _sam(sd), _sam(sd)
    eng = sam.engine
    assert eng.get_option("audit_passes") == 0 and eng.get_option("range_profile") == 0
    eng.set_option("audit_passes", 2)
    assert eng.get_option("range_profile") == 2
    eng.set_images(_tile(0))
    assert eng.get_option("audit_passes") == 1 and eng.get_option("range_profile") == 2
    eng.set_images(_tile(1))
    assert eng.get_option("audit_passes") == 0 and eng.get_option("range_profile") == 0
    eng.set_images(_tile(2))
    never.engine.set_images(_tile(2))
    assert torch.equal(eng.get_embedding(0), never.engine.get_embedding(0))
    rows = eng.range_profile()
    _check_rows(rows, cfg, passes=2)
    assert eng.column_stats("blocks.1.lin2_in")["n_rows"] == 2 * 4096
    eng.set_option("audit_passes", 1)                       # a new audit starts from zero
    assert not eng.range_profile().any()
    eng.set_option("audit_passes", 0)
    assert eng.get_option("range_profile") == 0
    eng.close()
    never.engine.close()
    # through the registry: the first pass is profiled, then the host reads the profile once and warns by name
    out = synth.heavy_tailed(sd, cfg, 0, **OUTSIDE)
    sam = samrs_amd.sam_model_registry["vit_tiny"](state_dict=out, audit_passes=1).to("cuda")
    pred = samrs_amd.SamPredictor(sam)
    with pytest.warns(audit.OperandRangeWarning, match=r"blocks\.0\.v"):
        pred.set_image(synth.make_image(0))
    assert sam.audit_report is not None and audit.exit_code(sam.audit_report) == 2
    assert sam.engine.get_option("range_profile") == 0
    with warnings.catch_warnings():
        warnings.simplefilter("error", audit.OperandRangeWarning)
        pred.set_image(synth.make_image(1))                 # nothing is read or said again
    sam.engine.close()
    sam = samrs_amd.sam_model_registry["vit_tiny"](state_dict=sd, audit_passes=1).to("cuda")
    with warnings.catch_warnings():
        warnings.simplefilter("error", audit.OperandRangeWarning)
        samrs_amd.SamPredictor(sam).set_image(synth.make_image(0))
    assert sam.audit_report is not None and audit.exit_code(sam.audit_report) == 0
    sam.engine.close()


def _child(args, timeout=600):
    return subprocess.run([sys.executable, "-m", "samrs_amd.audit"] + args, cwd=ROOT, timeout=timeout, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True)


def test_audit_cli_exit_status_gates_a_run(tmp_path):
    cfg = synth.CONFIGS["vit_tiny"]
    sd = synth.make_state_dict(cfg, 0)
    torch.save(synth.heavy_tailed(sd, cfg, 0, **OUTSIDE), tmp_path / "out.pth")
    torch.save(sd, tmp_path / "seeded.pth")
    r = _child(["--model", "vit_tiny", "--checkpoint", str(tmp_path / "out.pth"), "--synthetic", "2", "--passes", "1", "--json", str(tmp_path / "f.json")])
    print(r.stdout[-3000:])
    assert r.returncode == 2, r.stdout[-2000:]
    rep = json.loads((tmp_path / "f.json").read_text())
    sat = [f for f in rep["findings"] if f["kind"] == "SATURATED"]
    assert sat and sat[0]["sites"][0][0] == "blocks.0.v" and "blocks.0.lin2_in" in [n for n, _ in sat[0]["sites"]]
    assert "SATURATED" in r.stdout and "blocks.0.v" in r.stdout
    r = _child(["--model", "vit_tiny", "--checkpoint", str(tmp_path / "seeded.pth"), "--synthetic", "2", "--passes", "1"])
    assert r.returncode == 0, r.stdout[-2000:]


def test_generate_audit_passes_writes_the_same_files_plus_the_report(tmp_path):
    from samrs_amd import generate, tile_io
    img_dir = tmp_path / "img"
    img_dir.mkdir()
    ann = {}
    for i, (h, w) in enumerate([(1024, 1024), (600, 800), (1024, 1024)]):
        tile_io.write_rgb(str(img_dir / f"P{i:04d}.png"), synth.make_image(70 + i, h, w), 1)
        b, l = synth.make_boxes(70 + i, 23, h, w)
        ann[f"P{i:04d}"] = {"boxes": b.tolist(), "labels": l.tolist()}
    (tmp_path / "boxes.json").write_text(json.dumps(ann))

    def args(out, **kw):
        a = dict(images=str(img_dir), boxes=str(tmp_path / "boxes.json"), out=str(out), model="vit_tiny", checkpoint=None, precision="f16",
                 classes=None, n_classes=18, palette=None, box_batch=20, no_rle=False, batch=2)
        a.update(kw)
        return generate.argparse.Namespace(**a)

    def tree(d):
        return {os.path.relpath(os.path.join(p, f), d): open(os.path.join(p, f), "rb").read() for p, _, fs in os.walk(d) for f in fs}
    s0 = generate.run(args(tmp_path / "plain"))
    s1 = generate.run(args(tmp_path / "audited", audit_passes=1))
    assert s0 == s1
    t0, t1 = tree(tmp_path / "plain"), tree(tmp_path / "audited")
    extra = os.path.join("statistic", "audit.json")
    assert sorted(t1) == sorted(list(t0) + [extra])
    for k in t0:
        assert t0[k] == t1[k], k
    rep = json.loads(t1[extra])
    cfg = synth.CONFIGS["vit_tiny"]
    assert rep["passes"] == 1 and len(rep["sites"]) == 7 * cfg.depth + 3 and rep["sites"][0]["elements"] == 2 * 4096 * cfg.embed_dim
    assert not [f for f in rep["findings"] if f["kind"] == "SATURATED"]


def test_vit_h_two_tiles_report():
    """The shape the feature exists for: rows padded to 1408 elements, lin2's operand at 42 MB per tile."""
    cfg = synth.CONFIGS["vit_h"]
    sd = synth.make_state_dict(cfg, 0)
    sam = _sam(sd, name="vit_h", max_images=2, options={"range_profile": 2})
    eng = sam.engine
    t = torch.as_tensor(np.stack([synth.make_image(0), synth.make_image(1)]), device="cuda").contiguous()
    eng.set_images(t)
    rows = eng.range_profile()
    _check_rows(rows, cfg, n_img=2)
    assert rows.shape[0] == 7 * 32 + 3 and not (rows[:, 3] + rows[:, 4]).any()
    rep = audit.collect(eng, sd, cfg, 1)
    assert len(rep["gemms"]) == 4 * cfg.depth and all(s["consistent"] for s in rep["sites"])
    assert not [f for f in rep["findings"] if f["kind"] in ("SATURATED", "TIGHT")]
    text = audit.format_report(rep)
    print(text)
    assert "blocks.31.lin2_in" in text and "decoder.keys0" in text
    eng.close()

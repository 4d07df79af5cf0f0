#!/usr/bin/env python
"""bench.py -- SAM box->mask throughput on MI355X (BASELINE.json metric).

  python bench.py --gpus N --steps K --warmup W [--workload c2|c3|c4]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
         --master-port P bench.py --gpus N --steps K --warmup W

The timed loop IS the product loop: ``samrs_amd.driver.TilePipeline`` (what ``python -m samrs_amd.generate``
runs) -- batches of 8 x 1024^2 uint8 tiles through one ViT-H encoder pass, decode + ordered painting + transfers of
batch k-1 overlapped with the encoder of batch k on separate HIP streams.  One "step" = one 8-tile batch per rank.

  c2 (default, BASELINE.json configs[1]): 32 hboxes per tile in one box-only ``predict`` (multimask_output=False),
     thresholded full-resolution masks [32, 1, 1024, 1024] in HBM, painted class map + per-box areas to the host.
     ``value`` is measured with the tiles resident in HBM when the timed region starts (the pipeline's H2D stage
     degenerates to a device copy); ``pcie_inclusive`` is the SAME loop with the tiles starting in pinned host memory;
     ``cli_inclusive`` is ``samrs_amd.generate.run`` from PNG files on disk to gray / color PNG + pickle files on disk.
  c3 (configs[2]): DOTA-v2-shaped stream -- box counts per tile long-tailed (geometric, mean 32, cap 400), decoded in
     the reference's 20-box chunks, tiles handed to the ranks by a shared-counter work queue (driver.WorkQueue).
  c4 (configs[3]): instance path -- 32 FAIR1M-shaped rotated boxes per tile, enclosing-hbox prompt (or --c4-prompt
     rbox_mask: GPU-rasterised mask prompt), multimask_output=True, best-of-3 by predicted IoU.

Image-parallel: every rank runs its own replica, no collective on the data path (weak scaling); the only collective
is the final int64 statistics all-reduce, outside the step.  Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times --steps steps and prints the line (`value`, `ms_per_step` = milliseconds of one timed
step).  --full adds everything else the line can carry: the in-situ roofline of the dominant kernel, the secondary legs
(RLE-inclusive, PCIe-inclusive, the other operand-split mode, bf16, the all-split mode, the generation CLI, the reference's
20-box chunks), the CPU / torch-eager baselines and the committed parity figures; in a plain run those keys are null.
--dump-outputs DIR writes what the timed path handed its caller in the last timed step (rank 0) as DIR/<name>.npy
(float32 / float64): seg_mask [tiles, H, W] (class ids, 255 = unlabeled; c2 / c3), areas and quality (concatenated over the
tiles; quality for c4), boxes_per_tile and tile_index.  Inputs are seeded, so two builds can be compared file for file.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC only on this pool (RCCL needs it)

PEAK_MFMA_TFLOPS = 2500.0      # dense bf16/f16 MFMA, MI355X_MICROARCH.md chip table
PEAK_HBM_GBS = 8000.0
PMC_FILE = os.path.join(ROOT, "profiles", "dominant_kernel_pmc.json")


def flops_per_image(cfg, n_boxes: float) -> float:
    """Algorithmic FLOPs: padded query rows excluded, padded keys included."""
    D, depth, g, ws = cfg.embed_dim, cfg.depth, cfg.grid, cfg.window_size
    N = g * g
    n_glob = len(cfg.global_attn_indexes)
    n_win = depth - n_glob
    patch = 2.0 * N * D * 3 * cfg.patch_size ** 2
    lin = 2.0 * N * D * D * (3 + 1 + 4 + 4) * depth
    win_attn = n_win * 2.0 * 2.0 * N * (ws * ws) * D                # QK^T + PV, real queries x 196 keys
    win_rel = n_win * 2.0 * N * D * 2 * ws
    glb_attn = n_glob * 2.0 * 2.0 * N * N * D
    glb_rel = n_glob * 2.0 * N * D * 2 * g
    neck = 2.0 * N * D * 256 + 2.0 * N * 9 * 256 * 256
    enc = patch + lin + win_attn + win_rel + glb_attn + glb_rel + neck
    return enc + n_boxes * 3.623e9


def file_sha(path: str) -> str:
    return hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]


PARITY_FILE = os.path.join(ROOT, "profiles", "parity_stats.json")


def csrc_sha() -> str:
    """One hash over every device source the arithmetic of the path lives in (samrs_amd/csrc/*.hip, *.h): what a parity
    statement is a statement ABOUT.  tests/test_parity_gpu.py::test_vit_h_statistical_parity_sample writes the same hash
    next to the statistics it measures."""
    d = os.path.join(ROOT, "samrs_amd", "csrc")
    h = hashlib.sha256()
    for name in sorted(os.listdir(d)):
        if name.endswith((".hip", ".h")):
            h.update(name.encode())
            h.update(open(os.path.join(d, name), "rb").read())
    return h.hexdigest()[:16]


def parity_of_mode(split: int, workload: str, model: str = "vit_h"):
    """The parity figures that belong to the precision mode a bench line was produced in (VERDICT r04 "what's weak" 1: the
    line carried a throughput with no parity attached).  Read from profiles/parity_stats.json = the JSON the GPU test
    test_vit_h_statistical_parity_sample wrote on an MI355X (engine vs the pinned oracle, oracle/parity_sample.py), and reported
    only when it was measured on THIS build's device sources (hash-pinned like `roofline.traffic`)."""
    if model != "vit_h" or not os.path.exists(PARITY_FILE):
        return {"mode": split, "note": "no parity sample committed for this model"}
    st = json.load(open(PARITY_FILE))
    if st.get("csrc_sha16") != csrc_sha():
        return {"mode": split, "note": "profiles/parity_stats.json was measured on other device sources: not reported"}
    m = st.get("summary", {}).get(str(split))
    if not m:
        return {"mode": split, "note": f"profiles/parity_stats.json holds no sample for split {split}"}
    c4 = [m[t] for t in ("c4box", "c4mask") if t in m]
    out = {"mode": split, "vs": "oracle/sam_oracle.py fp32 (pinned to the real reference's fixtures), same seeded inputs",
           "c2_iou_min": round(m["c2"]["iou_min"], 5), "c2_n_masks": m["c2"]["n_masks"],
           "classmap_px_mean": m["c2"]["classmap_diff_mean"], "classmap_px_max": m["c2"]["classmap_diff_max"],
           "classmap_px_outside_unstable": m["c2"]["classmap_diff_outside_unstable"],
           "classmap_bit_identical": m["c2"]["classmap_diff_max"] == 0,
           "c4_iou_min": round(min(t["iou_min"] for t in c4), 5) if c4 else None,
           "c4_n_masks": sum(t["n_masks"] for t in c4), "c4_served_in_this_mode": bool(split & (64 | 16)),
           "n_masks": sum(t["n_masks"] for t in m.values()), "flips_outside_tau": sum(t["flips_outside_tau"] for t in m.values()),
           "tau_frac": st.get("tau_frac"), "csrc_sha16": st.get("csrc_sha16"), "device": st.get("device")}
    # round 6: (a) the floor -- the fp32 oracle itself on two backends (torch eager on the MI355X vs the host CPU, same 8 C2 tiles);
    # (b) checkpoint-like weights -- synth.heavy_tailed at ViT-H on the C2 fixture inputs (tests/test_outlier_gpu.py)
    fl = st.get("reference_backend_floor", {}).get("c2")
    if fl:
        out["reference_backend_floor_px"] = {"classmap_px_mean": fl["classmap_diff_mean"], "classmap_px_max": fl["classmap_diff_max"],
                                             "mask_flips_max": fl["flips_max"], "iou_min": round(fl["iou_min"], 6), "n_masks": fl["n_masks"],
                                             "what": "oracle fp32 in torch eager on this GPU vs on the host CPU"}
        out["classmap_px_over_floor"] = round(out["classmap_px_mean"] / max(fl["classmap_diff_mean"], 1e-9), 1)
    ht = st.get("heavy_tailed", {})
    key = f"mode{split}_on"
    if ht.get("csrc_sha16") == st.get("csrc_sha16") and key in ht.get("three_blocks", {}):
        out["heavy_tailed_iou_min"] = round(ht["three_blocks"][key]["iou_min"], 5)
        if key in ht.get("every_block", {}):
            out["heavy_tailed_every_block_iou_min"] = round(ht["every_block"][key]["iou_min"], 5)
        out["heavy_tailed_encoder_cost"] = {k: round(ht[k]["encoder_ms_8_tiles"]["cost"], 4) for k in ("three_blocks", "every_block") if k in ht}
        smp = ht.get("sample_every_block", {}).get(str(split))
        if smp:          # the statistical sample on the every-block weights (tests/test_outlier_gpu.py::test_heavy_tailed_statistical_sample)
            out["heavy_tailed_sample"] = {"c2_iou_min": round(smp["c2"]["iou_min"], 5), "c2_n_masks": smp["c2"]["n_masks"],
                                          "c4_iou_min": round(min(smp["c4box"]["iou_min"], smp["c4mask"]["iou_min"]), 5),
                                          "c4_n_masks": smp["c4box"]["n_masks"] + smp["c4mask"]["n_masks"],
                                          "c4_below_0999": smp["c4box"]["n_below_0999"] + smp["c4mask"]["n_below_0999"],
                                          "classmap_px_mean": smp["c2"]["classmap_diff_mean"]}
    if workload == "c4":
        out["headline_workload_iou_min"] = out["c4_iou_min"]
    else:
        out["headline_workload_iou_min"] = out["c2_iou_min"]
    return out


def _cpu_quota():
    """CPUs this container may use at once (cgroup v2 cpu.max), or None."""
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        return None if q == "max" else round(int(q) / int(p), 1)
    except Exception:
        return None


def _cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except Exception:
        pass
    return "unknown"


DUMP_BUDGET = 48 << 20           # bytes of seg_mask in float32 (the other arrays are a few KB)


def dump_outputs(out_dir: str, results) -> None:
    """--dump-outputs: the sink's copies of the last timed batch, (key, seg_mask, areas, quality) per tile, as .npy files.  A class-map
    stack larger than DUMP_BUDGET (batches above 8 tiles of 1024^2) is written as a fixed sample: the pixels at flat positions drawn
    once with numpy's default_rng(0), sorted, as seg_mask_sample.npy."""
    assert results, "--dump-outputs: the timed region handed no batch to the sink"
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"tile_index": np.array([float(k) for k, _, _, _ in results]),
              "boxes_per_tile": np.array([float(len(a)) for _, _, a, _ in results]),
              "areas": np.concatenate([a for _, _, a, _ in results]).astype(np.float64)}
    if all(q is not None for _, _, _, q in results):
        arrays["quality"] = np.concatenate([q for _, _, _, q in results]).astype(np.float32)
    if all(s is not None for _, s, _, _ in results) and len({s.shape for _, s, _, _ in results}) == 1:
        seg = np.stack([s for _, s, _, _ in results]).astype(np.float32)
        if seg.nbytes <= DUMP_BUDGET:
            arrays["seg_mask"] = seg
        else:
            idx = np.sort(np.random.default_rng(0).choice(seg.size, DUMP_BUDGET // 4, replace=False))
            arrays["seg_mask_sample"] = seg.reshape(-1)[idx]
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    print(f"[bench] --dump-outputs: {', '.join(f'{k} {list(v.shape)}' for k, v in arrays.items())} -> {out_dir}", file=sys.stderr, flush=True)


def _self_launch(n: int) -> None:
    """`python bench.py --gpus N` with N > 1 and no launcher around it: become the launcher.  Re-runs this same command line
    under `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port <free>` (one
    rank per GPU, RCCL) and exits with its status; rank 0's JSON line is the only thing on stdout.  The N = 1 path and a launch
    that already comes from torchrun (WORLD_SIZE set) never get here."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print(f"[bench] --gpus {n} without a launcher: re-executing under torch.distributed.run on 127.0.0.1:{port}", file=sys.stderr, flush=True)
    sys.exit(subprocess.call(cmd))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50, help="timed 8-tile steps (50 x ~56 ms: long enough for the socket's power / clock "
                    "steady state, which the loop runs at)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tile-pool", type=int, default=64, help="distinct synthetic tiles per rank rotated through the timed region")
    ap.add_argument("--workload", default="c2", choices=["c2", "c3", "c4"])
    ap.add_argument("--model", default="vit_h")
    ap.add_argument("--dtype", default="f16", choices=["f16", "bf16"],
                    help="MFMA operand type; f16 is the precision that meets the IoU>=0.999 parity bar (DESIGN.md)")
    ap.add_argument("--batch", type=int, default=8, help="tiles per encoder pass")
    ap.add_argument("--boxes", type=int, default=32, help="boxes per tile (c3: the mean of the long-tailed distribution)")
    ap.add_argument("--c4-prompt", default="box", choices=["box", "rbox_mask"])
    ap.add_argument("--box-batch", type=int, default=0,
                    help="c3: boxes per predict call (default 64 = the product's chunking, samrs_amd.generate --box-batch; the masks do "
                         "not depend on it: test_predict_batches_beyond_max_prompts.  The reference's 20, main_sam_hbox_semantic.py:91, "
                         "is timed beside it as `reference_chunking`)")
    ap.add_argument("--weights", default="normal", choices=["normal", "heavy_tailed", "heavy_tailed_every_block"],
                    help="normal: seeded N(0, sigma) weights (the headline).  heavy_tailed: synth.heavy_tailed on top (outlier LayerNorm gammas / "
                         "hidden units / v channels in the first, middle and last block, or in every block): what the engine's outlier-column "
                         "extension costs in the product loop (DESIGN.md 2)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-alt-dtype", action="store_true", help="skip the second (bf16) timing leg")
    ap.add_argument("--no-pcie-leg", action="store_true", help="skip the PCIe-inclusive measurement")
    ap.add_argument("--no-fast-leg", action="store_true", help="skip the measurement of the other operand-split mode (15 <-> 79)")
    ap.add_argument("--no-cli-leg", action="store_true", help="skip the end-to-end run of the generation CLI (PNG files in, files out)")
    ap.add_argument("--cli-tiles", type=int, default=320, help="tiles of the CLI leg")
    ap.add_argument("--no-rle-leg", action="store_true", help="skip the RLE-inclusive measurement (the reference's full output contract)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline does not need: the dominant kernel's in-situ roofline, the secondary "
                         "legs and baselines above (each --no-* flag still turns its own off) and the parity figures")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the arrays the timed path returned in its last timed step as DIR/<name>.npy (float32 / float64)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        _self_launch(args.gpus)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    # test hook for 1-GPU boxes: SAMRS_BENCH_SHARE_GPU=1 puts every rank on cuda:0 and uses gloo, which
    # exercises the N>1 control flow (barriers, MAX-over-ranks timing, work queue, statistics all-reduce)
    share = os.environ.get("SAMRS_BENCH_SHARE_GPU") == "1"
    if share:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # host threads: the weight synthesis below is torch-CPU work; N ranks x every hardware thread of the node oversubscribes a
    # container whose CPU quota is a fraction of it (16 of 256 on the pool's boxes)
    torch.set_num_threads(max(1, min(32, int((_cpu_quota() or len(os.sched_getaffinity(0))) // max(1, world)))))
    dist = None
    if world > 1:
        import torch.distributed as dist
        if share:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)  # nccl == RCCL on ROCm

    import samrs_amd
    from samrs_amd import driver, synth

    cfg = synth.CONFIGS[args.model]
    sd = synth.make_state_dict(cfg, 0)
    if args.weights != "normal":
        sd = synth.heavy_tailed(sd, cfg, 0, hidden_scale=3e3, v_scale=3e3, gamma_scale=30.0,
                                blocks=list(range(cfg.depth)) if args.weights == "heavy_tailed_every_block" else None)
    B = args.batch
    n_classes = 37 if args.workload == "c4" else 18
    # a pool of distinct synthetic tiles per rank (host, pinned) and their device copies: the timed region walks through all of
    # them (round 3 re-fed the same 8 tiles every step)
    n_pool = max(B, args.tile_pool)
    host_tiles = torch.stack([torch.from_numpy(synth.make_noise_image(rank * 1000 + i)) for i in range(n_pool)]).pin_memory()
    dev_tiles = host_tiles.to(dev)

    if args.workload == "c3":
        # the product's chunking (generate.py --box-batch 64); chunking is proven bit-irrelevant, so the reference's 20-box chunks
        # (main_sam_hbox_semantic.py:91) are a side leg, not the workload's definition (VERDICT r04 "what's weak" 10)
        box_batch, max_boxes = (args.box_batch or 64), 400
    else:
        box_batch, max_boxes = args.boxes, args.boxes

    def annotations(global_index: int):
        """Boxes + labels of tile `global_index` of the synthetic stream."""
        if args.workload == "c2":
            return synth.make_boxes(global_index, args.boxes)
        return synth.make_rboxes(global_index, args.boxes)

    total_tiles_hint = world * B * (args.steps + args.warmup) + 64
    if args.workload == "c3":
        counts_all = synth.long_tailed_box_counts(total_tiles_hint, seed=0, mean=float(args.boxes))
        ann_cache = {}

        def annotations(global_index: int):                  # noqa: F811  (cached: the counts come from one draw)
            if global_index not in ann_cache:
                ann_cache[global_index] = synth.make_boxes(global_index, int(counts_all[global_index]))
            return ann_cache[global_index]

    def make_pipe(sam, device_inputs, rle=False, chunk=None):
        if args.workload == "c4":
            return driver.InstancePipeline(sam, n_classes, prompt=args.c4_prompt, batch=B, box_batch=box_batch,
                                           max_boxes=max_boxes, device_inputs=device_inputs, rle=rle, rle_buffer_mb=512)
        return driver.TilePipeline(sam, n_classes, batch=B, box_batch=chunk or box_batch, max_boxes=max_boxes,
                                   device_inputs=device_inputs, rle=rle, rle_buffer_mb=512)

    def make_pipeline(precision, device_inputs):
        sam = samrs_amd.sam_model_registry[args.model](state_dict=sd, precision=precision, max_images=2 * B,
                                                       max_prompts=box_batch, max_points=1).to(dev)
        return sam, make_pipe(sam, device_inputs)

    counters = {"tiles": 0, "boxes": 0, "rle_bytes": 0}
    # --dump-outputs: once armed, the sink keeps host copies of the results of the last batch (static queue: batch number `last`
    # of this rank; the dynamic queue cannot know which batch is its last, so every batch is copied over the previous one)
    capture = {"armed": False, "batches": 0, "last": None, "results": None}

    def sink(results, release):
        for r in results:
            counters["boxes"] += len(r.labels)
            if r.rle_table is not None:
                counters["rle_bytes"] += int(r.rle_table[:, 1].sum())
        counters["tiles"] += len(results)
        if capture["armed"]:
            capture["batches"] += 1
            if capture["last"] is None or capture["batches"] == capture["last"]:
                capture["results"] = [(r.key, None if r.seg_mask is None else np.array(r.seg_mask), np.array(r.areas),
                                       None if r.quality is None else np.array(r.quality)) for r in results]
        release()

    def run_steps(pipe, n_steps, tiles, first_index, shared_queue=False):
        """n_steps 8-tile batches per rank through the product pipeline."""
        if shared_queue and world > 1:
            wq = driver.WorkQueue(world * n_steps * B, chunk=B, rank=rank, world=world, mode="dynamic",
                                  name=f"bench{first_index}")
        else:
            wq = driver.WorkQueue(world * n_steps * B, chunk=B, rank=rank, world=world, mode="static")

        def batches():
            for s0, s1 in wq:
                items = []
                for g in range(s0, s1):
                    bx, lb = annotations(first_index + g)
                    items.append(driver.WorkItem(first_index + g, tiles[g % len(tiles)], bx, lb))
                yield items
        return pipe.run(batches(), sink)

    def timed(pipe, tiles, steps, warmup, after_warmup=None, shared_queue=False):
        run_steps(pipe, warmup, tiles, 0, shared_queue)
        torch.cuda.synchronize()
        if after_warmup is not None:
            after_warmup()
        counters["tiles"] = counters["boxes"] = counters["rle_bytes"] = 0
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_steps(pipe, steps, tiles, world * warmup * B, shared_queue)
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        tiles_done, boxes_done = counters["tiles"], counters["boxes"]
        if dist is not None:
            t = torch.tensor([dt], dtype=torch.float64, device="cpu" if share else dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = t.item()
            c = torch.tensor([tiles_done, boxes_done], dtype=torch.int64, device="cpu" if share else dev)
            dist.all_reduce(c, op=dist.ReduceOp.SUM)
            tiles_done, boxes_done = int(c[0]), int(c[1])
        return dt, tiles_done, boxes_done

    shared_q = args.workload == "c3"
    sam, pipe = make_pipeline(args.dtype, device_inputs=True)
    eng = sam.engine
    eng_info = {k: eng.get_option(k) for k in ("outlier_cols", "outlier_blocks", "outlier_columns")}
    # --full: the engine brackets every launch of the dominant kernel (MLP lin1+GELU GEMM) with hipEvents on its
    # launch stream; warm-up launches are discarded, so the average below is over the timed region
    if args.full:
        eng.time_dominant_kernel(True)

    def after_warmup():
        if args.full:
            eng.dominant_kernel_time()
        if args.dump_outputs and rank == 0:
            capture.update(armed=True, batches=0, last=None if (shared_q and world > 1) else args.steps)

    dt, tiles_done, boxes_done = timed(pipe, dev_tiles, args.steps, args.warmup, after_warmup=after_warmup, shared_queue=shared_q)
    capture["armed"] = False
    if args.full:
        gemm_ms, gemm_launches, N, K = eng.dominant_kernel_time()
        eng.time_dominant_kernel(False)
    assert tiles_done == world * B * args.steps, (tiles_done, world, B, args.steps)
    value = tiles_done / dt
    boxes_per_tile = boxes_done / max(1, tiles_done)
    if rank == 0:
        print(f"[bench] {args.workload} {args.dtype}: {value:.2f} images/s over {world} GPU(s), {dt / args.steps * 1e3:.1f} ms/step, "
              f"{boxes_per_tile:.1f} boxes/tile", file=sys.stderr, flush=True)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, capture["results"])
    F = flops_per_image(cfg, boxes_per_tile)

    # ---- roofline of the dominant kernel: the MLP lin1+GELU GEMM (57.6 % of encoder FLOPs with lin2),
    # timed in situ over the timed region (see above) ----
    roofline = None
    if args.full:
        M = B * cfg.grid ** 2
        gemm_tflops = 2.0 * M * N * K / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0
        # HBM traffic of that kernel: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this same command
        # (tools/gpu_round.sh pmc), corrected as profiles/README.md describes and committed under profiles/ together with the
        # hash of the kernel source it was measured on -- a number taken on an older kernel is NOT reported.
        traffic, traffic_note = None, "no PMC summary committed for this kernel source"
        if args.model == "vit_h" and B == 8 and os.path.exists(PMC_FILE):
            pmc = json.load(open(PMC_FILE))
            if pmc.get("gemm_hip_sha16") == file_sha(os.path.join(ROOT, "samrs_amd", "csrc", "gemm.hip")):
                traffic, traffic_note = pmc.get("traffic_bytes_per_launch"), pmc.get("source", "profiles/")
            else:
                traffic_note = "profiles/dominant_kernel_pmc.json was measured on an older gemm.hip: not reported"
        roofline = {"bound": "mfma", "kernel": f"gemm_et<{args.dtype}> lin1+GELU M={M} N={N} K={K}",
                    "achieved": round(gemm_tflops, 1), "peak": PEAK_MFMA_TFLOPS, "unit": "TFLOP/s",
                    "frac": round(gemm_tflops / PEAK_MFMA_TFLOPS, 4), "traffic": traffic, "traffic_source": traffic_note,
                    "algorithmic_bytes": 2 * (M * K + N * K + M * N), "avg_launch_ms": round(gemm_ms, 4),
                    "launches_timed": gemm_launches, "algorithmic_flops_per_launch": 2.0 * M * N * K,
                    "whole_path_tflops": round(value / world * F / 1e12, 1),
                    "whole_path_frac": round(value / world * F / 1e12 / PEAK_MFMA_TFLOPS, 4)}

    # ---- the one collective of the path: class statistics all-reduce (outside the timed step) ----
    tot_pix, tot_ins = driver.reduce_statistics(pipe.class_pixels, pipe.class_instances)
    torch.cuda.synchronize()
    # every rank's LOCAL sums beside the reduced ones (all-gather of two int64 per rank): the line itself shows that the
    # all-reduce returned the serial sum of what the ranks painted
    local = torch.stack([pipe.class_pixels.sum(), pipe.class_instances.sum()]).to(torch.int64)
    per_rank = [local.cpu().tolist()]
    if dist is not None:
        lt = local.cpu() if share else local
        got = [torch.zeros_like(lt) for _ in range(world)]
        dist.all_gather(got, lt)
        per_rank = [g.cpu().tolist() for g in got]

    # ---- RLE-inclusive: the reference's FULL per-image output contract (main_sam_hbox_semantic.py:195-216): class map + areas
    # + the COCO RLE string of every instance.  Same loop, rle=True: the strings are encoded on the device (samrs_rle_encode)
    # and only they cross PCIe; the sink receives (offset, length) tables + the byte buffer.  NB: masks of random-init weights
    # are noise-like (~135 k runs per mask, ~140 KB per string; a real mask has a few thousand runs, a few KB).
    rle_leg = None
    if args.full and rank == 0 and world == 1 and not args.no_rle_leg:
        pipe_r = make_pipe(sam, True, rle=True)
        n_r = max(2, args.steps)
        dtr, tr, br = timed(pipe_r, dev_tiles, n_r, 1, shared_queue=False)
        rle_leg = {"value": round(tr / dtr, 3), "unit": "images/s", "steps": n_r, "vs_value": round(tr / dtr / value, 4),
                   "rle_bytes_per_mask": round(counters["rle_bytes"] / max(1, br), 1),
                   "what": "same loop with rle=True: + samrs_rle_encode per predict chunk (bit-pack, run boundaries, counts, "
                           "cocoapi string on the device) + D2H of the packed strings; masks stay in HBM"}
        del pipe_r

    # ---- c3 only: the same stream in the reference's own 20-box chunks (main_sam_hbox_semantic.py:91,157-181) ----
    chunk_leg = None
    if args.full and args.workload == "c3" and rank == 0 and world == 1 and box_batch != 20:
        pipe_c = make_pipe(sam, True, chunk=20)
        n_c = max(2, args.steps)
        dtc, tc, _ = timed(pipe_c, dev_tiles, n_c, 1, shared_queue=False)
        chunk_leg = {"value": round(tc / dtc, 3), "unit": "images/s", "steps": n_c, "box_batch": 20, "vs_value": round(tc / dtc / value, 4),
                     "what": "same loop, predict calls of 20 boxes like the reference's; bit-identical masks"}
        del pipe_c

    # ---- the other precision mode.  The pipelines pick the engine's operand-split mode by output contract (driver.TilePipeline
    # precision="auto"): single-mask output (c2 / c3) = split 15, every block GEMM at the 1x f16 rate (C2 fixtures: IoU >= 0.9995);
    # multimask output (c4) = the engine's ViT-H default, split 79 (+ the v third of qkv and proj of the leading 24 blocks on
    # hi + lo operands: what holds IoU >= 0.999 on the C4 fixtures).  This leg runs the same loop in the mode the headline did NOT use. ----
    other_mode = None
    split_used = pipe.split_mode if pipe.split_mode is not None else eng.get_option("split")
    if args.full and rank == 0 and world == 1 and not args.no_fast_leg and args.model == "vit_h":
        other = 79 if split_used == 15 else 15
        keep_mode, keep_allow = pipe.split_mode, pipe.allow_reduced
        try:
            pipe.split_mode, pipe.allow_reduced = other, True       # the pipeline's own calls run in the other mode (driver._mode)
            n_f = max(2, args.steps)
            dtf, tf, _ = timed(pipe, dev_tiles, n_f, 1, shared_queue=False)
            other_mode = {"value": round(tf / dtf, 3), "unit": "images/s", "steps": n_f, "split": other, "vs_value": round(tf / dtf / value, 4),
                          "note": "same loop in the other operand-split mode (15 = block GEMMs at the 1x rate; 79 = the multimask-grade "
                                  "default of a ViT-H engine, IoU >= 0.999 on the C4 fixtures too); not the headline"}
        except Exception as ex:                                      # e.g. SAMRS_SPLIT without the lo weights of bit 64
            other_mode = {"value": None, "note": f"not available: {ex}"}
        pipe.split_mode, pipe.allow_reduced = keep_mode, keep_allow

    # ---- PCIe-inclusive: the same product loop, tiles start in pinned host memory (3 MiB H2D per tile on its own
    # stream, prefetched one batch ahead); class maps + areas go back either way ----
    pcie = None
    if args.full and rank == 0 and world == 1 and not args.no_pcie_leg:
        del pipe
        pipe_h = make_pipe(sam, False)
        n_p = max(2, args.steps)
        dtp, tp, _ = timed(pipe_h, host_tiles, n_p, 1, shared_queue=False)
        pcie = {"value": round(tp / dtp, 3), "unit": "images/s", "steps": n_p,
                "what": "same TilePipeline loop, tiles start in pinned host memory: H2D 8 x 3 MiB per step prefetched on its own "
                        "stream + encoder + decoder + on-device paint + D2H 8 x 1 MiB class maps and per-box areas"}
        del pipe_h

    alt = None
    if args.full and not args.no_alt_dtype:
        other = "bf16" if args.dtype == "f16" else "f16"
        pipe = None
        del sam, eng
        torch.cuda.empty_cache()
        sam2, pipe2 = make_pipeline(other, device_inputs=True)
        n_a = max(2, args.steps // 2)
        dt2, t2, _ = timed(pipe2, dev_tiles, n_a, 1, shared_queue=False)
        alt = {"dtype": other, "value": round(t2 / dt2, 3),
               "note": "BASELINE.json configs[1] names bf16; bf16 operands miss the IoU >= 0.999 bar (0.996-0.998), so the f16 "
                       "number is the headline and bf16 is reported here only"}
        del sam2, pipe2

    # ---- the mode closest to the reference's own fp32 floor (VERDICT r05 "next round" 2): EVERY block GEMM on hi + lo operands (split 63,
    # MXFP4 lo terms).  Needs the lo copies of all block weights, i.e. an engine of its own; same loop, same tiles. ----
    all_split = None
    if args.full and rank == 0 and world == 1 and not args.no_fast_leg and args.model == "vit_h" and args.workload == "c2" and args.dtype == "f16":
        try:
            pipe = None
            torch.cuda.empty_cache()
            sam3 = samrs_amd.sam_model_registry[args.model](state_dict=sd, precision="f16", max_images=2 * B, max_prompts=box_batch, max_points=1,
                                                            options={"split": 63}).to(dev)
            pipe3 = make_pipe(sam3, True)
            pipe3.split_mode, pipe3.allow_reduced = 63, True
            n_s = max(2, args.steps // 2)
            dts, ts_, _ = timed(pipe3, dev_tiles, n_s, 1, shared_queue=False)
            all_split = {"value": round(ts_ / dts, 3), "unit": "images/s", "steps": n_s, "split": 63, "vs_value": round(ts_ / dts / value, 4),
                         "parity": parity_of_mode(63, args.workload, args.model),
                         "note": "same loop with all four block GEMMs of every block on hi + lo operands (MXFP4 lo terms): the mode closest to the "
                                 "fp32 backend floor; not the headline"}
            del sam3, pipe3
        except Exception as ex:
            all_split = {"value": None, "note": f"failed: {type(ex).__name__}: {ex}"}

    # ---- the generation CLI end to end: PNG tiles on disk -> samrs_amd.generate.run (reader pool over libsamrs_io.so,
    # TilePipeline with device RLE, writer pool) -> gray + color PNG + ins/*.pkl on disk.  The rate is that of generate's loop
    # (first read to last file written; its model build is outside).  Host-side work on this box's CPU slice is part of it. ----
    cli = None
    if args.full and rank == 0 and world == 1 and not args.no_cli_leg and args.workload == "c2":
        import argparse as _ap
        import shutil
        import tempfile
        from concurrent.futures import ThreadPoolExecutor
        from samrs_amd import generate, tile_io
        try:
            pipe = None
            torch.cuda.empty_cache()
            root = tempfile.mkdtemp(prefix="samrs_bench_cli_")
            n_cli = max(8 * B, min(40 * B, args.cli_tiles))
            os.makedirs(os.path.join(root, "img"))
            ann = {}
            for i in range(n_cli):
                bx, lb = synth.make_boxes(i, args.boxes)
                ann[f"T{i:05d}"] = {"boxes": bx.tolist(), "labels": lb.tolist()}
            with ThreadPoolExecutor(8) as ex:
                list(ex.map(lambda i: tile_io.write_rgb(os.path.join(root, "img", f"T{i:05d}.png"),
                                                        np.roll(host_tiles[i % len(host_tiles)].numpy(), 37 * (i // len(host_tiles)), axis=1), 1),
                            range(n_cli)))
            with open(os.path.join(root, "boxes.json"), "w") as f:
                json.dump(ann, f)
            ns = _ap.Namespace(images=os.path.join(root, "img"), boxes=os.path.join(root, "boxes.json"), out=os.path.join(root, "out"),
                               model=args.model, checkpoint=None, precision=args.dtype, classes=None, n_classes=18, palette=None,
                               box_batch=64, no_rle=False, batch=B, schedule="static", readers=0, writers=0, resume=False,
                               rle_buffer_mb=512, timing=True, png_level=-2, out_depth=4)
            import contextlib
            with contextlib.redirect_stdout(sys.stderr):             # stdout carries the ONE JSON line of this script, nothing else
                st = generate.run(ns)["timing"]
            per = {k: round(1e3 * v / st["images"], 1) for k, v in sorted(st["stage_thread_seconds"].items()) if not k.startswith("loop.")}
            cli = {"value": round(st["images"] / st["loop_seconds"], 3), "unit": "images/s", "tiles": st["images"],
                   "cpus": len(os.sched_getaffinity(0)), "cpu_quota": _cpu_quota(),
                   "readers": st.get("readers"), "writers": st.get("writers"),
                   "what": "python -m samrs_amd.generate end to end: 1024^2 PNG tiles read from disk, TilePipeline with per-instance "
                           "RLE on the device, gray + color PNG (one parse, two streams) + ins/*.pkl written; reader / writer threads "
                           "sized from this rank's share of the container's CPUs; first-call warm-up inside the timed loop",
                   "host_thread_ms_per_image": per}
            # The PNG pair is the largest host item (write.gray_color_png) and its cost is a function of the class map's RUNS: masks of
            # random-init weights are noise-like.  The same encoder call on class maps shaped like real annotations (32 filled ellipses
            # per tile), timed on this box's host: what the 8-rank CPU budget of a real job looks like.
            lut = tile_io.class_lut(generate.default_palette(18))
            yy, xx = np.mgrid[0:1024, 0:1024]
            blob_ms = []
            for k in range(3):
                rng = np.random.default_rng(9000 + k)
                seg = np.full((1024, 1024), 255, np.uint8)
                for _ in range(32):
                    cy, cx = rng.uniform(0, 1024, 2)
                    a, b2 = rng.uniform(8, 200, 2)
                    th = rng.uniform(0, np.pi)
                    u = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th)
                    v = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
                    seg[(u / a) ** 2 + (v / b2) ** 2 <= 1] = rng.integers(0, 18)
                t0 = time.perf_counter()
                for _ in range(4):
                    tile_io.write_label_pair(os.path.join(root, "g.png"), os.path.join(root, "c.png"), seg, lut)
                blob_ms.append((time.perf_counter() - t0) / 4 * 1e3)
            cli["png_pair_ms_on_blob_shaped_class_maps"] = round(float(np.median(blob_ms)), 2)
            cli["read_plus_png_pair_ms_with_blob_shaped_maps"] = round(per.get("read.decode", 0.0) + float(np.median(blob_ms)), 1)
            shutil.rmtree(root, ignore_errors=True)
        except Exception as ex:                                      # a secondary leg must not take the bench line down
            cli = {"value": None, "note": f"failed: {type(ex).__name__}: {ex}"}

    cpu_baseline = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        # the oracle (a port of the reference's algorithm) on the host cores: 1 warm-up tile, then 2 timed tiles with
        # 32 boxes each as 20 + 12 chunks (main_sam_hbox_semantic.py:157-181)
        from oracle import sam_oracle as so
        # threads = what this container may actually run at once: min(cgroup CPU quota, affinity mask, 32).  More threads than the
        # quota are throttled (the pool's boxes: 256 logical CPUs, quota 16), and the value drifts with the throttling
        n_thr = int(max(1, min(32, len(os.sched_getaffinity(0)), _cpu_quota() or 1e9)))
        torch.set_num_threads(n_thr)
        orc = so.OraclePredictor(sd, cfg)

        def one_tile(i):
            img = host_tiles[i].numpy()
            bx = torch.from_numpy(synth.make_boxes(i, 32)[0])
            t0 = time.perf_counter()
            orc.set_image(img)
            t1 = time.perf_counter()
            for s0, s1 in so.box_chunks(32, 20):
                orc.predict_torch(None, None, so.apply_boxes(bx[s0:s1], (1024, 1024)), None, multimask_output=False)
            return t1 - t0, time.perf_counter() - t1

        one_tile(0)
        times = [one_tile(1 + i) for i in range(3)]
        enc_s, dec_s = float(np.mean([t[0] for t in times])), float(np.mean([t[1] for t in times]))
        cpu_baseline = {"value": round(1.0 / (enc_s + dec_s), 4), "unit": "images/s", "cores": torch.get_num_threads(),
                        "cpu_model": _cpu_model(), "cpu_quota": _cpu_quota(), "logical_cpus": os.cpu_count(),
                        "kind": "port",
                        "pinned_to": "tests/golden/*.npz: outputs of the REAL reference (oracle/make_golden.py imports /root/reference) that "
                                     "tests/test_oracle_golden.py holds this port to (low-res logits within 2e-4, <= 8 flipped pixels per mask); "
                                     "the reference tree itself is not on the GPU box",
                        "sample": f"1 warm-up + 3 timed tiles, {args.model}: set_image {enc_s:.1f}s + 32 boxes (20+12) "
                                                  f"{dec_s:.1f}s per tile, fp32 torch-CPU oracle"}
        # "the reference as users run it" -- the same oracle code in torch eager fp32 on this GPU
        # (rocBLAS / MIOpen behind torch), same tiles, same 20 + 12 box chunks, one tile at a time as the reference driver does
        try:
            sd_gpu = {k: v.to(dev) for k, v in sd.items()}
            orc = so.OraclePredictor(sd_gpu, cfg)

            def one_tile_gpu(i):
                img = host_tiles[i].numpy()
                bx = torch.from_numpy(synth.make_boxes(i, 32)[0]).to(dev)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                orc.set_image(img)
                for s0, s1 in so.box_chunks(32, 20):
                    m, _, _ = orc.predict_torch(None, None, so.apply_boxes(bx[s0:s1], (1024, 1024)), None, multimask_output=False)
                    m.cpu()                                         # main_sam_hbox_semantic.py:189
                torch.cuda.synchronize()
                return time.perf_counter() - t0

            one_tile_gpu(0)
            tg = float(np.mean([one_tile_gpu(1 + i) for i in range(3)]))
            cpu_baseline["eager_gpu"] = {"value": round(1.0 / tg, 3), "unit": "images/s",
                                         "note": "same oracle, torch eager fp32 on cuda:0, 1 warm-up + 3 timed tiles; not the "
                                                 "product path (no library of this repo is involved)"}
            del sd_gpu, orc
        except Exception as ex:                                      # a baseline leg must not take the bench line down
            cpu_baseline["eager_gpu"] = {"value": None, "note": f"failed: {type(ex).__name__}: {ex}"}

    if rank == 0:
        wl = {"c2": f"{args.model} SAM, batch={B}x1024^2 synthetic tiles, {args.boxes} hboxes/img in one box-only predict, "
                    f"multimask_output=False, masks u8 in HBM, painted class map + areas to host (BASELINE.json configs[1])",
              "c3": f"{args.model} SAM, DOTA-v2-shaped stream of 1024^2 synthetic tiles, boxes/img geometric(mean {args.boxes}, cap 400) "
                    f"in {box_batch}-box chunks, shared-counter work queue (BASELINE.json configs[2])",
              "c4": f"{args.model} SAM, instance path, {args.boxes} FAIR1M-shaped rboxes/img, prompt={args.c4_prompt}, "
                    f"multimask_output=True, best-of-3 (BASELINE.json configs[3])"}[args.workload]
        out = {
            "metric": f"images/sec (1024^2, {args.model}, {boxes_per_tile:.0f} boxes/img) SAM box->mask", "value": round(value, 3), "unit": "images/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": wl, "tiles_per_step": world * B, "boxes_per_tile": round(boxes_per_tile, 2),
                       "parallelism": f"image-parallel x{world}",
                       "weights": "seeded random init (no checkpoint available)" if args.weights == "normal" else
                                  f"seeded random init + synth.heavy_tailed ({args.weights}): outlier columns "
                                  f"{eng_info.get('outlier_columns')} in {eng_info.get('outlier_blocks')} blocks, option outlier_cols = {eng_info.get('outlier_cols')}",
                       "loop": "samrs_amd.driver.TilePipeline (the product loop of samrs_amd.generate): H2D / encoder / decoder+paint+D2H "
                               "on three HIP streams, two embedding slot sets",
                       "inputs": f"{n_pool} distinct tiles per rank rotated through the timed region, resident in HBM when it starts (the bench "
                                 "contract's `value`); `pcie_inclusive` = the same loop with the tiles starting in pinned host memory "
                                 "(BASELINE.md 4.3: H2D + D2H inside) -- the transfers are hidden, the two agree within noise",
                       "accumulate": "f32", "operand_split": split_used},
            "flops_per_image": F, "roofline": roofline, "cpu_baseline": cpu_baseline, "alt_dtype": alt, "pcie_inclusive": pcie,
            "rle_inclusive": rle_leg, "cli_inclusive": cli, "other_precision_mode": other_mode, "all_split_mode": all_split,
            "parity": parity_of_mode(int(split_used), args.workload, args.model) if args.full else None, "reference_chunking": chunk_leg,
            "full": args.full,
            "boxes_per_s": round(boxes_done / dt, 1),
            "stats_allreduce": {"total_pixels": int(tot_pix.sum().item()), "total_instances": int(tot_ins.sum().item()),
                                "per_rank_local": [{"pixels": int(a), "instances": int(b)} for a, b in per_rank]},
        }
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

"""What the checkpoint audit costs per encoder pass (GPU): ViT-H, 8 tiles, seeded weights, the 1x-rate mode the generation CLI runs
("split" = 15).  Four arms, alternating, three rounds: options off / "range_check" = 1 (the existing scan, unchanged code: the
yardstick) / "range_profile" = 1 / "range_profile" = 2.  Prints a table and, with --out, writes it to a file
(profiles/audit_cost.txt keeps one).

    python tools/audit_cost.py [--rounds 3] [--passes 5] [--tiles 8] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import samrs_amd                                            # noqa: E402
from samrs_amd import synth                                 # noqa: E402

ARMS = (("off", {"range_check": 0, "range_profile": 0}), ("range_check=1", {"range_check": 1, "range_profile": 0}),
        ("range_profile=1", {"range_check": 0, "range_profile": 1}), ("range_profile=2", {"range_check": 0, "range_profile": 2}))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", default="vit_h")
    ap.add_argument("--tiles", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", type=int, default=5, help="timed encoder passes per arm and round")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    cfg = synth.CONFIGS[a.model]
    sam = samrs_amd.sam_model_registry[a.model](precision="f16", max_images=a.tiles, options={"split": 15}).to("cuda")
    eng = sam.engine
    # two tile stacks, alternated: a pass never finds its input resident from the pass before
    stacks = [torch.as_tensor(np.stack([synth.make_noise_image(8 * k + i) for i in range(a.tiles)]), device="cuda").contiguous() for k in range(2)]
    for _, opts in ARMS:                                     # first use of every mode allocates its buffers: outside the timing
        for k, v in opts.items():
            eng.set_option(k, v)
        eng.set_images(stacks[0])
    torch.cuda.synchronize()
    times = {name: [] for name, _ in ARMS}
    for _ in range(a.rounds):
        for name, opts in ARMS:
            for k, v in opts.items():
                eng.set_option(k, v)
            eng.set_images(stacks[1])                        # one untimed pass in the arm's mode
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(a.passes):
                eng.set_images(stacks[i & 1])
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.passes)
    for k in ("range_check", "range_profile"):
        eng.set_option(k, 0)
    D, M = cfg.embed_dim, a.tiles * 4096
    scanned = 2 * M * (cfg.depth * 10 * D + D + 2 * 256)     # bytes of operand tensors one pass's sites hold
    col_bytes = 2 * M * cfg.depth * 7 * D                    # of which the column statistics read again
    med = {n: statistics.median(v) for n, v in times.items()}
    base, scan = med["off"], med["range_check=1"] - med["off"]
    lines = [f"{a.model}, {a.tiles} tiles per encoder pass, split 15, f16 operands on {torch.cuda.get_device_name(0)}; ms per pass, "
             f"{a.rounds} alternating rounds x {a.passes} passes (median of the rounds; all rounds listed)",
             f"operand bytes the sites of one pass hold: {scanned / 1e9:.2f} GB (the column statistics read {col_bytes / 1e9:.2f} GB of them again)",
             f"{'arm':18s} {'ms / pass':>10s} {'extra ms':>9s} {'x scan':>7s} {'GB/s of the extra pass':>23s}   rounds"]
    for name, _ in ARMS:
        extra = med[name] - base
        nbytes = scanned + (col_bytes if name.endswith("=2") else 0)
        lines.append(f"{name:18s} {med[name]:10.2f} {extra:9.2f} {(extra / scan if name != 'off' and scan > 0 else float('nan')):7.2f} "
                     f"{(nbytes / extra / 1e6 if name != 'off' and extra > 0 else float('nan')):23.0f}   "
                     + " ".join(f"{v:.2f}" for v in times[name]))
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

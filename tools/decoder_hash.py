"""GPU: sha256 of what the mask decoder computes -- low-res logits, IoU predictions, masks and the TOK0 / KF / KE / Q / HYPER buffers as
samrs_predict leaves them -- for every reachable decoder route (decoder_fusion 1 / 0 x upscaler_fused 1 / 0 x split 15 / 3) crossed with
every kind of call (box; 8 points, T = 14; box + mask; mask only; each with multimask 0 / 1 and return_logits 0 / 1; one
samrs_predict_multi call of 3 + 3 prompts over two slots at max_prompts = 4, whose first chunk spans both images and whose second holds
one; one samrs_set_embedding + predict, which also hashes K0F), at vit_tiny on seeded embeddings in two slots, under the library named by
SAMRS_LIB_PATH -- two builds that print the same digests issue the same launches on the same arguments.  The last line is ViT-H in its
default mode with 32 boxes.  usage: decoder_hash.py [f16|bf16]"""
import hashlib, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import samrs_amd
from samrs_amd import synth

prec_name = sys.argv[1] if len(sys.argv) > 1 else "f16"
dev = torch.device("cuda")
SIZE = (1024, 1024)


def digest(eng, outs, n_last, T, extra=()):
    """outs: tensors of the call; n_last: prompts of the call's last chunk (what the buffers hold)."""
    tokens, C = eng.cfg.grid ** 2, eng.cfg.out_chans
    bufs = [("TOK0", (n_last, T, C), torch.float32), ("KF", (n_last, tokens, C), torch.float32), ("KE", (n_last, tokens, C), torch.int16),
            ("Q", (n_last, T, C), torch.float32), ("HYPER", (n_last, 4, C // 8), torch.float32)] + list(extra)
    h = hashlib.sha256()
    for t in outs:
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    for name, shape, dt in bufs:
        h.update(eng.debug_copy_buffer(name, torch.empty(shape, dtype=dt, device=dev)).view(torch.uint8).cpu().numpy().tobytes())
    torch.cuda.synchronize()
    return h.hexdigest()[:16]


def embedding(eng, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, eng.cfg.out_chans, eng.cfg.grid, eng.cfg.grid, generator=g)


def prompts(n, seed):
    g = torch.Generator().manual_seed(seed)
    boxes = torch.from_numpy(synth.make_boxes(seed, n)[0]).float()
    coords = torch.rand(n, 8, 2, generator=g) * 1023
    labels = torch.randint(0, 2, (n, 8), generator=g, dtype=torch.int32)
    labels[n - 1, 5:] = -1
    mask = torch.randn(n, 1, 256, 256, generator=g) * 4.0
    return boxes.to(dev), coords.to(dev), labels.to(dev), mask.to(dev)


sam = samrs_amd.sam_model_registry["vit_tiny"](precision=prec_name, max_prompts=4, max_images=2, max_points=8)
sam.to(device="cuda")
eng = sam.engine
boxes, coords, labels, mask = prompts(3, 3)
boxes6 = prompts(6, 4)[0]
KINDS = [("box", boxes, None, None, None, 7), ("points8", None, coords, labels, None, 14), ("box+mask", boxes, None, None, mask, 7),
         ("mask", None, None, None, mask, 5)]
for fusion in (1, 0):
    for up_fused in (1, 0):
        for split in (15, 3):
            route = f"fusion {fusion} upscaler_fused {up_fused} split {split:2d}"
            with eng.options(decoder_fusion=fusion, upscaler_fused=up_fused, split=split):
                for slot in (0, 1):
                    eng.set_embedding(embedding(eng, 10 + slot).to(dev), slot)
                for kind, b, pc, pl, m, T in KINDS:
                    for multimask in (0, 1):
                        for logits in (0, 1):
                            masks, iou, low = eng.predict(1, b, pc, pl, m, bool(multimask), bool(logits), SIZE, SIZE)
                            print(f"{route} | {kind} multimask {multimask} logits {logits}", digest(eng, [low, iou, masks], 3, T), flush=True)
                masks, iou, low = eng.predict_multi([0, 1], [3, 3], boxes6, None, None, None, False, False, [SIZE, (768, 1024)],
                                                    [SIZE, (600, 800)])
                print(f"{route} | predict_multi 3 + 3 boxes over two slots", digest(eng, low + iou + masks, 2, 7), flush=True)
                eng.set_embedding(embedding(eng, 20).to(dev), 0)
                masks, iou, low = eng.predict(0, boxes, None, None, None, False, False, SIZE, SIZE)
                print(f"{route} | set_embedding + box", digest(eng, [low, iou, masks], 3, 7, [("K0F", (4096, 256), torch.float32)]), flush=True)
eng.close()
del sam, eng

sam = samrs_amd.sam_model_registry["vit_h"](precision=prec_name, max_prompts=32)
sam.to(device="cuda")
eng = sam.engine
eng.set_embedding(embedding(eng, 30).to(dev), 0)
masks, iou, low = eng.predict(0, prompts(32, 5)[0], None, None, None, False, False, SIZE, SIZE)
print(f"vit_h default mode (split {eng.get_option('split')}) | 32 boxes", digest(eng, [low, iou, masks], 32, 7), flush=True)

"""GPU: sha256 of the outputs of the encoder's four block GEMMs (ViT-H shapes, seeded operands, fp32 outputs accumulate into a non-zero C)
and of every kernel the selection rule (csrc/gemm_select.h) can reach in the product build, at the smallest shape the rule sends there,
under the library named by SAMRS_LIB_PATH -- two builds that print the same digests compute the same bits.  The last line is the
padded-operand-stride case of the two kernels that take a stride (persistent pair-stage: qkv, four-wave: lin1 + GELU), through the path
that sets it: the embedding of 4 tiles on the two-block 1280-wide model, option "operand_pad" = 1.  usage: gemm_hash.py [f16|bf16]"""
import ctypes, hashlib, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from samrs_amd import engine

lib = engine.load_library()
lib.samrs_debug_set_gemm_variant.argtypes = [ctypes.c_int]
lib.samrs_debug_set_gemm_variant.restype = None
prec_name = sys.argv[1] if len(sys.argv) > 1 else "f16"
prec = engine.PRECISIONS[prec_name]
dt = torch.float16 if prec_name == "f16" else torch.bfloat16
dev = torch.device("cuda")
s = torch.cuda.current_stream().cuda_stream
g = torch.Generator().manual_seed(5)
# name, M, N, K, out_f32, gelu, accumulate, variant (8 = the automatic rule; the 256x320 staggered kernel is reached by a forced variant only:
# the rule prefers the pair-stage kernel whenever K % 64 == 0, which every launch satisfies)
SHAPES = [("qkv", 32768, 3840, 1280, 0, 0, 0, 8), ("proj+res", 32768, 1280, 1280, 1, 0, 1, 8), ("lin1+gelu", 32768, 5120, 1280, 0, 1, 0, 8),
          ("lin2+res", 32768, 1280, 5120, 1, 0, 1, 8), ("proj b=3", 3 * 4096, 1280, 1280, 1, 0, 1, 8), ("neck-like", 4096, 256, 1280, 1, 0, 0, 8),
          ("persistent pair-stage", 4096, 5120, 128, 0, 0, 0, 8), ("four-wave", 16384, 5120, 256, 0, 1, 0, 8),
          ("one-tile pair-stage", 16384, 1280, 128, 1, 0, 1, 8), ("256x320 staggered (variant 10)", 256, 640, 64, 1, 0, 0, 10),
          ("256x256 staggered", 32768, 2048, 64, 0, 0, 0, 8), ("dual", 256, 128, 64, 0, 1, 0, 8), ("staggered", 256, 2048, 64, 0, 0, 0, 8),
          ("K=256 streaming", 65536, 256, 256, 0, 0, 0, 8), ("base", 128, 128, 64, 0, 0, 0, 8)]
for name, M, N, K, of32, gelu, acc, variant in SHAPES:
    A = torch.randn(M, K, generator=g).to(dev).to(dt)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev).to(dt)
    bias = torch.randn(N, generator=g).to(dev)
    C = torch.randn(M, N, generator=g).to(dev) if of32 else torch.zeros(M, N, dtype=torch.int16, device=dev)
    lib.samrs_debug_set_gemm_variant(variant)
    rc = lib.samrs_k_gemm(prec, A.data_ptr(), W.data_ptr(), C.data_ptr(), bias.data_ptr(), None, 0, M, N, K, of32, gelu, acc, s)
    lib.samrs_debug_set_gemm_variant(8)
    torch.cuda.synchronize()
    print(name, rc, hashlib.sha256(C.cpu().numpy().tobytes()).hexdigest()[:16], flush=True)

import samrs_amd
from samrs_amd import synth
sam = samrs_amd.sam_model_registry["vit_tiny1280"](precision=prec_name, max_prompts=8, max_images=4)
sam.to(device="cuda")
eng = sam.engine
tiles = torch.stack([torch.as_tensor(synth.make_noise_image(90 + i)) for i in range(4)]).cuda()
for pad in (1, 0):
    with eng.options(operand_pad=pad):
        eng.set_images(tiles, 0)
        emb = torch.stack([eng.get_embedding(i).clone() for i in range(4)])
        in_force = eng.get_option("operand_pad")
    torch.cuda.synchronize()
    print(f"padded operands (qkv, lin1+gelu of 4 tiles, operand_pad {pad})", in_force,
          hashlib.sha256(emb.cpu().numpy().tobytes()).hexdigest()[:16], flush=True)

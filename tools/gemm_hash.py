"""GPU: sha256 of the outputs of the encoder's four block GEMMs (ViT-H shapes, seeded operands, fp32 outputs accumulate into a non-zero C)
and of every kernel the selection rule (csrc/gemm_select.h) can reach in the product build, at the smallest shape the rule sends there,
under the library named by SAMRS_LIB_PATH -- two builds that print the same digests compute the same bits.  Then the public launchers
beside the rule, once each at their smallest shape through their hooks: launch_gemm_f32 (csrc/gemm_decoder.hip), launch_gemm_et_gln
(csrc/gemm_dual.hip), launch_gemm_et_split3, launch_mx4_pack and launch_gemm_et_mx (csrc/gemm.hip).  The last lines are embeddings
of 4 tiles on the two-block 1280-wide model: the padded-operand-stride case of the two kernels that take a stride (persistent pair-stage:
qkv; four-wave: lin1 + GELU; both csrc/gemm.hip) through the option that sets it, "operand_pad" = 1, and the two launchers
without a hook, the LayerNorm tail ("ln_tail" = 1) and the outlier-column stage ("outlier_cols" = 7 / 0).  usage: gemm_hash.py [f16|bf16]"""
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


def sha(*ts):
    torch.cuda.synchronize()
    return " ".join(hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:16] for t in ts)


def hi_lo(x):       # the two-term operand split, made here so that it does not depend on the library under test
    hi = x.to(dev).to(dt)
    return hi, (x.to(dev) - hi.float()).to(dt)


# the public launchers that do not go through the selection rule, each once at its smallest shape, through their hooks
for K in (16, 32, 256):     # launch_gemm_f32: K split over S = 1, 2, 16 waves
    A, W, bias, C = (torch.randn(*sh, generator=g).to(dev) for sh in ((32, K), (32, K), (32,), (32, 32)))
    rc = lib.samrs_k_gemm_f32(A.data_ptr(), K, W.data_ptr(), bias.data_ptr(), C.data_ptr(), 32, 32, 32, K, 1, 1, s)
    print(f"f32 K={K}", rc, sha(C), flush=True)
M = 256
for N, K in ((128, 64), (256, 64), (320, 64), (640, 128)):      # K = 128: two stages per tile, what the persistent kernel is tested at
    Ah, Al = hi_lo(torch.randn(M, K, generator=g))
    Bh, Bl = hi_lo(torch.randn(N, K, generator=g) / K ** 0.5)
    bias = torch.randn(N, generator=g).to(dev)
    if N == 128:            # launch_gemm_et_gln: GELU(LayerNorm2d_64), ET output; with lo operands the split product, fp32 output
        gb = torch.cat([1 + 0.2 * torch.randn(64, generator=g), 0.2 * torch.randn(64, generator=g)]).to(dev)
        for lo in (False, True):
            C = torch.zeros(M, N, dtype=torch.float32 if lo else torch.int16, device=dev)
            rc = lib.samrs_k_gemm_gln(prec, Ah.data_ptr(), Bh.data_ptr(), C.data_ptr(), bias.data_ptr(), gb.data_ptr(), M, N, K,
                                      Al.data_ptr() if lo else None, Bl.data_ptr() if lo else None, s)
            print(f"gln lo={int(lo)}", rc, sha(C), flush=True)
        continue
    if N != 640:            # launch_gemm_et_split3: fp32 output on the 256 x 320 and the 256 x 256 tile, ET output (persistent kernel)
        for of32 in ((1, 0) if N == 320 else (1,)):
            C = torch.randn(M, N, generator=g).to(dev) if of32 else torch.zeros(M, N, dtype=torch.int16, device=dev)
            rc = lib.samrs_k_gemm_split3(prec, Ah.data_ptr(), Al.data_ptr(), Bh.data_ptr(), Bl.data_ptr(), C.data_ptr(), bias.data_ptr(),
                                         M, N, K, of32, of32, 0, s)
            print(f"split3 N={N} out_f32={of32}", rc, sha(C), flush=True)
    if N == 256:
        continue
    # launch_mx4_pack (K padded to the smallest Kp, 256) then launch_gemm_et_mx: fp32 and ET output (N = 320); GELU + MX rows out
    # (N = 640, the smallest N whose MX rows fill whole stages), with lo terms (gemm_et_mx_kernel) and without (persistent pair-stage)
    Kp, packed = 256, []
    for hi, lo, rows, is_b in ((Ah, Al, M, 0), (Bh, Bl, N, 1)):
        q = [torch.zeros(rows, Kp // 2, dtype=torch.uint8, device=dev) for _ in range(2)]
        sc = [torch.zeros(int(lib.samrs_k_mx_scale_bytes(rows, Kp, is_b)), dtype=torch.uint8, device=dev) for _ in range(2)]
        rc = lib.samrs_k_mx4_pack(prec, None, hi.data_ptr(), lo.data_ptr(), None, q[0].data_ptr(), q[1].data_ptr(), sc[0].data_ptr(),
                                  sc[1].data_ptr(), rows, K, K, Kp, is_b, s)
        print(f"mx4_pack rows={rows} is_b={is_b}", rc, sha(*q, *sc), flush=True)
        packed.append((q, sc))
    (qa, sa), (qb, sb) = packed
    mx_ops = (qa[1].data_ptr(), qa[0].data_ptr(), sa[1].data_ptr(), sa[0].data_ptr(), qb[0].data_ptr(), qb[1].data_ptr(), sb[0].data_ptr(),
              sb[1].data_ptr())
    if N == 320:
        for of32 in (1, 0):
            C = torch.randn(M, N, generator=g).to(dev) if of32 else torch.zeros(M, N, dtype=torch.int16, device=dev)
            rc = lib.samrs_k_gemm_mx(prec, Ah.data_ptr(), Bh.data_ptr(), C.data_ptr(), bias.data_ptr(), M, N, K, Kp, *mx_ops, of32, of32, 0, s)
            print(f"gemm_mx out_f32={of32}", rc, sha(C), flush=True)
    else:
        Ko = N // 80 * 96
        for flags in (1, 3):
            C = torch.zeros(M, N, dtype=torch.int16, device=dev)
            oq = [torch.zeros(M, Ko // 2, dtype=torch.uint8, device=dev) for _ in range(2)]
            osc = [torch.zeros(int(lib.samrs_k_mx_scale_bytes(M, Ko, 0)), dtype=torch.uint8, device=dev) for _ in range(2)]
            rc = lib.samrs_k_gemm_mx_gelu_mxout(prec, Ah.data_ptr(), Bh.data_ptr(), C.data_ptr(), bias.data_ptr(), M, N, K, Kp, *mx_ops, flags,
                                                oq[0].data_ptr(), oq[1].data_ptr(), osc[0].data_ptr(), osc[1].data_ptr(), s)
            print(f"gemm_mx_gelu_mxout flags={flags}", rc, sha(C, *oq, *osc), flush=True)

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
# the two launchers without a hook, in situ on the same model: the LayerNorm tail (launch_gemm_et_lntail behind proj / lin2) and the
# outlier-column stage (launch_gemm_et_ext; 0 = the plain launches instead)
for opts in ({"ln_tail": 1}, {"outlier_cols": 7}, {"outlier_cols": 0}):
    with eng.options(**opts):
        eng.set_images(tiles, 0)
        emb = torch.stack([eng.get_embedding(i).clone() for i in range(4)])
        in_force = [eng.get_option(k) for k in opts]
    print(f"embedding of 4 tiles, {opts}", in_force, sha(emb), flush=True)

"""GPU: every kernel the GEMM selection rule (samrs_amd/csrc/gemm_select.h) reaches in the product build, at the smallest shape the
rule sends there, in both operand types: samrs_debug_gemm_choice names the expected kernel, samrs_k_gemm runs, and the result is the
fp64 product (comparison and tolerances of tests/test_kernels_gpu.py: fp32 outputs rel L2 < 2e-6, ET outputs within 1.5 ulp of the
rounded reference).  All under the automatic variant but one: the 256x320 staggered kernel is reached by a forced variant only (the
automatic rule prefers the pair-stage kernel whenever K % 64 == 0, which every launch satisfies), here as variant 10.

The two launch options the engine passes explicitly (kernels.h GemmOpts):
  * ld (padded operand rows of qkv / lin1, on both kernels that take a stride, with either erf form): the launches alone, with NaN
    in the pad columns, against the dense launch and the fp64 product in tests/test_outlier_kernels_gpu.py test_padded_row_gemm (the
    strides the rule refuses: tests/test_gemm_select_host.py); inside a whole engine in tests/test_parity_gpu.py
    test_operand_row_padding_is_bit_identical;
  * gelu_form = 2: test_gelu_form_reaches_the_kernel below."""
import ctypes
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_kernels_gpu import PRECS, dev, et_bits, rel_err, stream  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from samrs_amd import engine
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return engine.load_library()


# kernel (enum GemmKernel), ni, mode | M, N, K | out_f32, gelu, accumulate | variant
CASES = [("X64P", 0, 0, 4096, 5120, 128, 0, 0, 0, 8), ("W4X", 0, 0, 16384, 5120, 256, 0, 1, 0, 8), ("X64", 5, 3, 16384, 1280, 128, 1, 0, 1, 8),
         ("STAG_256x320", 0, 0, 256, 640, 64, 1, 0, 0, 10), ("STAG_256x256", 0, 0, 32768, 2048, 64, 0, 0, 0, 8),
         ("DUAL", 0, 0, 256, 128, 64, 0, 1, 0, 8), ("STAG", 0, 0, 256, 2048, 64, 0, 0, 0, 8), ("K256", 0, 0, 65536, 256, 256, 0, 0, 0, 8),
         ("BASE", 0, 0, 128, 128, 64, 0, 0, 0, 8)]
KERNELS = ["BASE", "STAG", "DUAL", "DUAL_LOCKSTEP", "STAG_256x256", "STAG_256x320", "X64", "X64P", "W4X", "K256"]


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS, ids=[p[0] for p in PRECS])
@pytest.mark.parametrize("kernel,ni,mode,M,N,K,out_f32,gelu,accumulate,variant", CASES, ids=[c[0] for c in CASES])
def test_rule_picks_and_kernel_computes(lib, kernel, ni, mode, M, N, K, out_f32, gelu, accumulate, variant, name, prec, dt, ulp):
    out8 = (ctypes.c_int32 * 8)()
    lib.samrs_debug_gemm_choice(prec, M, N, K, out_f32, gelu, accumulate, 0, 0, variant, out8)
    assert out8[4] == 0 and (KERNELS[out8[0]], out8[1], out8[2]) == (kernel, ni, mode), list(out8)
    g = torch.Generator().manual_seed(M + N + K)
    _, Ab = et_bits(torch.randn(M, K, generator=g), dt)
    _, Bb = et_bits(torch.randn(N, K, generator=g) / math.sqrt(K), dt)
    Ad, Bd, bias = dev(Ab), dev(Bb), dev(torch.randn(N, generator=g))
    ref = Ad.view(dt).double() @ Bd.view(dt).double().t() + bias.double()
    if out_f32:
        C0 = torch.randn(M, N, generator=g).cuda()
        out = C0.clone()
        if accumulate:
            ref += C0.double()
    else:
        out = torch.empty(M, N, dtype=torch.int16, device="cuda")
    lib.samrs_debug_set_gemm_variant.argtypes = [ctypes.c_int]
    lib.samrs_debug_set_gemm_variant(variant)
    try:
        rc = lib.samrs_k_gemm(prec, Ad.data_ptr(), Bd.data_ptr(), out.data_ptr(), bias.data_ptr(), None, 0, M, N, K, out_f32, gelu, accumulate, stream())
    finally:
        lib.samrs_debug_set_gemm_variant(8)
    assert rc == 0
    torch.cuda.synchronize()
    if out_f32:
        r, mx = rel_err(out, ref)
        print(f"{kernel} {name} {M}x{N}x{K} fp32: rel {r:.2e} max {mx:.2e}")
        assert r < 2e-6
    else:
        ref_e = F.gelu(ref.float()) if gelu else ref.float()
        err = ((out.view(dt).float() - ref_e).abs() / ref_e.abs().clamp(min=1e-2)).max().item()
        print(f"{kernel} {name} {M}x{N}x{K} ET{' + GELU' if gelu else ''}: max rel {err:.2e}")
        assert err < 1.5 * ulp


def test_gelu_form_reaches_the_kernel(lib):
    """lin1 of one tile at width 1280 (4096 x 5120 x 1280, ET + GELU) runs on the persistent pair-stage kernel, whose epilogue has two erf
    forms; the engine names the form in the launch (option "gelu_fast": -1 = automatic, on in the default split-15 mode).  The form
    asked for must be the one that runs: the automatic choice gives the bits of gelu_fast = 1, and gelu_fast = 0 gives other bits
    (the two forms differ by up to 3e-7 in erf, A-S 7.1.28 against 7.1.26: of the 2 x 21 M hidden values some round the other way).
    How close each form is to the oracle is the parity tests' matter (tests/test_parity_gpu.py runs both: split 15 and split 79)."""
    from samrs_amd import synth
    from test_parity_gpu import get_predictor
    out8 = (ctypes.c_int32 * 8)()
    lib.samrs_debug_gemm_choice(1, 4096, 5120, 1280, 0, 1, 0, 0, 0, 8, out8)
    assert out8[4] == 0 and KERNELS[out8[0]] == "X64P", list(out8)
    eng = get_predictor("vit_tiny1280", "f16").model.engine
    tile = torch.as_tensor(synth.make_noise_image(7))[None].cuda()
    emb = {}
    with eng.options(split=15):
        for form in (-1, 1, 0):
            with eng.options(gelu_fast=form):
                eng.set_images(tile, 0)
                emb[form] = eng.get_embedding(0).clone()
    assert emb[1].abs().max() > 0
    assert torch.equal(emb[-1], emb[1])
    assert not torch.equal(emb[0], emb[1])

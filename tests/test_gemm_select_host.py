"""CPU: the GEMM selection rule (samrs_amd/csrc/gemm_select.h) through samrs_debug_gemm_choice -- no launch, no device.

1. Every row of tests/gemm_select_cases.json -- the answers of the rule as it stood before it was written down in one place (recorded with
   the launchers stubbed; the table's "about" says how) -- is still the answer: kernel, its parameters, refusals, and what the three
   planning predicates say of the shape.
2. The planning predicates are statements about the rule, over the grid the rule was compared on: operands may be padded (gemm_ld_ok)
   exactly when the plain ET launch, strided as the engine then launches it, runs on one of the two kernels that take a stride, and
   the outlier-column stage (gemm_ext_ok) only where the fp32 accumulate launch of the shape picks the one-tile pair-stage kernel.
   Domain: shapes a plain launch takes (M, N % 128 == 0, K % 64 == 0).  The predicates also answer for N = 320 (whole 256 x 320 tiles,
   which the EXT / LayerNorm-tail launches need) where a plain launch is refused; no engine has such a width (embed_dim % 128 == 0)."""
import ctypes
import itertools
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["BASE", "STAG", "DUAL", "DUAL_LOCKSTEP", "STAG_256x256", "STAG_256x320", "X64", "X64P", "W4X", "K256", "M32", "W4", "ABL_BIG", "ABL_X64"]


@pytest.fixture(scope="module")
def choice():
    import __graft_entry__ as ge
    ge.build_library()
    from samrs_amd import engine
    lib = engine.load_library()
    out = (ctypes.c_int32 * 8)()

    def ask(prec, M, N, K, out_f32=0, gelu=0, accumulate=0, add2d=0, ld=0, variant=8):
        for i in range(8):
            out[i] = -1
        lib.samrs_debug_gemm_choice(prec, M, N, K, out_f32, gelu, accumulate, add2d, ld, variant, out)
        return dict(kernel=KERNELS[out[0]], ni=out[1], mode=out[2], persistent=out[3], reject=out[4], ld_ok=out[5], ext_ok=out[6], lntail_ok=out[7])
    return ask


def test_enumerators_match_the_header():
    text = open(os.path.join(ROOT, "samrs_amd", "csrc", "gemm_select.h")).read()
    body = text[text.index("enum class GemmKernel {"):]
    body = body[body.index("{") + 1:body.index("};")]
    names = [line.split(",")[0].strip() for line in body.splitlines() if line.strip() and not line.strip().startswith("//")]
    assert names == KERNELS
    assert json.load(open(os.path.join(ROOT, "tests", "gemm_select_cases.json")))["kernels"] == KERNELS


def test_recorded_table(choice):
    cases = json.load(open(os.path.join(ROOT, "tests", "gemm_select_cases.json")))["cases"]
    assert len(cases) >= 300
    reached = set()
    wrong = []
    for c in cases:
        got = choice(c["prec"], c["M"], c["N"], c["K"], c["out_f32"], c["gelu"], c["accumulate"], c["add2d"], c["ld"], c["variant"])
        want = {k: c[k] for k in got}
        if got["reject"] and want["reject"]:          # a refusal carries no kernel
            got = {k: got[k] for k in ("reject", "ld_ok", "ext_ok", "lntail_ok")}
            want = {k: want[k] for k in got}
        elif not want["reject"]:
            reached.add(want["kernel"])
        if got != want:
            wrong.append((c["what"], want, got))
    assert not wrong, wrong[:5]
    # every kernel of the product build is in the table
    assert reached == set(KERNELS[:10]), reached


def test_stride_keeps_the_dma_pieces_aligned(choice):
    """Both kernels that take an operand stride fetch 16-byte LDS-DMA pieces at byte offset 2 (row ld + ...) from an aligned base: a
    stride is taken exactly when it is >= K and a multiple of 8 elements, on either kernel and in either operand type."""
    for prec in (0, 1):
        for M, N, K, gelu, kernel in ((4096, 5120, 128, 0, "X64P"), (16384, 5120, 256, 1, "W4X"), (32768, 3840, 1280, 0, "X64P")):
            for ld in range(K - 8, K + 137):
                got = choice(prec, M, N, K, gelu=gelu, ld=ld)
                if ld >= K and ld % 8 == 0:
                    assert not got["reject"] and got["kernel"] == kernel, (prec, M, N, K, ld, got)
                else:
                    assert got["reject"], (prec, M, N, K, ld, got)
            assert choice(prec, M, N, K, gelu=gelu, ld=-8)["reject"]


GRID_M = [128, 256, 384, 4096, 8192, 12288, 16384, 32768, 65536]
GRID_N = [128, 256, 320, 384, 640, 1280, 1536, 2048, 2560, 3840, 5120]
GRID_K = [32, 64, 96, 128, 256, 1280, 1536, 1600, 5120]


def test_predicates_are_statements_about_the_rule(choice):
    n_ld = n_ext = 0
    for M, N, K in itertools.product(GRID_M, GRID_N, GRID_K):
        if M % 128 or N % 128 or K % 64:
            continue
        for gelu in (0, 1):
            strided = choice(1, M, N, K, gelu=gelu, ld=K + 64)
            takes = not strided["reject"] and strided["kernel"] in ("X64P", "W4X")
            assert bool(strided["ld_ok"]) == takes, (M, N, K, gelu, strided)
            if "SAMRS_GEMM_M32" not in os.environ:       # the A/B mask of an experiments build redirects unstrided launches
                plain = choice(1, M, N, K, gelu=gelu)
                assert bool(plain["ld_ok"]) == (not plain["reject"] and plain["kernel"] in ("X64P", "W4X")), (M, N, K, gelu, plain)
            n_ld += takes
        resid = choice(1, M, N, K, out_f32=1, accumulate=1)
        if resid["ext_ok"] and "SAMRS_GEMM_M32" not in os.environ:
            assert not resid["reject"] and (resid["kernel"], resid["ni"], resid["mode"]) == ("X64", 5, 3), (M, N, K, resid)
            n_ext += 1
        if resid["lntail_ok"]:
            assert resid["ext_ok"] and N <= 1280, (M, N, K, resid)
        # under a forced variant nothing is padded and the outlier stage takes its own launch; the LayerNorm tail does not look at it
        forced = choice(1, M, N, K, out_f32=1, accumulate=1, variant=6)
        assert not forced["ld_ok"] and not forced["ext_ok"] and forced["lntail_ok"] == resid["lntail_ok"]
    assert n_ld > 0 and n_ext > 0

"""GPU: the batched fp32 GEMM of the decoder's token side, LayerNorm as the decoder and the neck call it, and the image ingest /
embedding hand-over / reference-grade GELU kernels, each alone through its kernel-level entry point
(include/samrs_hip_internal.h), against a float64 statement of the same operation on the operands exactly as the kernel receives
them.  Conventions of tests/test_decoder_kernels_gpu.py and tests/test_outlier_kernels_gpu.py (`Guarded`, `fp32_bound`, `rel_l2`,
`et_bits`, `round_et64`, `et_excess`, `pair_excess`, `split_bits` come from there):

  * every output is a [guard | window | guard] buffer pre-filled with the NaN pattern of its type; afterwards every element the
    kernel owns is finite and every element it does not own -- the guards, the columns [N, ldc) of a GEMM row, the stripes of
    another problem -- holds that pattern (or, when the launch accumulates, the bits of C0) bit for bit;
  * operand rows that have a stride carry NaN in their pad columns: a kernel that reads them shows it;
  * deterministic bounds, fixed by the arithmetic and not measured: a GEMM element is within (K + 8) 2^-24 (sum_k |a_k w_k| +
    |bias_n| + |C0_mn|) of the fp64 value (the worst case of any fp32 summation order, 8 for bias, ReLU, accumulate and the LDS
    combine); a constant LayerNorm row is beta to one rounding; data movement, ET rounding and the patch normalisation are bit for
    bit; launches repeat bit for bit, and a GEMM row's bits depend neither on the rows nor on the problems that share its launch;
  * everything else: rel L2 <= `fp32_bound` = 8 x the rel-L2 noise of the same formula evaluated by torch in float32, floor 3e-6,
    per problem of a GEMM batch and per ROW of a LayerNorm launch.

Measured on the kernels as they stand (MI355X; the worst case of each group; "noise" = the float32 evaluation of the reference
formula against float64; 677 cases, 4.0 s for the whole file).

  kernel / launch       case (worst of the group)                        measured              bound
  --------------------  -----------------------------------------------  --------------------  -------------------------------
  gemm_f32 per element  engine launches (171): mlp1 231 x 2048 x 256     0.024 of the bound    (K + 8) 2^-24 (sum |a w| + ..)
                        K splits (252): K 16, count 5, 17 x 40           0.128 of the bound    the same
  gemm_f32 rel L2       engine launches: mlp2 7 x 256 x 2048 magnitudes  2.1e-7                3.0e-6 (noise 2.9e-7)
    (per problem)       the others, all kinds                            1.1e-7 .. 1.2e-7      3.0e-6 (noise 0.7 .. 1.9e-7)
                        K splits with more than one element              6.0e-7 (K 48, 33 x 1) 4.5e-6 (noise 5.7e-7)
                        K splits, ONE element (M = N = 1; the element    3.8e-6 (K 80)         7.3e-6 (noise 9.1e-7): 0.52 of
                        bound is the check that counts there)            1.5e-5 (K 1280)       it; 2.1e-4 (noise 2.6e-5)
  gemm_f32 bits         second launch; rows [0, m1) + [m1, M); every     0 differing bits      exact
                        problem in a launch of its own; stripes alone
  layernorm fp32        N(0, 1) 3 + 0.5 / constant row / magnitudes,     1.0e-7 .. 1.5e-7      3.0e-6 (noise 6.1e-8 .. 7.7e-8)
    (worst ROW)         in place, in place + ET, D edges, window source
                        0.003 +- 0.001 (the case that shows eps)         3.8e-7                3.0e-6 (noise 2.0e-7)
                        1000 +- 1, 64 rows in place + ET                 1.35e-4               5.0e-4 (noise 6.2e-5)
                        (the mean of 256 values near 1000 carries 2^-24 1000 = 6e-5 per rounding against a spread of 0.58;
                        torch's float32 LayerNorm pays the same, which is why the bound comes from the reference's noise)
  layernorm ET          1000 +- 1, 64 rows, f16                          beyond ulp 5.9e-6     5.0e-4; = ET(fp32 output) bit for
                                                                                               bit in all 44 cases with both
  layernorm in place    all 70 cases                                     0 differing bits      exact (= the separate buffer)
  layernorm window      grids 14, 15, 28, 29 x 1, 2 images               0 differing bits      exact (plain rows / zero rows)
  constant row          all 26 cases that hold one                       within the bound      2^-23 |beta| per element
  patch_im2col          all 96 cases, hi and lo                          0 differing bits      exact: the device's fp32 division
                                                                                               is IEEE (-O3, no fast-math flag)
  transpose_f32         7 shapes, there and back                         0 differing bits      exact
  neck_im2col           18 cases                                         0 differing bits      exact
  gelu_split hi         n 1028, f16                                      beyond ulp 7.0e-10    3.0e-6 (the floor)
  gelu_split hi + lo    n 1028, bf16                                     beyond rep. 2.3e-7    3.0e-6 (noise 2.4e-8)
                        (single elements of the negative tail are relative errors of 3e-2 in bf16 -- Abramowitz-Stegun 7.1.26 is
                        absolute-accurate, common.h -- and GELU(-6) = -5.9e-9 is zero in f16: a rel L2 does not see them, and
                        lin2 sums these values against others of order 1)
                        |lo| <= ulp(hi) / 2                              0 violations          exact

No kernel missed a bound and no host check was found missing.  Where the rounding of A + A2 sits is pinned by the "cancel" kind
only in this sense: A2 = -A (1 + d) makes the sum 2^-20 of its terms, the fp32 sum of two such values is exact (Sterbenz), and the
element bound scales with the SUM -- a kernel that multiplied A and A2 separately, or added after a rounding of its own, would be
2^-24 |A| |W| off: a sixteenth of the result, thousands of times the bound.

What the one-line mutations do to this file (each rebuilt in a scratch copy and loaded through SAMRS_LIB_PATH; each stays inside the
buffers of these tests: the window gather's input and the patch kernel's image carry spare rows behind them for that reason, and the
transpose's guards are 32 output rows deep):
  gemm_f32  blockIdx.z -> 0                     218: 84 engine launches (every count > 1), 125 of the 126 K splits with count 5, all 9
                                                independence cases
            pa2[h] for h == 0 only              223: 48 engine launches (those with an addend and more than 16 rows), 166 K splits, 9
                                                independence cases
            bias[n] -> bias[nl]                 205: 135 engine launches (every N > 32), the 70 K splits with N = 40 and a bias
            ReLU after the accumulate           124 of the 126 K splits with count 5 (the launches that set both)
            wave * KW -> wave * FKS             142: 124 of the 126 K splits with S > 1 and more than one slab, the 18 mlp2 launches (K 2048;
                                                at K = 256 KW = FKS = 16 and the mutant is the kernel)
  layernorm eps -> 0                            40: every "const" case (26: NaN in the constant row) and every "small" case
                                                (14: rel L2 O(1))
            valid forced true                   the 8 window cases at grids 15 and 29 (NaN rows where zeros belong)
            x / y of the window exchanged       the 12 window cases at grids 15, 28, 29 (grid 14 is one window)
  patch     c_mean[c] -> c_mean[2 - c]          all 96 cases
            y < in_h -> y <= in_h               the 64 cases whose height is not the full grid
            lo never written                    the 48 cases with A_lo
  transpose output guard r < rows only          1 x 1, 31 x 33, 33 x 31, 100 x 7: the guards behind the window
Everything in this file has been run on the device, against the kernels and against every mutant.
"""
import ctypes
import math
import os
import sys
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_decoder_kernels_gpu import Guarded, PRECS, dev, et_bits, et_excess, fp32_bound, gen, rel_l2, round_et64, stream  # noqa: E402
from test_outlier_kernels_gpu import et_f64, layernorm_ref, magnitudes, pair_excess, split_bits, ulp_of  # noqa: E402

pytestmark = pytest.mark.gpu

PREC_IDS = [p[0] for p in PRECS]
U24 = 2.0 ** -24
NAN32 = 0x7FC00000
FLOOR = 3e-6                                   # the floor of `fp32_bound`
F32_BATCH_MAX = 5                              # kernels.h


@pytest.fixture(scope="module")
def lib():
    from samrs_amd import engine
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return engine.load_library()


def i32bits(t):
    return t.contiguous().view(torch.int32)


def fill_window(g, values):
    """write fp32 / int16 `values` (CPU, the Guarded's shape) into its window"""
    raw = values.contiguous().view(torch.int32 if g.dt == torch.float32 else torch.int16).reshape(-1)
    g.buf[g.g:g.g + g.n] = raw.cuda()


# ==================================================================================================================
# A. batched fp32 GEMM
# ==================================================================================================================
def ptrs(values):
    return (ctypes.c_void_p * len(values))(*values)


def draw(kind, shape, g):
    if kind == "magnitudes":
        return magnitudes(shape, g)
    return torch.randn(shape, generator=g)


def strided(values, ld):
    """device rows of ld floats: `values` [M][K] in front, NaN behind"""
    M, K = values.shape
    buf = torch.full((M, ld), float("nan"))
    buf[:, :K] = values
    return buf.cuda()


class Batch:
    """operands of `count` problems of one shape, as the kernel receives them: A[z] / A2[z] (None: no addend) [M][K], W[z] [N][K],
    bias[z] (None: null) [N] on the CPU, and the device pointers that go with them.  kind: normal N(0, 1); magnitudes +-10^U(-3, 3);
    zero_rows: normal with one row of A (and of its addend) and one row of W all zero; cancel: A2 = -A (1 + d), |d| <= 2^-20, where
    an addend is given.  layout: dense -- every problem its own rows of lda floats; tokens -- one [M][T][K] buffer, problem z reads
    token 1 + z (the last problem token 0) of every row group, lda = T K (run_heads, first layer); w_off -- W and bias start
    `w_off` rows / elements into a larger weight (the IoU head's column slice)."""

    def __init__(self, count, M, N, K, lda, kind, a2, seed, bias=None, layout="dense", w_off=0):
        g = gen(seed)
        self.count, self.M, self.N, self.K, self.lda = count, M, N, K, lda
        self.keep, self.A, self.A2, self.W, self.bias = [], [], [], [], []
        self.pA, self.pA2, self.pW, self.pb = [], [], [], []
        bias = bias if bias is not None else (True,) * count
        zr_m, zr_n = M // 2, N // 2
        if layout == "tokens":
            T = lda // K
            q = draw(kind, (M, T, K), g)
            if kind == "zero_rows":
                q[zr_m] = 0.0
            qd = q.cuda()
            self.keep.append(qd)
        for z in range(count):
            if layout == "tokens":
                tok = 1 + z if z < count - 1 else 0
                A, pA = q[:, tok, :].contiguous(), qd.data_ptr() + 4 * tok * K
            else:
                A = draw(kind, (M, K), g)
                if kind == "zero_rows":
                    A[zr_m] = 0.0
                Ad = strided(A, lda)
                self.keep.append(Ad)
                pA = Ad.data_ptr()
            A2, pA2 = None, None
            if a2[z]:
                if kind == "cancel":
                    A2 = -(A.double() * (1.0 + (torch.rand(M, K, generator=g, dtype=torch.float64) * 2 - 1) * 2.0 ** -20)).float()
                else:
                    A2 = draw(kind, (M, K), g)
                if kind == "zero_rows":
                    A2[zr_m] = 0.0
                A2d = strided(A2, lda)
                self.keep.append(A2d)
                pA2 = A2d.data_ptr()
            Wfull = draw(kind, (N + w_off, K), g) * (1.0 if kind == "magnitudes" else 1.0 / math.sqrt(K))
            bfull = draw(kind, (N + w_off,), g)
            if kind == "zero_rows":
                Wfull[w_off + zr_n] = 0.0
            Wd, bd = Wfull.cuda(), bfull.cuda()
            self.keep += [Wd, bd]
            self.A.append(A); self.A2.append(A2); self.W.append(Wfull[w_off:]); self.bias.append(bfull[w_off:] if bias[z] else None)
            self.pA.append(pA); self.pA2.append(pA2); self.pW.append(Wd.data_ptr() + 4 * w_off * K)
            self.pb.append(bd.data_ptr() + 4 * w_off if bias[z] else None)

    def a32(self, z):
        """what the kernel multiplies: A, or A + A2 rounded to fp32 ONCE (torch adds in float32)"""
        return self.A[z] if self.A2[z] is None else self.A[z] + self.A2[z]

    def reference(self, z, relu, C0, dtype):
        v = self.a32(z).to(dtype) @ self.W[z].to(dtype).t()
        if self.bias[z] is not None:
            v = v + self.bias[z].to(dtype)
        if relu:
            v = v.clamp(min=0.0)
        return v + C0.to(dtype) if C0 is not None else v

    def magnitude(self, z, C0):
        """sum_k |a_k w_k| + |bias_n| + |C0_mn| in fp64"""
        v = self.a32(z).double().abs() @ self.W[z].double().abs().t()
        if self.bias[z] is not None:
            v = v + self.bias[z].double().abs()
        return v + C0.double().abs() if C0 is not None else v


def gemm_launch(lib, b, pC, ldc, relu, acc, zs=None, rows=None, M=None, N=None, K=None, lda=None, count=None, pA=None, pA2="same", pW=None):
    """one launch of problems `zs` (default: all) on rows [rows[0], rows[1]) (default: all); the keyword overrides are for refusals"""
    zs = list(range(b.count)) if zs is None else zs
    r0, r1 = rows if rows else (0, b.M)
    off = 4 * r0 * b.lda
    A = pA if pA is not None else [b.pA[z] + off for z in zs]
    if pA2 == "same":
        pA2 = [b.pA2[z] + off if b.pA2[z] is not None else None for z in zs]
        pA2 = ptrs(pA2) if any(p is not None for p in pA2) or len(zs) > 1 else None      # a single problem without addend: the null ARRAY
    else:
        pA2 = ptrs(pA2)
    W = pW if pW is not None else [b.pW[z] for z in zs]
    C = [pC[z] + 4 * r0 * ldc for z in zs]
    return lib.samrs_k_gemm_f32_batch(ptrs(A), pA2, ptrs(W), ptrs([b.pb[z] for z in zs]), ptrs(C), len(zs) if count is None else count,
                                      b.lda if lda is None else lda, ldc, (r1 - r0) if M is None else M, b.N if N is None else N,
                                      b.K if K is None else K, relu, acc, stream())


class GemmOut:
    """the outputs of a batch: one Guarded [M][ldc] per problem, or (stripes) ONE Guarded [M][ldc] that problem z enters at column
    z N; the window holds NaN, or C0 when the launch accumulates"""

    def __init__(self, b, ldc, C0=None, stripes=False):
        self.b, self.ldc, self.stripes = b, ldc, stripes
        self.bufs = [Guarded((b.M, ldc), torch.float32) for _ in range(1 if stripes else b.count)]
        self.C0 = C0
        if C0 is not None:
            for buf, c0 in zip(self.bufs, C0):
                fill_window(buf, c0)
        self.pC = [self.bufs[0].ptr + 4 * z * b.N for z in range(b.count)] if stripes else [g.ptr for g in self.bufs]

    def read(self, what):
        """per problem: int32 bits of the whole [M][ldc] window it lives in (guards checked)"""
        return [i32bits(g.read(what, finite=False)) for g in self.bufs]


def check_batch(lib, b, ldc, relu, acc, what, stripes=False):
    """assertions 1 - 4 of a launch; returns the bits of every problem's window and the figures for the table"""
    N, M = b.N, b.M
    g = gen(977 + M + N)
    C0 = None
    if acc:
        C0 = [draw("normal", (M, ldc), g) for _ in range(b.count)]
    outs = []
    for _ in range(2):                                                     # (4) launched twice, fresh outputs
        o = GemmOut(b, ldc, C0, stripes)
        assert gemm_launch(lib, b, o.pC, ldc, relu, acc) == 0, what
        outs.append(o.read(what))
    first, second = outs
    assert all(torch.equal(x, y) for x, y in zip(first, second)), f"{what}: a second launch gives other bits"
    worst_el, worst_l2, worst_noise = 0.0, 0.0, 0.0
    for z in range(b.count):
        win = first[0] if stripes else first[z]
        c0 = (C0[0] if stripes else C0[z]) if acc else None
        col0 = z * N if stripes else 0
        own = torch.zeros(M, ldc, dtype=torch.bool)
        own[:, col0:col0 + N] = True
        if stripes:
            own[:, :b.count * N] = True                                    # the other problems' stripes: theirs, checked in their turn
        # (1) outside [M][N]: NaN pattern, or C0's bits
        rest = i32bits(c0) if acc else torch.full((M, ldc), NAN32, dtype=torch.int32)
        stray = int(((win != rest) & ~own).sum())
        assert stray == 0, f"{what} problem {z}: {stray} elements outside its [M][N] window were written"
        got = win.view(torch.float32)[:, col0:col0 + N]
        assert bool(torch.isfinite(got).all()), f"{what} problem {z}: elements of its window not written, or not finite"
        c0w = c0[:, col0:col0 + N] if acc else None
        ref64, ref32 = b.reference(z, relu, c0w, torch.float64), b.reference(z, relu, c0w, torch.float32)
        # (2) per element, the worst case of any summation order
        lim = (b.K + 8) * U24 * b.magnitude(z, c0w)
        err = (got.double() - ref64).abs()
        over = err > lim
        el = (err / lim.clamp(min=1e-300)).max().item() if lim.numel() else 0.0
        assert not bool(over.any()), f"{what} problem {z}: {int(over.sum())} elements beyond (K + 8) 2^-24 (sum |a w| + |bias| + |C0|), worst {el:.2f} x"
        # (3) rel L2 of the problem
        bound, noise = fp32_bound(ref32, ref64)
        r = rel_l2(got, ref64)
        assert r <= bound, f"{what} problem {z}: rel L2 {r:.2e} > {bound:.2e} (noise {noise:.2e})"
        worst_el = max(worst_el, el)
        if r >= worst_l2:
            worst_l2, worst_noise = r, noise
    print(f"gemm_f32 {what}: worst element {worst_el:.3f} of its bound, worst problem rel L2 {worst_l2:.2e} (noise {worst_noise:.2e})")
    return first


ENGINE_C, ENGINE_CI = 256, 128


def engine_launches():
    """(id, count, M-rule, N, K, lda-rule, ldc, relu, acc, a2, layout, w_off, kinds) of engine_decode.hip's launches"""
    C, Ci = ENGINE_C, ENGINE_CI
    cases = []
    all_kinds, no_a2 = ("normal", "magnitudes", "zero_rows", "cancel"), ("normal", "magnitudes", "zero_rows")
    for T in (7, 9):
        for n in (1, 3, 33):
            BT = n * T
            for name, count, M, N, K, lda, ldc, relu, acc, a2, layout, kinds in (
                    ("qkv", 3, BT, C, C, C, C, 0, 0, (1, 1, 0), "dense", all_kinds),
                    ("i2t_kv", 2, BT, Ci, C, C, Ci, 0, 0, (1, 0), "dense", all_kinds),
                    ("heads0", 5, n, C, C, T * C, C, 1, 0, (0,) * 5, "tokens", no_a2),
                    ("sum", 1, BT, Ci, C, C, Ci, 0, 0, (1,), "dense", all_kinds),
                    ("mlp1", 1, BT, 2048, C, C, 2048, 1, 0, (0,), "dense", no_a2),
                    ("mlp2", 1, BT, C, 2048, 2048, C, 0, 1, (0,), "dense", no_a2)):
                for kind in kinds:
                    cases.append(pytest.param(name, count, M, N, K, lda, ldc, relu, acc, a2, layout, 0, kind, id=f"{name}-T{T}-n{n}-{kind}"))
    for n in (1, 3, 33):
        for kind in no_a2:
            cases.append(pytest.param("heads1", 5, n, C, C, C, C, 1, 0, (0,) * 5, "dense", 0, kind, id=f"heads1-n{n}-{kind}"))
            cases.append(pytest.param("heads2", 4, n, C // 8, C, C, 4 * (C // 8), 0, 0, (0,) * 4, "stripes", 0, kind, id=f"heads2-n{n}-{kind}"))
            for nsel, sel0 in ((1, 0), (3, 1), (4, 0)):
                cases.append(pytest.param("iou", 1, n, nsel, C, C, nsel, 0, 0, (0,), "dense", sel0, kind, id=f"iou-n{n}-nsel{nsel}-{kind}"))
    return cases


@pytest.mark.parametrize("name,count,M,N,K,lda,ldc,relu,acc,a2,layout,w_off,kind", engine_launches())
def test_gemm_f32_batch_engine_launches(lib, name, count, M, N, K, lda, ldc, relu, acc, a2, layout, w_off, kind):
    """every launch of engine_decode.hip at C = 256: the problem count, the addend on some problems only, lda = T C, the interleaved
    stripes and the offset weight of the IoU head, as the engine sends them"""
    stripes = layout == "stripes"
    b = Batch(count, M, N, K, lda, kind, a2, seed=zlib.crc32(f"{name} {M} {N} {K} {kind}".encode()), layout="dense" if stripes else layout, w_off=w_off)
    what = f"{name} count {count} {M}x{N}x{K} lda {lda} ldc {ldc} {kind}"
    together = check_batch(lib, b, ldc, relu, acc, what, stripes)
    if stripes:
        # each problem alone into a NaN-filled row buffer: its stripe holds the bits of the launch of all four, the other three NaN
        for z in range(count):
            o = GemmOut(b, ldc, None, True)
            assert gemm_launch(lib, b, o.pC, ldc, relu, acc, zs=[z]) == 0
            alone = o.read(f"{what} problem {z} alone")[0]
            want = torch.full((M, ldc), NAN32, dtype=torch.int32)
            want[:, z * N:(z + 1) * N] = together[0][:, z * N:(z + 1) * N]
            assert torch.equal(alone, want), f"{what}: problem {z} alone wrote outside its stripe, or other bits than in the batch"


K_SPLITS = [(16, 1), (48, 1), (80, 1), (32, 2), (96, 2), (160, 2), (64, 4), (192, 4), (320, 4), (128, 8), (384, 8), (640, 8), (256, 16),
            (1280, 16)]


def k_split(K):
    S = 1
    while S < 16 and K % (32 * S) == 0:
        S *= 2
    return S


@pytest.mark.parametrize("count", [1, 5])
@pytest.mark.parametrize("N", [1, 31, 40])
@pytest.mark.parametrize("M", [1, 17, 33])
@pytest.mark.parametrize("K,S", K_SPLITS, ids=[f"K{k}-S{s}" for k, s in K_SPLITS])
def test_gemm_f32_batch_k_splits(lib, K, S, M, N, count):
    """every K split of the launcher with 1, 3 and 5 slabs per wave (the ring holds 4), strided rows on both sides, an addend on
    some problems and a null bias on one; count 5 runs ReLU and accumulate together (ReLU first)"""
    assert k_split(K) == S
    ki = [k for k, _ in K_SPLITS].index(K)
    if count == 5:
        a2, bias, relu, acc = (0, 1, 0, 1, 1), (1, 1, 1, 0, 1), 1, 1
    else:
        a2, bias, relu, acc = (1,), (M != 17,), (ki % 3 == 1) * 1, (ki % 3 == 2) * 1
    b = Batch(count, M, N, K, K + 4, "normal", a2, seed=K * 7 + M * 3 + N + count, bias=bias)
    check_batch(lib, b, N + 3, relu, acc, f"K {K} S {S} count {count} {M}x{N} relu {relu} acc {acc}")


ROW_CASES = [(256, 256, 0, 0), (2048, 40, 0, 1), (48, 31, 1, 0)]


@pytest.mark.parametrize("K,N,relu,acc", ROW_CASES, ids=[f"K{c[0]}-N{c[1]}" for c in ROW_CASES])
@pytest.mark.parametrize("M,m1", [(33, 20), (32, 12), (63, 1)])
def test_gemm_f32_batch_row_and_problem_independence(lib, M, m1, K, N, relu, acc):
    """the launcher's promise: the bits of a row depend neither on how many rows the launch carries (rows [0, m1) and [m1, M) in two
    launches) nor on the problems it shares the launch with (each problem in a launch of its own)"""
    count, a2 = 3, (1, 1, 0)
    b = Batch(count, M, N, K, K, "normal", a2, seed=M + m1 + K + N)
    ldc = N + 3
    C0 = [torch.randn(M, ldc, generator=gen(5 + z)) for z in range(count)] if acc else None

    def run(parts, groups):
        o = GemmOut(b, ldc, C0)
        for rows in parts:
            for zs in groups:
                assert gemm_launch(lib, b, o.pC, ldc, relu, acc, zs=zs, rows=rows) == 0
        return o.read("row independence")
    whole = run([(0, M)], [None])
    halves = run([(0, m1), (m1, M)], [None])
    singles = run([(0, M)], [[z] for z in range(count)])
    for z in range(count):
        assert torch.equal(whole[z], halves[z]), f"problem {z}: rows [0, {m1}) + [{m1}, {M}) differ from the launch of all {M}"
        assert torch.equal(whole[z], singles[z]), f"problem {z}: a launch of its own differs from the batch"


def test_gemm_f32_batch_refusals(lib):
    """what the engine never sends is refused on the host, nothing written"""
    M, N, K = 5, 8, 32
    b = Batch(F32_BATCH_MAX + 1, M, N, K, K + 4, "normal", (1,) * 6, seed=1)
    o = GemmOut(b, N)
    two = [0, 1]

    def call(**kw):
        kw.setdefault("zs", two)
        return gemm_launch(lib, b, o.pC, kw.pop("ldc", N), 0, 0, **kw)
    assert call(count=0) != 0
    assert call(zs=list(range(6))) != 0
    b24 = Batch(2, M, N, 24, 28, "normal", (1, 1), seed=2)
    assert gemm_launch(lib, b24, o.pC, N, 0, 0) != 0                                  # K = 24
    assert call(lda=K + 2) != 0
    assert call(lda=K - 4) != 0
    assert call(ldc=N - 1) != 0
    assert call(pA=[b.pA[0], b.pA[1] + 4]) != 0                                         # A[1] 4 bytes off
    assert call(pA2=[b.pA2[0] + 4, b.pA2[1]]) != 0                                      # A2[0] 4 bytes off
    assert call(pW=[b.pW[0], None]) != 0
    assert call(M=0) != 0 and call(N=0) != 0
    assert all(g.untouched() for g in o.bufs)
    assert call() == 0                                                                  # and the same call, unmodified, runs
    assert bool(torch.isfinite(o.bufs[0].read("refusals: valid call")).all())


# ==================================================================================================================
# B. LayerNorm as the decoder and the neck call it
# ==================================================================================================================
LN_KINDS = ["normal", "bigmean", "const", "magnitudes", "small"]


def ln_input(kind, rows, D, g):
    if kind == "bigmean":
        return 1000.0 + (torch.rand(rows, D, generator=g) * 2 - 1)
    if kind == "small":                                    # the case that shows eps: variance 3.3e-7 against eps 1e-5
        return 0.003 + (torch.rand(rows, D, generator=g) * 2 - 1) * 0.001
    if kind == "magnitudes":
        return magnitudes((rows, D), g)
    X = torch.randn(rows, D, generator=g) * 3.0 + 0.5
    if kind == "const":
        X[rows // 2] = 2.5
    return X


def ln_params(D, g):
    return 1.0 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)


def ln_call(lib, prec, x_ptr, gd, bd, eps, out_et, out_f32, rows, D, window_mode=0, n_images=1, grid=0, window=0):
    return lib.samrs_k_layernorm(prec, x_ptr, gd.data_ptr(), bd.data_ptr(), eps, out_et, out_f32, rows, D, window_mode, n_images, grid,
                                 window, stream())


def ln_check(what, kind, X, gamma, beta, eps, got32, got_et, ulp):
    """per-ROW rel L2 of the fp32 output and `et_excess` of the ET output under `fp32_bound` of the case; the constant row; eps"""
    ref64 = layernorm_ref(X, gamma, beta, eps, torch.float64)
    ref32 = F.layer_norm(X, (X.shape[1],), gamma, beta, eps)
    bound, noise = fp32_bound(ref32, ref64)
    rn = ref64.norm(dim=1).clamp(min=1e-300)
    worst = 0.0
    if got32 is not None:
        rows_err = (got32.double() - ref64).norm(dim=1) / rn
        worst = rows_err.max().item()
        assert worst <= bound, f"{what}: row {int(rows_err.argmax())} rel L2 {worst:.2e} > {bound:.2e} (noise {noise:.2e})"
    exc = 0.0
    if got_et is not None:
        exc = et_excess(got_et.float(), ref64, ulp)
        assert exc <= bound, f"{what}: ET beyond one ulp {exc:.2e} > {bound:.2e}"
    print(f"layernorm {what}: worst row rel L2 {worst:.2e}, ET beyond ulp {exc:.2e} (noise {noise:.2e}, bound {bound:.2e})")
    if kind == "const" and got32 is not None:
        r = X.shape[0] // 2
        lim = 2.0 ** -23 * beta.double().abs().clamp(min=2.0 ** -126)
        assert bool(((got32[r].double() - beta.double()).abs() <= lim).all()), f"{what}: the constant row is not beta to one rounding"
    if kind == "small":
        # the test sees eps: the fp64 reference with the encoder's 1e-6 in the decoder's place misses the bound on every row
        other = layernorm_ref(X, gamma, beta, 1e-6 if eps == 1e-5 else 1e-5, torch.float64)
        miss = (other - ref64).norm(dim=1) / rn
        assert bool((miss > bound).all()), f"{what}: eps is not visible at this case ({miss.min().item():.2e} <= {bound:.2e})"
    return bound


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("kind", LN_KINDS)
@pytest.mark.parametrize("rows", [1, 3, 7, 63, 4 * 9 + 1])
def test_layernorm_in_place_tokens(lib, rows, kind, name, prec, dt, ulp):
    """ln_tokens: out_f32 == X, no ET output, eps 1e-5, D = 256: the bits of the launch into a separate buffer"""
    D, eps = 256, 1e-5
    g = gen(rows * 31 + LN_KINDS.index(kind))
    X = ln_input(kind, rows, D, g)
    gamma, beta = ln_params(D, g)
    gd, bd, Xd = dev(gamma), dev(beta), dev(X)
    sep, inp = Guarded((rows, D), torch.float32), Guarded((rows, D), torch.float32)
    fill_window(inp, X)
    assert ln_call(lib, prec, Xd.data_ptr(), gd, bd, eps, None, sep.ptr, rows, D) == 0
    assert ln_call(lib, prec, inp.ptr, gd, bd, eps, None, inp.ptr, rows, D) == 0
    a, b = sep.read("layernorm separate"), inp.read("layernorm in place")
    assert torch.equal(i32bits(a), i32bits(b)), "the in-place launch differs from the launch into a separate buffer"
    assert torch.equal(i32bits(Xd.cpu()), i32bits(X)), "the launch into a separate buffer changed its input"
    ln_check(f"in place {kind} rows {rows} {name}", kind, X, gamma, beta, eps, b, None, ulp)


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("kind", LN_KINDS)
@pytest.mark.parametrize("rows", [5, 64])
def test_layernorm_in_place_with_et(lib, rows, kind, name, prec, dt, ulp):
    """run_dec_layer's KF / KE: out_f32 == X and an ET output in the same launch; ET = ET(the fp32 output) bit for bit"""
    D, eps = 256, 1e-5
    g = gen(rows * 37 + LN_KINDS.index(kind))
    X = ln_input(kind, rows, D, g)
    gamma, beta = ln_params(D, g)
    gd, bd, Xd = dev(gamma), dev(beta), dev(X)
    sep, sep_et = Guarded((rows, D), torch.float32), Guarded((rows, D), dt)
    inp, inp_et = Guarded((rows, D), torch.float32), Guarded((rows, D), dt)
    fill_window(inp, X)
    assert ln_call(lib, prec, Xd.data_ptr(), gd, bd, eps, sep_et.ptr, sep.ptr, rows, D) == 0
    assert ln_call(lib, prec, inp.ptr, gd, bd, eps, inp_et.ptr, inp.ptr, rows, D) == 0
    a, b = sep.read("layernorm separate"), inp.read("layernorm in place")
    assert torch.equal(i32bits(a), i32bits(b)), "the in-place launch differs from the launch into a separate buffer"
    ea, eb = sep_et.read("layernorm ET separate"), inp_et.read("layernorm ET in place")
    want = et_bits(b, dt)[1]
    assert torch.equal(eb.view(torch.int16), want) and torch.equal(ea.view(torch.int16), want), "the ET output is not ET(the fp32 output)"
    ln_check(f"in place + ET {kind} rows {rows} {name}", kind, X, gamma, beta, eps, b, eb, ulp)


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("kind", ["normal", "const"])
@pytest.mark.parametrize("D", [4, 252, 256, 260, 1280, 2048])
def test_layernorm_width_edges(lib, D, kind, name, prec, dt, ulp):
    """one float4, a partial lane pass on either side of a full one, LN_MAXV's ceiling; 5 rows: the last block owns one"""
    rows, eps = 5, 1e-5
    g = gen(D + LN_KINDS.index(kind))
    X = ln_input(kind, rows, D, g)
    gamma, beta = ln_params(D, g)
    gd, bd, Xd = dev(gamma), dev(beta), dev(X)
    o32, oet = Guarded((rows, D), torch.float32), Guarded((rows, D), dt)
    assert ln_call(lib, prec, Xd.data_ptr(), gd, bd, eps, oet.ptr, o32.ptr, rows, D) == 0
    got = o32.read(f"layernorm D {D}")
    e = oet.read(f"layernorm ET D {D}")
    assert torch.equal(e.view(torch.int16), et_bits(got, dt)[1])
    ln_check(f"D {D} {kind} {name}", kind, X, gamma, beta, eps, got, e, ulp)


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS, ids=PREC_IDS)
def test_layernorm_refuses_widths(lib, name, prec, dt, ulp):
    X, gd, bd = torch.zeros(4, 2052).cuda(), torch.ones(2052).cuda(), torch.zeros(2052).cuda()
    o32, oet = Guarded((4, 2052), torch.float32), Guarded((4, 2052), dt)
    for D in (2052, 6):
        assert ln_call(lib, prec, X.data_ptr(), gd, bd, 1e-5, oet.ptr, o32.ptr, 4, D) != 0
    assert o32.untouched() and oet.untouched()


def window_rows(n_images, grid, window):
    """per output row of the window order: (valid, source row)"""
    nw = -(-grid // window)
    w2 = window * window
    r = torch.arange(n_images * nw * nw * w2)
    t, win, im = r % w2, (r // w2) % (nw * nw), r // (w2 * nw * nw)
    y = (win // nw) * window + t // window
    x = (win % nw) * window + t % window
    return (y < grid) & (x < grid), (im * grid + y) * grid + x


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("n_images", [1, 2])
@pytest.mark.parametrize("grid", [14, 15, 28, 29])
def test_layernorm_window_gather(lib, grid, n_images, name, prec, dt, ulp):
    """window 14: no padding, one padded ring, an exact multiple, one over: padded rows zero bits, live rows the plain launch's"""
    D, window, eps = 64, 14, 1e-6
    g = gen(grid * 3 + n_images)
    rows = n_images * grid * grid
    X = ln_input("normal", rows, D, g)
    gamma, beta = ln_params(D, g)
    # NaN rows behind the input, up to where the padded positions of the last image would index: a gather that followed them stays
    # inside the allocation and shows
    nw = -(-grid // window)
    Xd = torch.cat([X, torch.full(((nw * window) ** 2, D), float("nan"))]).cuda()
    gd, bd = dev(gamma), dev(beta)
    p32, pet = Guarded((rows, D), torch.float32), Guarded((rows, D), dt)
    assert ln_call(lib, prec, Xd.data_ptr(), gd, bd, eps, pet.ptr, p32.ptr, rows, D) == 0
    plain32, plain_et = i32bits(p32.read("layernorm plain")), pet.read("layernorm plain ET").view(torch.int16)
    valid, src = window_rows(n_images, grid, window)
    rows_out = valid.numel()
    assert int(valid.sum()) == rows and (grid % window != 0) == bool((~valid).any())
    w32, wet = Guarded((rows_out, D), torch.float32), Guarded((rows_out, D), dt)
    assert ln_call(lib, prec, Xd.data_ptr(), gd, bd, eps, wet.ptr, w32.ptr, rows_out, D, 1, n_images, grid, window) == 0
    got32, got_et = i32bits(w32.read("layernorm window", finite=False)), wet.read("layernorm window ET", finite=False).view(torch.int16)
    want32, want_et = torch.zeros(rows_out, D, dtype=torch.int32), torch.zeros(rows_out, D, dtype=torch.int16)
    want32[valid], want_et[valid] = plain32[src[valid]], plain_et[src[valid]]
    assert torch.equal(got32, want32), f"fp32: {int((got32 != want32).any(1).sum())} rows differ from plain rows / zero padding"
    assert torch.equal(got_et, want_et), f"ET: {int((got_et != want_et).any(1).sum())} rows differ from plain rows / zero padding"
    # an ET-only launch (the encoder's norm1) and an fp32-only one: the same bits, nothing asked for, nothing written
    only_et, only_32 = Guarded((rows_out, D), dt), Guarded((rows_out, D), torch.float32)
    assert ln_call(lib, prec, Xd.data_ptr(), gd, bd, eps, only_et.ptr, None, rows_out, D, 1, n_images, grid, window) == 0
    assert ln_call(lib, prec, Xd.data_ptr(), gd, bd, eps, None, only_32.ptr, rows_out, D, 1, n_images, grid, window) == 0
    assert torch.equal(only_et.read("window ET only", finite=False).view(torch.int16), want_et)
    assert torch.equal(i32bits(only_32.read("window fp32 only", finite=False)), want32)
    ln_check(f"window grid {grid} n {n_images} {name}", "normal", X, gamma, beta, eps, p32.read("plain"), pet.read("plain ET"), ulp)


# ==================================================================================================================
# C. image ingest, hand-over, reference-grade GELU
# ==================================================================================================================
PIXEL_MEAN = np.array([123.675, 116.28, 103.53], dtype=np.float32)          # modeling/sam.py:27
PIXEL_STD = np.array([58.395, 57.12, 57.375], dtype=np.float32)             # modeling/sam.py:28
PATCH_SIZES = ["full", (1, 1), "ragged", (17, 9), (16, 8), ("full", 23)]


def patch_reference(img, grid, P):
    """numpy float32: (p - mean[c]) / std[c] inside the image, 0 outside -> [n g g][3 P P], k = c P P + ky P + kx"""
    n, in_h, in_w, _ = img.shape
    S = grid * P
    canvas = np.zeros((n, S, S, 3), dtype=np.float32)
    h, w = min(in_h, S), min(in_w, S)
    canvas[:, :h, :w] = (img[:, :h, :w].astype(np.float32) - PIXEL_MEAN) / PIXEL_STD
    assert canvas.dtype == np.float32
    v = canvas.reshape(n, grid, P, grid, P, 3).transpose(0, 1, 3, 5, 2, 4)      # n, py, px, c, ky, kx
    return torch.from_numpy(np.ascontiguousarray(v).reshape(n * grid * grid, 3 * P * P))


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("with_lo", [True, False], ids=["lo", "no-lo"])
@pytest.mark.parametrize("size", PATCH_SIZES, ids=["full", "1x1", "ragged", "17x9", "16x8", "fullx23"])
@pytest.mark.parametrize("n_images", [1, 3])
@pytest.mark.parametrize("grid", [2, 4])
def test_patch_im2col(lib, grid, n_images, size, with_lo, name, prec, dt, ulp):
    """normalisation, zero padding of ragged tiles and the hi | lo split, bit for bit against numpy float32 (IEEE division) and
    torch's ET rounding; images 1 and 2 of a batch of three are all 0 and all 255"""
    P, full = 16, grid * 16
    in_h, in_w = (full, full) if size == "full" else (full - 1, full - 7) if size == "ragged" else size
    in_h = full if in_h == "full" else in_h
    rng = np.random.default_rng(grid * 100 + n_images * 10 + in_h + in_w)
    img = rng.integers(0, 256, size=(n_images, in_h, in_w, 3), dtype=np.uint8)
    if n_images == 3:
        img[1], img[2] = 0, 255
    rows, Kp = n_images * grid * grid, 3 * P * P
    A, lo = Guarded((rows, Kp), dt), Guarded((rows, Kp), dt)
    # one more pixel row of 77s behind the last image: a read at y == in_h stays inside the allocation and shows
    imgd = torch.cat([torch.from_numpy(img).reshape(-1), torch.full((3 * in_w + 32,), 77, dtype=torch.uint8)]).cuda()
    assert lib.samrs_k_patch_im2col(prec, imgd.data_ptr(), A.ptr, lo.ptr if with_lo else None, n_images, in_h, in_w, grid, P, stream()) == 0
    v = patch_reference(img, grid, P)
    want_hi, want_lo = split_bits(v, dt)
    got = A.read("patch_im2col").view(torch.int16)
    bad = got != want_hi
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} hi elements differ (first at row, k = {bad.nonzero()[0].tolist()})"
    if with_lo:
        got_lo = lo.read("patch_im2col lo").view(torch.int16)
        bad = got_lo != want_lo
        assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} lo elements differ (first at row, k = {bad.nonzero()[0].tolist()})"
    else:
        assert lo.untouched(), "the launch without A_lo wrote to the stand-in"


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS, ids=PREC_IDS)
def test_patch_im2col_refusals(lib, name, prec, dt, ulp):
    img = torch.zeros(2 * 32 * 32 * 3, dtype=torch.uint8).cuda()
    A, lo = Guarded((8, 768), dt), Guarded((8, 768), dt)
    for patch, in_h, in_w, n, grid in ((12, 32, 32, 1, 2), (16, 0, 32, 1, 2), (16, 32, 0, 1, 2), (16, 32, 32, 0, 2), (16, 32, 32, 1, 0), (0, 32, 32, 1, 2)):
        assert lib.samrs_k_patch_im2col(prec, img.data_ptr(), A.ptr, lo.ptr, n, in_h, in_w, grid, patch, stream()) != 0, (patch, in_h, in_w, n, grid)
    assert lib.samrs_k_patch_im2col(prec, None, A.ptr, lo.ptr, 1, 32, 32, 2, 16, stream()) != 0
    assert lib.samrs_k_patch_im2col(prec, img.data_ptr(), None, lo.ptr, 1, 32, 32, 2, 16, stream()) != 0
    assert A.untouched() and lo.untouched()


TRANSPOSE_SHAPES = [(1, 1), (31, 33), (32, 32), (33, 31), (64, 256), (100, 7), (256, 4096)]


@pytest.mark.parametrize("rows,cols", TRANSPOSE_SHAPES, ids=[f"{r}x{c}" for r, c in TRANSPOSE_SHAPES])
def test_transpose_f32(lib, rows, cols):
    """random 32-bit patterns (NaN payloads, infinities, subnormals among them) and -0.0, compared as int32; the guards are 32 output
    rows deep, so that a store past the column count would land in them"""
    g = gen(rows * 4099 + cols)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, cols), generator=g, dtype=torch.int64).to(torch.int32)
    special = torch.tensor([-2 ** 31, 0x7FC00001, -0x3EDCBB, 0x7F800001, 0x7F800000, 1], dtype=torch.int64).to(torch.int32)      # -0.0, NaN payloads
    flat = bits.view(-1)
    flat[:min(flat.numel(), special.numel())] = special[:flat.numel()]
    if flat.numel() > 8:
        flat[-1] = special[0]
    src = bits.cuda()
    out = Guarded((cols, rows), torch.float32, rows=32)
    assert lib.samrs_k_transpose_f32(src.data_ptr(), out.ptr, rows, cols, stream()) == 0
    got = i32bits(out.read("transpose_f32", finite=False))
    assert torch.equal(got, bits.t().contiguous()), "not the transpose, bit for bit"
    back = Guarded((rows, cols), torch.float32, rows=32)
    assert lib.samrs_k_transpose_f32(out.ptr, back.ptr, cols, rows, stream()) == 0
    assert torch.equal(i32bits(back.read("transpose_f32 inverse", finite=False)), bits), "transpose and inverse do not return the input"


def test_transpose_f32_refusals(lib):
    src, out = torch.zeros(64).cuda(), Guarded((8, 8), torch.float32)
    assert lib.samrs_k_transpose_f32(src.data_ptr(), out.ptr, 0, 8, stream()) != 0
    assert lib.samrs_k_transpose_f32(src.data_ptr(), out.ptr, 8, 0, stream()) != 0
    assert lib.samrs_k_transpose_f32(None, out.ptr, 8, 8, stream()) != 0
    assert lib.samrs_k_transpose_f32(src.data_ptr(), None, 8, 8, stream()) != 0
    assert out.untouched()


@pytest.mark.parametrize("n_images", [1, 2])
@pytest.mark.parametrize("C", [8, 24, 256])
@pytest.mark.parametrize("grid", [1, 2, 3])
def test_neck_im2col(lib, grid, C, n_images):
    """the 3x3 / pad 1 gather on random 16-bit patterns at grids where every position touches the border; C = 24: a tap is three chunks"""
    g = gen(grid * 1000 + C + n_images)
    img = torch.randint(-2 ** 15, 2 ** 15 - 1, (n_images, grid, grid, C), generator=g, dtype=torch.int64).to(torch.int16)
    img[img == 0] = 1                                                         # zero is the padding's value
    src = img.cuda()
    out = Guarded((n_images * grid * grid, 9 * C), torch.float16)
    assert lib.samrs_k_neck_im2col(src.data_ptr(), out.ptr, n_images, grid, C, stream()) == 0
    got = out.read("neck_im2col", finite=False).view(torch.int16).view(n_images, grid, grid, 9, C)
    want = torch.zeros(n_images, grid, grid, 9, C, dtype=torch.int16)
    for ky in range(3):
        for kx in range(3):
            ys, xs = slice(max(0, 1 - ky), grid - max(0, ky - 1)), slice(max(0, 1 - kx), grid - max(0, kx - 1))
            yd, xd = slice(max(0, ky - 1), grid - max(0, 1 - ky)), slice(max(0, kx - 1), grid - max(0, 1 - kx))
            want[:, ys, xs, ky * 3 + kx] = img[:, yd, xd]
    assert torch.equal(got, want), "neck im2col is not the 3x3 / pad 1 gather"


def gelu64(x):
    """exact-erf GELU in fp64 without the cancellation of 1 + erf in the negative tail: 0.5 x erfc(-x / sqrt 2)"""
    x = x.double()
    return 0.5 * x * torch.special.erfc(-x * math.sqrt(0.5))


GELU_CASES = {"n4-a": [0.0, -0.0, 6.0, -6.0], "n4-b": [20.0, -20.0, 1.0, -1.0], "n1028": None}


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("case", list(GELU_CASES))
def test_gelu_split(lib, case, name, prec, dt, ulp):
    """hi = ET(GELU(x)) to one ulp, hi + lo to the fp32 noise of the erf form beyond the split's representational term, |lo| <= ulp(hi) / 2"""
    if GELU_CASES[case] is not None:
        x = torch.tensor(GELU_CASES[case])
    else:
        g = gen(1028)
        x = (10.0 ** (torch.rand(1028, generator=g) * 4.3 - 3.0)) * (torch.randint(0, 2, (1028,), generator=g) * 2 - 1).float()
        x[:8] = torch.tensor([0.0, -0.0, 6.0, -6.0, 20.0, -20.0, 1.0, -1.0])
    n = x.numel()
    hi, lo = Guarded((n,), dt), Guarded((n,), dt)
    xd = dev(x)
    assert lib.samrs_k_gelu_split(prec, xd.data_ptr(), hi.ptr, lo.ptr, n, stream()) == 0
    hb, lb = hi.read("gelu_split hi").view(torch.int16), lo.read("gelu_split lo").view(torch.int16)
    ref64 = gelu64(x)
    bound, noise = fp32_bound(F.gelu(x), ref64)
    h_exc = et_excess(et_f64(hb, dt), round_et64(ref64, dt), ulp)
    exc = pair_excess(hb, lb, ref64, dt)
    worst = ((et_f64(hb, dt) + et_f64(lb, dt) - ref64).abs() / ref64.abs().clamp(min=1e-30)).max().item()
    print(f"gelu_split {case} {name}: hi beyond one ulp {h_exc:.2e} (floor {FLOOR:.1e}); hi + lo beyond the representational term {exc:.2e} "
          f"(noise {noise:.2e}, bound {bound:.2e}); worst element rel {worst:.2e}")
    assert h_exc <= FLOOR
    assert exc <= bound
    slack = 2.0 ** -25 if dt == torch.float16 else 0.0
    over = int((et_f64(lb, dt).abs() > 0.5 * ulp_of(et_f64(hb, dt), dt) + slack).sum())
    assert over == 0, f"{over} lo values exceed half an ulp of their hi"


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS, ids=PREC_IDS)
def test_gelu_split_refusals(lib, name, prec, dt, ulp):
    x, hi, lo = torch.zeros(16).cuda(), Guarded((16,), dt), Guarded((16,), dt)
    assert lib.samrs_k_gelu_split(prec, x.data_ptr(), hi.ptr, lo.ptr, 6, stream()) != 0
    assert lib.samrs_k_gelu_split(prec, x.data_ptr(), hi.ptr, lo.ptr, 0, stream()) != 0
    assert lib.samrs_k_gelu_split(prec, x.data_ptr(), None, lo.ptr, 8, stream()) != 0
    assert lib.samrs_k_gelu_split(prec, x.data_ptr(), hi.ptr, None, 8, stream()) != 0
    assert hi.untouched() and lo.untouched()

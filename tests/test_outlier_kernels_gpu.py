"""GPU: the outlier-column kernels and the padded-row / EXT-stage GEMM launches of the ViT-H product path, each alone through its
kernel-level entry point (include/samrs_hip_internal.h), against a float64 statement of the same operation on the same
already-rounded operands.  Conventions of tests/test_decoder_kernels_gpu.py (`Guarded`, `fp32_bound`, `et_bits`, `round_et64`,
`et_excess` come from there):

  * every output is a [guard | window | guard] buffer pre-filled with the NaN pattern of its type; afterwards every element the
    kernel owns is finite and every element it does not own -- the guards, and the columns of a padded row that belong to another
    producer -- holds that pattern bit for bit;
  * index arrays are distinct, ascending, below the column count, and hold column 0 and the last column (one index: the last);
  * pure data movement and ET rounding is compared bit for bit with hi = ET(w), lo = ET(w - float(hi)) taken by torch on the CPU;
  * a hi + lo pair is judged by what its sum misses of the fp64 value beyond the representational term 2^-(2p+2) |ref| (p = 11 f16,
    8 bf16; + 2^-25 for f16's subnormal floor): the rel L2 of that excess must meet `fp32_bound`, 8 x the rel-L2 noise of the same
    formula evaluated in float32, floor 3e-6;
  * GEMM outputs: ET within 1.5 ulp of the fp64 product with the denominator clamp of tests/test_gemm_select_gpu.py, fp32 rel L2
    below 2e-6 and every 256 x 320 tile within `fp32_bound` on its own.

Measured on the kernels as they stand (MI355X; the worst case of each group; "noise" = the float32 evaluation of the reference
formula against float64; "beyond rep." = rel L2 of what hi + lo misses beyond the representational term).

  kernel / launch       case (worst of the group)                      measured              bound
  --------------------  ---------------------------------------------  --------------------  ---------------------------------
  outlier_weight_ext    all 96 cases (dense side operand, padded copy)  0 mismatching bits    exact; foreign columns untouched
  outlier_side_weight   42 accepted cases, 12 refused                   0 mismatching bits    exact (ET rows and fp32 bias)
  outlier_gather        all 24 cases                                    0 mismatching bits    exact
  weight_norms col_sq   1000 x 130 / one sum: 37 x 70                   8.4e-8 / 2.2e-7       3.0e-6 (noise 5.2e-8) / 38 2^-24
  weight_norms row_sq   16 x 64 / one sum: 1000 x 130                   5.2e-8 / 1.3e-7       3.0e-6 (noise 6.8e-8) / 131 2^-24
                        second launch, either output alone              same bits             exact
  range_scan            12 strided + 12 dense launches                  exact counts          exact; pad columns not counted
  layernorm_ext         live columns, hi slots, zeros: 96 cases         0 mismatching bits    exact (= the dense launch)
    hi + lo, f16        rows 4, D 64, ld 192, n_oc 4                    beyond rep. 8.4e-8    3.0e-6 (noise 7.8e-8); hi alone
                                                                                              2.0e-4 .. 4.4e-4
    hi + lo, bf16       rows 1, D 64, ld 192, n_oc 1 (ONE element)      beyond rep. 2.2e-6    3.0e-6 (noise 1.6e-7); hi alone
                                                                                              1.4e-3 .. 2.3e-3
                        (the term 2^-(2p+2) |ref| is half of the worst case 2^-(2p+1) |ref| of rounding o - hi to ET, so a bf16
                        element may exceed it by up to 2^-18 = 3.8e-6 of itself: the cases with few elements come closest --
                        1.9e-6 with 5, 1.3e-6 with 32 -- and the seeds are fixed; f16's 2^-24 is far below the floor)
  outlier_side_gemm     f16: M 64, K 1344, lda 1408                     beyond rep. 1.7e-7    3.0e-6 (noise 2.2e-7)
                        bf16: M 64, K 160, lda 160                      beyond rep. 6.5e-7    3.0e-6 (noise 8.5e-8)
                        |lo| <= ulp(hi) / 2, dead units                 0 violations          exact
  padded-row GEMM X64P  f16 K 1344 / bf16 K 128, both strides           0.53 / 0.50 ulp       1.5 ulp; the bits of the dense launch
  padded-row GEMM W4X   f16 K 320 / bf16 K 256, both erf forms          0.51 / 0.50 ulp       1.5 ulp; the bits of the dense launch
  EXT-stage GEMM        f16 16384 x 1280 x 320, no bias                 9.0e-8, tile 9.1e-8   2e-6; tile 3.0e-6 (noise 2.0e-7)
                        bf16 16384 x 1280 x 320, no bias                7.5e-8, tile 7.6e-8   2e-6; tile 3.0e-6 (noise 8.5e-8)
  proj chain            f16 (fp64 emulation of the chain: 2.1e-7)       2.3e-7                3.2e-6 (noise 1.8e-7, + 2^-22)
                          plain launch, no side product                 2.9e-4                >= 10 x the chain: 1280 x
                        bf16 (emulation 4.5e-6)                         4.5e-6                1.8e-5 (noise 1.8e-7, + 2^-16)
                          plain launch                                  2.4e-3                >= 10 x the chain: 530 x

No kernel missed a bound.  Reading gemm_et_x64p_kernel and gemm_et_w4x_kernel for the stride showed one gap on the host: both fetch
16-byte LDS-DMA pieces at byte offset 2 (row ld + 8 chunk), so a stride must be a multiple of 8 elements, and gemm_select took any
ld >= K.  It now refuses the others (tests/test_gemm_select_host.py, test_padded_row_gemm_refusals here); nothing but whole
multiples of 64 is launched.

What the one-line mutations do to this file (each rebuilt in a scratch copy and loaded through SAMRS_LIB_PATH, each in bounds; 372
cases in all):
  lo | hi halves exchanged in the LayerNorm extension     all 96 test_layernorm_extension cases ([D + 32 + j] != column idx[j])
  idx[j] -> j in outlier_weight_ext_kernel                the 72 test_outlier_weight_ext cases with n_oc > 0, both proj chains
  lo / hi exchanged in outlier_gather_kernel              all 24 test_outlier_gather cases, both proj chains
  bs1 read from bias[fr] in outlier_side_gemm_kernel      all 32 test_outlier_side_gemm cases
  LD forced to K in gemm_et_x64p_kernel                   the 12 X64P cases of test_padded_row_gemm (NaN from the pad, or other bits)
  EXT stage of gemm_et_x64_kernel skipped                 all 16 test_ext_stage_gemm cases, both proj chains
  row phase from ph + 16 in weight_col_norms_kernel       the 8 test_weight_norms cases that ask for col_sq
"""
import ctypes
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_decoder_kernels_gpu import Guarded, NAN_ET, PRECS, dev, et_bits, et_excess, fp32_bound, gen, rel_l2, round_et64, stream  # noqa: E402,F401

pytestmark = pytest.mark.gpu

PREC_IDS = [p[0] for p in PRECS]
SIG_BITS = {torch.float16: 11, torch.bfloat16: 8}              # p: significand bits with the hidden one
KERNELS = ["BASE", "STAG", "DUAL", "DUAL_LOCKSTEP", "STAG_256x256", "STAG_256x320", "X64", "X64P", "W4X", "K256"]


@pytest.fixture(scope="module")
def lib():
    from samrs_amd import engine
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return engine.load_library()


# ------------------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------------------
def pick(n, bound, g):
    """n distinct ascending indices below `bound` that hold 0 and bound - 1 (n == 1: the last column alone)"""
    assert 0 <= n <= bound
    if n == 0:
        return torch.zeros(0, dtype=torch.int32)
    if n == 1:
        return torch.tensor([bound - 1], dtype=torch.int32)
    mid = torch.randperm(bound - 2, generator=g)[:n - 2] + 1
    return torch.cat([torch.tensor([0]), mid.sort().values, torch.tensor([bound - 1])]).to(torch.int32)


def magnitudes(shape, g):
    """+- 10^U(-3, 3): inside the f16 range, six decades"""
    return (10.0 ** (torch.rand(shape, generator=g) * 6.0 - 3.0)) * (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


def split_bits(w, dt):
    """fp32 -> int16 bits of hi = ET(w) and lo = ET(w - float(hi)) (w - hi is exact in fp32)"""
    hi_f, hi_b = et_bits(w, dt)
    _, lo_b = et_bits(w - hi_f, dt)
    return hi_b, lo_b


def owned_bits(g, what, owned):
    """int16 window of an ET `Guarded` after a launch: guards intact (read), every element outside the boolean mask `owned` still
    the NaN pattern, every element inside finite"""
    v = g.read(what, finite=False)
    b = v.view(torch.int16)
    fill = torch.tensor(g.fill, dtype=torch.int32).to(torch.int16)
    stray = int(((b != fill) & ~owned).sum())
    assert stray == 0, f"{what}: {stray} elements that belong to another producer were written"
    bad = int((~torch.isfinite(v.float()) & owned).sum())
    assert bad == 0, f"{what}: {bad} owned elements are not finite (not written, or NaN / inf computed)"
    return b


def et_f64(bits, dt):
    return bits.view(dt).double()


def pair_excess(hi_bits, lo_bits, ref64, dt):
    """rel L2 of what float(hi) + float(lo) misses of ref64 beyond the representational term of a two-term split"""
    p = SIG_BITS[dt]
    rep = 2.0 ** -(2 * p + 2) * ref64.abs() + (2.0 ** -25 if dt == torch.float16 else 0.0)
    err = (et_f64(hi_bits, dt) + et_f64(lo_bits, dt) - ref64).abs()
    return ((err - rep).clamp(min=0.0).norm() / ref64.norm().clamp(min=1e-300)).item()


def ulp_of(x64, dt):
    """ulp of the ET values x64 (float64 tensor of ET-representable values); zero and subnormals: the subnormal step"""
    p = SIG_BITS[dt]
    emin = -13 if dt == torch.float16 else -125               # frexp exponent of the smallest normal
    _, e = torch.frexp(x64)
    e = torch.where(x64 == 0, torch.full_like(e, emin), e).clamp(min=emin)
    return torch.ldexp(torch.ones_like(x64), e - p)


def i32(t):
    return t.to(torch.int32).cuda().contiguous()


def ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


# ------------------------------------------------------------------------------------------------------------------
# pure data movement and rounding
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,prec,dt,ulp", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("layout,K,ld,col0", [("dense", 70, 64, 0), ("pad192", 64, 192, 64), ("pad256", 128, 256, 128)],
                         ids=["dense", "pad192", "pad256"])
@pytest.mark.parametrize("n_oc", [0, 1, 31, 32])
@pytest.mark.parametrize("N", [1, 8, 9, 1003])
def test_outlier_weight_ext(lib, N, n_oc, layout, K, ld, col0, name, prec, dt, ulp):
    """out[r][col0 + j] = hi, [col0 + 32 + j] = lo of W[r][idx[j]]; unused slots zero; the other columns of the row untouched"""
    g = gen(1000 * N + 10 * n_oc + K)
    W = magnitudes((N, K), g)
    idx = pick(n_oc, K, g)
    out = Guarded((N, ld), dt)
    Wd, idxd = dev(W), i32(idx)
    rc = lib.samrs_k_outlier_weight_ext(prec, Wd.data_ptr(), N, K, ptr(idxd), n_oc, out.ptr, ld, col0, stream())
    assert rc == 0
    owned = torch.zeros(N, ld, dtype=torch.bool)
    owned[:, col0:col0 + 64] = True
    got = owned_bits(out, f"outlier_weight_ext {layout}", owned)
    want = torch.zeros(N, 64, dtype=torch.int16)
    if n_oc:
        hi, lo = split_bits(W[:, idx.long()], dt)
        want[:, :n_oc], want[:, 32:32 + n_oc] = hi, lo
    wrong = int((got[:, col0:col0 + 64] != want).sum())
    assert wrong == 0, f"{wrong} of {N * 64} extension elements differ from ET(w) | ET(w - hi)"


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("Ks", [64, 128, 192])
@pytest.mark.parametrize("n1", [0, 4, 32])
@pytest.mark.parametrize("n2", [1, 5, 32])
def test_outlier_side_weight(lib, n2, n1, Ks, name, prec, dt, ulp):
    """rows j < n2 = ET(W1[idx2[j]]) | hi | lo of its columns idx1 | zeros, rows >= n2 zero, bias_out = b1[idx2] | zeros; the
    combinations the launcher does not take (an extension without room for it) are refused with nothing written"""
    D, rows1 = 64, 100
    g = gen(100 * n2 + n1 + Ks)
    W1, b1 = magnitudes((rows1, D), g), torch.randn(rows1, generator=g)
    idx2, idx1 = pick(n2, rows1, g), pick(n1, D, g)
    out, bias_out = Guarded((32, Ks), dt), Guarded((32,), torch.float32)
    W1d, b1d, i2d, i1d = dev(W1), dev(b1), i32(idx2), i32(idx1)
    rc = lib.samrs_k_outlier_side_weight(prec, W1d.data_ptr(), b1d.data_ptr(), rows1, D, i2d.data_ptr(), n2, ptr(i1d), n1, out.ptr, Ks,
                                         bias_out.ptr, stream())
    if Ks < D + (64 if n1 else 0):
        assert rc != 0 and out.untouched() and bias_out.untouched()
        return
    assert rc == 0
    got = owned_bits(out, "outlier_side_weight", torch.ones(32, Ks, dtype=torch.bool))
    want = torch.zeros(32, Ks, dtype=torch.int16)
    src = W1[idx2.long()]
    want[:n2, :D] = et_bits(src, dt)[1]
    if n1:
        hi, lo = split_bits(src[:, idx1.long()], dt)
        want[:n2, D:D + n1], want[:n2, D + 32:D + 32 + n1] = hi, lo
    wrong = int((got != want).sum())
    assert wrong == 0, f"{wrong} of {32 * Ks} side-weight elements differ"
    bo = bias_out.read("outlier_side_weight bias_out")
    wb = torch.zeros(32)
    wb[:n2] = b1[idx2.long()]
    assert torch.equal(bo.view(torch.int32), wb.view(torch.int32))


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("n_oc", [1, 31, 32])
@pytest.mark.parametrize("rows", [1, 4, 5, 4099])
def test_outlier_gather(lib, rows, n_oc, name, prec, dt, ulp):
    """out[r][j] = lo[r][idx[j]], out[r][32 + j] = hi[r][idx[j]], zeros behind n_oc; hi and lo from different random streams"""
    D = 128
    hi = et_bits(torch.randn(rows, D, generator=gen(7 * rows + n_oc)), dt)[1]
    lo = et_bits(torch.randn(rows, D, generator=gen(7 * rows + n_oc + 100000)) * 2.0 ** -11, dt)[1]
    idx = pick(n_oc, D, gen(rows + n_oc))
    out = Guarded((rows, 64), dt)
    hid, lod, idxd = dev(hi), dev(lo), i32(idx)
    assert lib.samrs_k_outlier_gather(hid.data_ptr(), lod.data_ptr(), D, idxd.data_ptr(), n_oc, out.ptr, rows, stream()) == 0
    got = owned_bits(out, "outlier_gather", torch.ones(rows, 64, dtype=torch.bool))
    want = torch.zeros(rows, 64, dtype=torch.int16)
    want[:, :n_oc], want[:, 32:32 + n_oc] = lo[:, idx.long()], hi[:, idx.long()]
    wrong = int((got != want).sum())
    assert wrong == 0, f"{wrong} of {rows * 64} gathered elements differ"


# ------------------------------------------------------------------------------------------------------------------
# reductions
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["both", "cols", "rows"])
@pytest.mark.parametrize("N,K", [(1, 1), (37, 70), (16, 64), (1000, 130)])
def test_weight_norms(lib, N, K, which):
    """squared column / row norms against fp64 sums, bound = `fp32_bound` of the same sums in torch float32; either output alone with
    the other pointer null; a second launch gives the same bits (no atomics)"""
    W = torch.randn(N, K, generator=gen(N * 131 + K)) * 0.05
    Wd = dev(W)
    col = Guarded((K,), torch.float32) if which != "rows" else None
    row = Guarded((N,), torch.float32) if which != "cols" else None

    def launch():
        assert lib.samrs_k_weight_norms(Wd.data_ptr(), N, K, col.ptr if col else None, row.ptr if row else None, stream()) == 0
        return [b.read(f"weight_norms {nm}").clone() if b else None for b, nm in ((col, "col_sq"), (row, "row_sq"))]
    first = launch()
    for got, dim, nm in zip(first, (0, 1), ("col_sq", "row_sq")):
        if got is None:
            continue
        ref64 = (W.double() ** 2).sum(dim)
        bound, noise = fp32_bound((W ** 2).sum(dim), ref64)
        r = rel_l2(got, ref64)
        worst = ((got.double() - ref64).abs() / ref64).max().item()
        print(f"weight_norms {nm} {N}x{K}: rel L2 {r:.2e} (noise {noise:.2e}, bound {bound:.2e}), worst element {worst:.2e}")
        assert r <= bound
        # no single sum may hide in the norm: a sum of n squares in fp32, in any order, is within n 2^-24 of the exact one
        assert worst <= (W.shape[dim] + 1) * 2.0 ** -24
    second = launch()
    for a, b in zip(first, second):
        assert (a is None and b is None) or torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("rows", [1, 300])
@pytest.mark.parametrize("cols,ld", [(64, 64), (64, 192), (192, 256)])
def test_range_scan_strided(lib, cols, ld, rows, name, prec, dt, ulp):
    """the counter rises by exactly the planted live values: the pad columns are full of saturated patterns and are not counted"""
    sat = [0x7bff, 0xfbff, 0x7c00, 0xfc00, 0x7e00] if dt == torch.float16 else [0x7f80, 0xff80, 0x7fc0]
    sat = torch.tensor(sat, dtype=torch.int32).to(torch.int16)
    g = gen(rows * 1000 + cols + ld)
    x = sat[torch.randint(0, len(sat), (rows, ld), generator=g)]
    x[:, :cols] = et_bits(torch.randn(rows, cols, generator=g) * 100.0, dt)[1]          # far from saturation in either type
    spots = {(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1), (rows // 2, cols // 2), (rows // 3, 7), (rows // 3, 8)}
    for k, (r, c) in enumerate(sorted(spots)):
        x[r, c] = sat[k % len(sat)]
    counter = torch.tensor([-7, 5, -7], dtype=torch.int64).cuda()
    xd = dev(x)
    assert lib.samrs_k_range_scan(prec, xd.data_ptr(), rows * cols, cols, ld, counter.data_ptr() + 8, stream()) == 0
    torch.cuda.synchronize()
    assert counter.tolist() == [-7, 5 + len(spots), -7]
    dense = dev(x[:, :cols])
    assert lib.samrs_k_range_scan(prec, dense.data_ptr(), rows * cols, 0, 0, counter.data_ptr() + 8, stream()) == 0
    torch.cuda.synchronize()
    assert counter.tolist() == [-7, 5 + 2 * len(spots), -7]
    # host-side refusals: nothing is launched
    for n, c, l in ((rows * cols, cols, cols - 8), (rows * cols, cols + 4, ld + 4), (rows * cols + 8, cols, ld), (rows * cols - 4, 0, 0)):
        assert lib.samrs_k_range_scan(prec, xd.data_ptr(), n, c, l, counter.data_ptr() + 8, stream()) != 0
    torch.cuda.synchronize()
    assert counter.tolist() == [-7, 5 + 2 * len(spots), -7]


# ------------------------------------------------------------------------------------------------------------------
# LayerNorm with the extension
# ------------------------------------------------------------------------------------------------------------------
def layernorm_ref(X, gamma, beta, eps, dtype):
    x = X.to(dtype)
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma.to(dtype) + beta.to(dtype)


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("n_oc", [1, 4, 32])
@pytest.mark.parametrize("pad", [64, 128])
@pytest.mark.parametrize("D", [64, 1280])
@pytest.mark.parametrize("rows", [1, 4, 5, 1001])
def test_layernorm_extension(lib, rows, D, pad, n_oc, name, prec, dt, ulp):
    ld = D + pad
    g = gen(rows * 7 + D + pad + n_oc)
    X = torch.randn(rows, D, generator=g) * 2.0 + 0.5
    idx = pick(n_oc, D, g)
    gamma, beta = 1.0 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    gamma[idx.long()] *= 30.0
    eps = 1e-6
    Xd, gd, bd, idxd = dev(X), dev(gamma), dev(beta), i32(idx)
    dense, ext = Guarded((rows, D), dt), Guarded((rows, ld), dt)
    assert lib.samrs_k_layernorm(prec, Xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), eps, dense.ptr, None, rows, D, 0, 1, 0, 0, stream()) == 0
    assert lib.samrs_k_layernorm_ext(prec, Xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), eps, ext.ptr, rows, D, ld, idxd.data_ptr(), n_oc, 0,
                                     stream()) == 0
    want_live = owned_bits(dense, "layernorm dense", torch.ones(rows, D, dtype=torch.bool))
    got = owned_bits(ext, "layernorm extension", torch.ones(rows, ld, dtype=torch.bool))
    assert torch.equal(got[:, :D], want_live), "the live columns differ from the dense launch of the same kernel"
    lo, hi = got[:, D:D + n_oc], got[:, D + 32:D + 32 + n_oc]
    assert torch.equal(hi, got[:, idx.long()]), "[D + 32 + j] is not the value the launch wrote at column idx[j]"
    assert not got[:, D + n_oc:D + 32].any() and not got[:, D + 32 + n_oc:].any(), "unused slots / the rest of the padded row are not zero"
    ref64 = layernorm_ref(X, gamma, beta, eps, torch.float64)[:, idx.long()]
    bound, noise = fp32_bound(layernorm_ref(X, gamma, beta, eps, torch.float32)[:, idx.long()], ref64)
    exc = pair_excess(hi, lo, ref64, dt)
    print(f"layernorm_ext {name} rows {rows} D {D} ld {ld} n_oc {n_oc}: hi + lo beyond the representational term {exc:.2e} "
          f"(noise {noise:.2e}, bound {bound:.2e}); hi alone rel L2 {rel_l2(et_f64(hi, dt), ref64):.2e}")
    assert exc <= bound


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS, ids=PREC_IDS)
def test_layernorm_extension_refusals(lib, name, prec, dt, ulp):
    rows, D = 4, 64
    X, gamma, beta = dev(torch.randn(rows, D)), dev(torch.ones(D)), dev(torch.zeros(D))
    idx = i32(torch.arange(32))
    out = Guarded((rows, D + 128), dt)

    def call(ld, n_oc, window_mode, idx_t=idx):
        return lib.samrs_k_layernorm_ext(prec, X.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1e-6, out.ptr, rows, D, ld, idx_t.data_ptr(), n_oc,
                                         window_mode, stream())
    assert call(D + 128, 33, 0) != 0
    assert call(D + 32, 4, 0) != 0
    assert call(D + 128, 4, 1) != 0
    assert call(D + 128, 2, 0, i32(torch.tensor([3, D]))) != 0            # an index at the column count
    assert call(D + 128, 2, 0, i32(torch.tensor([5, 5]))) != 0            # not distinct
    assert out.untouched()


# ------------------------------------------------------------------------------------------------------------------
# outlier_side_gemm
# ------------------------------------------------------------------------------------------------------------------
UNUSED_UNITS = [5, 17] + list(range(20, 31))        # units 0 and 31 are live


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5)))


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("pad", [0, 64])
@pytest.mark.parametrize("K", [32, 96, 160, 1344])
@pytest.mark.parametrize("M", [64, 192])
def test_outlier_side_gemm(lib, M, K, pad, name, prec, dt, ulp):
    """out[r][u] = lo, out[r][32 + u] = hi of GELU(Y Ws^T + b) before its rounding; Y rows of lda elements whose pad holds NaN"""
    lda = K + pad
    g = gen(M + 10 * K + pad)
    Yf, Yb = et_bits(torch.randn(M, K, generator=g), dt)
    Wf, Wb = et_bits(torch.randn(32, K, generator=g) / math.sqrt(K), dt)
    bias = torch.randn(32, generator=g) * 0.5 + torch.arange(32) * 0.03
    Wf[UNUSED_UNITS], Wb[UNUSED_UNITS], bias[UNUSED_UNITS] = 0.0, 0, 0.0
    Y = torch.full((M, lda), NAN_ET[dt], dtype=torch.int32).to(torch.int16)
    Y[:, :K] = Yb
    out = Guarded((M, 64), dt)
    Yd, Wd, bd = dev(Y), dev(Wb), dev(bias)
    assert lib.samrs_k_outlier_side_gemm(prec, Yd.data_ptr(), lda, Wd.data_ptr(), bd.data_ptr(), M, K, out.ptr, stream()) == 0
    got = owned_bits(out, "outlier_side_gemm", torch.ones(M, 64, dtype=torch.bool))
    lo, hi = got[:, :32], got[:, 32:]
    ref64 = gelu_erf(Yf.double() @ Wf.double().t() + bias.double())
    bound, noise = fp32_bound(gelu_erf(Yf @ Wf.t() + bias), ref64)
    exc = pair_excess(hi, lo, ref64, dt)
    print(f"outlier_side_gemm {name} M {M} K {K} lda {lda}: hi + lo beyond the representational term {exc:.2e} (noise {noise:.2e}, "
          f"bound {bound:.2e}); hi alone rel L2 {rel_l2(et_f64(hi, dt), ref64):.2e}")
    assert exc <= bound
    # hi is ET(g) and lo the rest: |g - hi| <= ulp(hi) / 2, and rounding is monotonic, so |lo| <= ET(ulp(hi) / 2) -- a power of two,
    # itself an ET value unless it falls below f16's subnormal step 2^-24 (then lo is at most that step = ulp / 2 + 2^-25)
    hi64, lo64 = et_f64(hi, dt), et_f64(lo, dt)
    slack = 2.0 ** -25 if dt == torch.float16 else 0.0
    over = int((lo64.abs() > 0.5 * ulp_of(hi64, dt) + slack).sum())
    assert over == 0, f"{over} lo values exceed half an ulp of their hi"
    assert not hi[:, UNUSED_UNITS].any() and not lo[:, UNUSED_UNITS].any(), "a unit with zero weights and bias is not exactly zero"


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS, ids=PREC_IDS)
def test_outlier_side_gemm_refusals(lib, name, prec, dt, ulp):
    Y, Ws, bias = torch.zeros(256, 128, dtype=torch.int16).cuda(), torch.zeros(32, 128, dtype=torch.int16).cuda(), torch.zeros(32).cuda()
    out = Guarded((256, 64), dt)
    for M, K, lda in ((100, 64, 64), (64, 48, 64), (64, 64, 56), (64, 64, 68), (0, 64, 64)):
        assert lib.samrs_k_outlier_side_gemm(prec, Y.data_ptr(), lda, Ws.data_ptr(), bias.data_ptr(), M, K, out.ptr, stream()) != 0, (M, K, lda)
    assert out.untouched()


# ------------------------------------------------------------------------------------------------------------------
# GEMMs: padded operand rows, the EXT stage
# ------------------------------------------------------------------------------------------------------------------
def choice(lib, prec, M, N, K, out_f32=0, gelu=0, accumulate=0, ld=0):
    out8 = (ctypes.c_int32 * 8)()
    lib.samrs_debug_gemm_choice(prec, M, N, K, out_f32, gelu, accumulate, 0, ld, 8, out8)
    return dict(kernel=KERNELS[out8[0]] if 0 <= out8[0] < len(KERNELS) else out8[0], ni=out8[1], mode=out8[2], reject=out8[4],
                ld_ok=out8[5], ext_ok=out8[6])


def dev_window(g, what):
    """a `Guarded`'s window ON the device (these outputs are too large to bring to the host per case), guards checked there"""
    torch.cuda.synchronize()
    front, back = g.buf[:g.g], g.buf[g.g + g.n:]
    assert bool((front == g.fill).all()) and bool((back == g.fill).all()), f"{what}: wrote outside its window"
    w = g.buf[g.g:g.g + g.n]
    return (w.view(g.dt) if g.dt != torch.int32 else w).view(g.shape)


def padded(bits, ld, dt):
    """device copy of ET bits [rows][K] as rows of ld elements whose pad columns hold the NaN pattern"""
    rows, K = bits.shape
    buf = torch.full((rows, ld), NAN_ET[dt], dtype=torch.int32).to(torch.int16).cuda()
    buf[:, :K] = bits.cuda()
    return buf


_gemm_case = {}


def gemm_case(lib, prec, dt, M, N, K, gelu, gelu_form):
    """operands, the dense launch's output bits and the fp64 reference of one shape, computed once and shared by its strided cases
    (one entry is kept: the cases of a shape run back to back)"""
    key = (prec, M, N, K, gelu, gelu_form)
    if _gemm_case.get("key") != key:
        _gemm_case.clear()
        g = gen(M + N + K)
        Ab = et_bits(torch.randn(M, K, generator=g), dt)[1]
        Bb = et_bits(torch.randn(N, K, generator=g) / math.sqrt(K), dt)[1]
        bias = dev(torch.randn(N, generator=g))
        Ad, Bd = dev(Ab), dev(Bb)
        ref = Ad.view(dt).double() @ Bd.view(dt).double().t() + bias.double()
        ref_e = F.gelu(ref.float()) if gelu else ref.float()
        del ref
        out = Guarded((M, N), dt)
        assert lib.samrs_k_gemm_ld(prec, Ad.data_ptr(), Bd.data_ptr(), out.ptr, bias.data_ptr(), M, N, K, 0, gelu, gelu_form, stream()) == 0
        dense = dev_window(out, "dense launch").clone()
        _gemm_case.update(key=key, Ab=Ab, Bb=Bb, bias=bias, ref_e=ref_e, dense=dense)
    return _gemm_case


LD_CASES = [("X64P", 4096, 5120, K, K + pad, 0, 1) for K in (128, 192, 1344) for pad in (64, 128)] + \
           [("W4X", 16384, 5120, K, K + 64, 1, form) for K in (256, 320) for form in (1, 2)]


@pytest.mark.parametrize("kernel,M,N,K,ld,gelu,gelu_form", LD_CASES, ids=[f"{c[0]}-K{c[3]}-ld{c[4]}-form{c[6]}" for c in LD_CASES])
@pytest.mark.parametrize("name,prec,dt,ulp", PRECS, ids=PREC_IDS)       # the outer loop: the cases of a shape share their reference
def test_padded_row_gemm(lib, kernel, M, N, K, ld, gelu, gelu_form, name, prec, dt, ulp):
    """operand rows at a stride of ld elements, the pad full of NaN: the bits of the dense launch, finite, and the fp64 product"""
    for stride in (0, ld):
        ch = choice(lib, prec, M, N, K, gelu=gelu, ld=stride)
        assert ch["reject"] == 0 and ch["kernel"] == kernel and ch["ld_ok"] == 1, ch
    c = gemm_case(lib, prec, dt, M, N, K, gelu, gelu_form)
    Ap, Bp = padded(c["Ab"], ld, dt), padded(c["Bb"], ld, dt)
    out = Guarded((M, N), dt)
    assert lib.samrs_k_gemm_ld(prec, Ap.data_ptr(), Bp.data_ptr(), out.ptr, c["bias"].data_ptr(), M, N, K, ld, gelu, gelu_form, stream()) == 0
    got = dev_window(out, "padded launch")
    assert bool(torch.isfinite(got.float()).all()), "the padded launch produced non-finite values (it read its pad columns?)"
    ref_e = c["ref_e"]
    err = ((got.float() - ref_e).abs() / ref_e.abs().clamp(min=1e-2)).max().item()
    same = torch.equal(got.view(torch.int16), c["dense"].view(torch.int16))
    print(f"{kernel} {name} {M}x{N}x{K} ld {ld} gelu {gelu} form {gelu_form}: max rel {err:.2e} ({err / ulp:.2f} ulp), bit-identical with dense: {same}")
    assert same, "the padded launch differs from the dense launch of the same operands"
    assert err < 1.5 * ulp


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS, ids=PREC_IDS)
def test_padded_row_gemm_refusals(lib, name, prec, dt, ulp):
    """strides the kernels' 16-byte DMA pieces do not take, and a stride on a launch that runs on another kernel: refused by the rule and
    by the entry point, nothing launched"""
    M, N, K = 4096, 5120, 128
    A, B = torch.zeros(M, K + 8, dtype=torch.int16).cuda(), torch.zeros(N, K + 8, dtype=torch.int16).cuda()
    out = Guarded((M, N), dt)
    for ld in (K - 8, K + 1, K + 4, K + 6):
        assert choice(lib, prec, M, N, K, ld=ld)["reject"] == 1
        assert lib.samrs_k_gemm_ld(prec, A.data_ptr(), B.data_ptr(), out.ptr, None, M, N, K, ld, 0, 1, stream()) != 0
    assert choice(lib, prec, 256, 128, 64, ld=128)["reject"] == 1                         # the 128 x 128 kernel takes no stride
    assert lib.samrs_k_gemm_ld(prec, A.data_ptr(), B.data_ptr(), out.ptr, None, 256, 128, 64, 128, 0, 1, stream()) != 0
    assert out.untouched()


EXT_SHAPES = [(16384, 1280, 128), (16384, 1280, 192), (16384, 1280, 320), (8192, 2560, 128)]


def tile_norms(x, tm=256, tn=320):
    M, N = x.shape
    return x.double().view(M // tm, tm, N // tn, tn).pow(2).sum((1, 3)).sqrt()


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "no-bias"])
@pytest.mark.parametrize("M,N,K", EXT_SHAPES, ids=[f"{m}x{n}x{k}" for m, n, k in EXT_SHAPES])
def test_ext_stage_gemm(lib, M, N, K, with_bias, name, prec, dt, ulp):
    """C += A B^T + Ax Bx^T + bias with a side product as large as the main one: a dropped or misrouted stage is an O(1) error"""
    ch = choice(lib, prec, M, N, K, out_f32=1, accumulate=1)
    assert ch["ext_ok"] == 1 and (ch["kernel"], ch["ni"], ch["mode"]) == ("X64", 5, 3), ch
    g = gen(M + N + K + with_bias)
    A = dev(et_bits(torch.randn(M, K, generator=g), dt)[1])
    B = dev(et_bits(torch.randn(N, K, generator=g) / math.sqrt(K), dt)[1])
    Ax = dev(et_bits(torch.randn(M, 64, generator=g), dt)[1])
    Bx = dev(et_bits(torch.randn(N, 64, generator=g) / 8.0, dt)[1])
    bias = dev(torch.randn(N, generator=g)) if with_bias else None
    C0 = torch.randn(M, N, generator=g).cuda()
    C = Guarded((M, N), torch.float32)
    dev_window(C, "C0").copy_(C0)
    assert lib.samrs_k_gemm_ext(prec, A.data_ptr(), B.data_ptr(), Ax.data_ptr(), Bx.data_ptr(), C.ptr, ptr(bias), M, N, K, stream()) == 0
    got = dev_window(C, "EXT launch")
    assert bool(torch.isfinite(got).all())

    def formula(dtype):
        r = C0.to(dtype) + A.view(dt).to(dtype) @ B.view(dt).to(dtype).t() + Ax.view(dt).to(dtype) @ Bx.view(dt).to(dtype).t()
        return r + bias.to(dtype) if with_bias else r
    ref64, ref32 = formula(torch.float64), formula(torch.float32)
    r = rel_l2(got, ref64)
    ref_t = tile_norms(ref64)
    err_t, noise_t = tile_norms(got.double() - ref64) / ref_t, tile_norms(ref32.double() - ref64) / ref_t
    bound_t = (8.0 * noise_t).clamp(min=3e-6)
    worst = int((err_t / bound_t).argmax())
    print(f"gemm_ext {name} {M}x{N}x{K} bias {with_bias}: rel L2 {r:.2e}; worst 256 x 320 tile {err_t.flatten()[worst].item():.2e} "
          f"(noise {noise_t.flatten()[worst].item():.2e}, bound {bound_t.flatten()[worst].item():.2e})")
    assert r < 2e-6
    assert bool((err_t <= bound_t).all()), f"{int((err_t > bound_t).sum())} tiles miss their bound"


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS, ids=PREC_IDS)
def test_ext_stage_gemm_refusal(lib, name, prec, dt, ulp):
    M, N, K = 4096, 768, 128
    assert choice(lib, prec, M, N, K, out_f32=1, accumulate=1)["ext_ok"] == 0
    A, B = torch.zeros(M, K, dtype=torch.int16).cuda(), torch.zeros(N, K, dtype=torch.int16).cuda()
    Ax, Bx = torch.zeros(M, 64, dtype=torch.int16).cuda(), torch.zeros(N, 64, dtype=torch.int16).cuda()
    C = Guarded((M, N), torch.float32)
    assert lib.samrs_k_gemm_ext(prec, A.data_ptr(), B.data_ptr(), Ax.data_ptr(), Bx.data_ptr(), C.ptr, None, M, N, K, stream()) != 0
    assert lib.samrs_k_gemm_ext(prec, A.data_ptr(), B.data_ptr(), Ax.data_ptr(), Bx.data_ptr(), C.ptr, None, 16384, 1280, 64, stream()) != 0
    assert C.untouched()


# ------------------------------------------------------------------------------------------------------------------
# producer and consumer chain of proj: the one place where the benefit is measurable (fp32 output)
# ------------------------------------------------------------------------------------------------------------------
CHAIN_M, CHAIN_N, CHAIN_K, CHAIN_HOT, CHAIN_SCALE = 16384, 1280, 128, 4, 3000.0


def chain_operands(dt, device="cpu"):
    """Yf: N(0, 1) activations with CHAIN_HOT columns x CHAIN_SCALE, W: N(0, 1 / K); their two-term splits; the column list"""
    g = gen(4242)
    idx = pick(CHAIN_HOT, CHAIN_K, g)
    Yf = torch.randn(CHAIN_M, CHAIN_K, generator=g)
    Yf[:, idx.long()] *= CHAIN_SCALE
    W = torch.randn(CHAIN_N, CHAIN_K, generator=g) / math.sqrt(CHAIN_K)
    Yhi = Yf.to(dt) if dt != torch.float16 else Yf.clamp(-65504.0, 65504.0).to(dt)
    Ylo = (Yf - Yhi.float()).to(dt)
    Whi = W.to(dt)
    Wlo = (W - Whi.float()).to(dt)
    return [t.to(device) for t in (idx, Yf, W, Yhi, Ylo, Whi, Wlo)]


def chain_emulation(dt, device="cpu", dtype=torch.float64):
    """In `dtype` (float64: exact to 1e-16): the reference (un-rounded Yf and W on the hot columns, the ET-rounded values elsewhere),
    what the chain computes (hi x hi everywhere + lo x hi + hi x lo on the hot columns: the reference minus lo x lo and the rounding
    of lo) and what the plain launch computes (hi x hi).  CHAIN_SCALE and CHAIN_HOT were chosen with this function on the CPU: at
    x3000 on 4 of 128 columns the hot columns carry all but 3.4e-6 of the output's energy, the plain product misses the reference by
    the operands' rounding (rel L2 2.9e-4 f16, 2.4e-3 bf16) and the chain by lo x lo and lo's rounding (2.1e-7 f16, 4.5e-6 bf16),
    against bounds of 3.2e-6 and 1.8e-5."""
    idx, Yf, W, Yhi, Ylo, Whi, Wlo = chain_operands(dt, device)
    h = idx.long()
    c = lambda t: t.to(dtype)  # noqa: E731
    plain = c(Yhi) @ c(Whi).t()
    hot_hi = c(Yhi)[:, h] @ c(Whi)[:, h].t()
    ref = plain - hot_hi + c(Yf)[:, h] @ c(W)[:, h].t()
    chain = plain + c(Ylo)[:, h] @ c(Whi)[:, h].t() + c(Yhi)[:, h] @ c(Wlo)[:, h].t()
    return ref, chain, plain


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS, ids=PREC_IDS)
def test_proj_chain_gains_what_the_split_promises(lib, name, prec, dt, ulp):
    """outlier_gather -> outlier_weight_ext (ld = 64) -> samrs_k_gemm_ext with C0 = 0, against fp64; the plain launch of the same
    operands without the side product is the power check"""
    M, N, K, p = CHAIN_M, CHAIN_N, CHAIN_K, SIG_BITS[dt]
    assert choice(lib, prec, M, N, K, out_f32=1, accumulate=1)["ext_ok"] == 1
    idx, Yf, W, Yhi, Ylo, Whi, Wlo = chain_operands(dt, "cuda")
    ref64, emu_chain, emu_plain = chain_emulation(dt, "cuda")
    ref32 = chain_emulation(dt, "cuda", torch.float32)[0]
    bound, noise = fp32_bound(ref32, ref64)
    bound += 2.0 ** (-2 * p)                                           # the dropped lo x lo term
    idxd, Wd = i32(idx), W.contiguous()
    Ax, Bx = Guarded((M, 64), dt), Guarded((N, 64), dt)
    assert lib.samrs_k_outlier_gather(Yhi.data_ptr(), Ylo.data_ptr(), K, idxd.data_ptr(), CHAIN_HOT, Ax.ptr, M, stream()) == 0
    assert lib.samrs_k_outlier_weight_ext(prec, Wd.data_ptr(), N, K, idxd.data_ptr(), CHAIN_HOT, Bx.ptr, 64, 0, stream()) == 0
    C = Guarded((M, N), torch.float32)
    dev_window(C, "C0").zero_()
    assert lib.samrs_k_gemm_ext(prec, Yhi.data_ptr(), Whi.data_ptr(), Ax.ptr, Bx.ptr, C.ptr, None, M, N, K, stream()) == 0
    got = dev_window(C, "chain")
    assert bool(torch.isfinite(got).all())
    P = Guarded((M, N), torch.float32)
    dev_window(P, "P0").zero_()
    assert lib.samrs_k_gemm(prec, Yhi.data_ptr(), Whi.data_ptr(), P.ptr, None, None, 0, M, N, K, 1, 0, 1, stream()) == 0
    plain = dev_window(P, "plain")
    r_chain, r_plain = rel_l2(got, ref64), rel_l2(plain, ref64)
    e_chain, e_plain = rel_l2(emu_chain, ref64), rel_l2(emu_plain, ref64)
    print(f"proj chain {name}: chain rel L2 {r_chain:.2e} (fp64 emulation of the chain {e_chain:.2e}; noise {noise:.2e}, bound {bound:.2e}), "
          f"plain launch {r_plain:.2e} (emulation {e_plain:.2e})")
    assert e_plain >= 10.0 * bound, "the setup has no power: the plain product is within 10 x the chain's bound"
    assert r_chain <= bound
    assert r_plain >= 10.0 * r_chain

"""GPU: the three entry points of the mask upscaler alone -- samrs_k_upscaler_fused (upscaler_fused.hip, route ONE_KERNEL),
samrs_k_gemm_gln (the GLN flavour of gemm_et_dual_kernel, gemm_dual.hip) and samrs_k_upscale2_masks (upscale2_mask_kernel,
decoder_kernels.hip; routes GLN and GLN_SPLIT run the last two in a row) -- per element against a float64 CPU statement of
mask_decoder.py:53-59,154-167 on the same already-rounded operands, at the shapes the engine runs them at: the persistent walk of the
fused kernel (more tiles than blocks, a block's consecutive tiles in different prompts), every k-tile count around the three-stage
ring of the GLN GEMM, its grouped block mapping with a full and a partial group of m tiles.

Conventions (those of tests/test_decoder_kernels_gpu.py, whose helpers are imported)
  * Every output is [guard | window | guard], pre-filled with the NaN pattern of its type; afterwards every window element is finite
    and both guards are bit-for-bit untouched (`Guarded`).
  * Un-split: keys / A, both weight matrices and U1 are rounded to the element type on the host.  Split: every operand is hi + lo,
    hi = ET(x), lo = ET(x - hi), and the reference takes the EXACT fp64 sum hi + lo as the operand.
  * u = 2^-11 (f16) | 2^-8 (bf16), tau = 2^-25 (f16) | 0 (bf16) as in tests/test_encoder_attention_gpu.py; U = 2^-24.

The per-element bound (`ln_gelu_bound`, `stage2_bound`, `mask_bound`; every E below is an absolute error bound in fp64, per element)
  GEMM        y = sum_j a_j b_j + bias.  Products of two ET values are exact in fp32 (22 | 16 significand bits).  An accumulator that nm
              MFMA instructions are chained on is rounded twice per instruction (the sum of its 32 products, the add to the
              accumulator) and twice more (meeting the other K half / the bias), each rounding relative to a partial sum of at most
              S = sum_j |a_j||b_j|:   E_y = ((2 nm + 2) U + u'^2) S + U |bias|,   u' = u (1 + u) and the u'^2 term -- the dropped
              lo x lo products -- in split mode only.  nm: fused ConvT #1 4 (12 split), GLN GEMM K / 32 (3 K / 32), ConvT #2 2 (6).
  LayerNorm   over 64 channels, mean first: E_m = mean E_y + 18 U mean |y| (a value passes 16 serial and 2 cross-lane adds),
              v = y - m: E_v = E_y + E_m + U |v|, var = mean v^2: E_var = mean (2 |v| E_v + E_v^2) + 20 U var, w = var + eps,
              rstd = w^-1/2 with relative error rho = (w / (w - E_var))^1/2 - 1 + 3 U (the add, the root, the division),
              z = v rstd gamma + beta:   E_z = |gamma| rstd (E_v + |v| (rho + 2 U)) (1 + rho) + U |z|.
  GELU        E_g = 1.13 E_z + G(z), 1.13 >= max |gelu'|, and G the error of the kernels' erfc (Abramowitz-Stegun 7.1.26, absolute
              error 1.5e-7 on erfc, times |x| / 2) and of its fp32 evaluation: G(x) = 0.75e-7 |x| + U ((64 + 2 x^2) h + |gelu(x)|),
              h = |x| erfc(|x| / sqrt 2) / 2 the term the polynomial, the reciprocal and the exp2 (argument error U x^2) produce.
  operand 2   split: g is split in registers, E_op = E_g + u'^2 (|g| + E_g) + tau.  Un-split: g is rounded to ET, and fp32 noise can
              push it to the other neighbour than the fp64 reference's: E_op = E_g + 2 u (|g| + E_g) + tau, one ET step.
  ConvT #2    E_y2 = sum_k |w2_ck| E_op_k + the GEMM term on S2 = sum_k |w2_ck||op_k|;  E_g2 = 1.13 E_y2 + G(y2).
  dot         E = sum_c |hyper_c| E_g2_c + 12 U sum_c |hyper_c||g2_c| (a product, two 4-term partial sums, 2 cross-lane adds).
Asserted: max |got - ref| / E <= 1.  The constants count roundings, none is fitted to a kernel; the same chain evaluated by torch in
float32 on the CPU must stay under the bound as well (asserted in every case before the kernel runs: if it does not, the bound is
wrong).  The fused kernel also keeps the rel-L2 check of the old tests, with the bound taken from the reference as `fp32_bound` does:
rel L2 <= max(8 x the rel L2 of the float32 restatement against fp64, 3e-6).  Un-split it is applied to what exceeds one ET step of
every g_k (`et_excess` style: sum_c |hyper_c| 1.13 sum_k |w2_ck| (2 u |g_k| + tau) is taken off |err| first, on both sides): the
plain rel L2 is a count of a few hundred to a handful of flipped neighbours (bf16, 256 tokens: 2e-6 for float32 on the CPU, 3e-5 for
the kernel, both far inside the per-element bound), so 8 x one such count bounds nothing; it is printed.  Split, both sides of it are the kernel's own algebra in place of the exact chain (`fused_chain`, model):
the two products without their lo x lo terms and g as its two-term split, so that only fp32 rounding is left to be measured -- the
per-element bound sums absolute values over 64 x 32 terms and is 10 to 1000 times the error of a correct kernel, this one is not.
GLN GEMM, ET output: what exceeds the final rounding, |got - ref| - u |ref| - tau clamped at 0, against E_g (1 + u).

Input families of the fused kernel (seeded, `fused_x`; GLN: the same through `bias` and zero rows of A)
  uniform     keys N(0, 1), w1 N(0, 1) / 16, b1 0.3 N, gamma 1 + 0.2 N, beta 0.2 N, w2 N / 8, b2 0.3 N, hyper N(0, 1)
  eps         per prompt tokens 0, 17 and the last have all-zero keys, so y = b1 exactly there; b1 of group 1 is 0.5 + 1e-3 N(0, 1)
              (variance of the order of eps: with eps = 1e-5 the reference leaves the bound on such rows of every prompt, asserted) and b1 of
              group 2 is exactly 0.25 (variance 0, rstd = eps^-1/2, output GELU(beta) through the chain; NaN with eps dropped)
  bigmean     b1 of group 3 + 50 against deviations of order 1
  tails       w2 and b2 x 4: the second GELU's arguments pass -6 and +6 (asserted)
  zero_hyper  the hyper rows of prompt 1 all zero: its outputs are exactly 0.0
  same        prompts 0, 1, 2 share their keys, prompt 2 also the hyper rows of prompt 0: low[2] == low[0] bit for bit, low[1] is
              held to the reference like every other case
  probe       ConvT #2 and the dot made transparent: every row of w2 holds a single 1 (output channel (s2, c2) reads channel
              (32 s2 + c2) % 64), every hyper row two ones: an output is the sum of two GELU(g_k + b2) and the bound carries no
              sum over 64 x 32 absolute values -- an error of the first stage of 1e-5 is visible

Bit for bit: low[b] of a persistent-walk launch == low of an n = 1 launch (one tile per block, no walk, no prefetch) on prompt b's
keys and hyper rows, for every b; three repeats of the walk launch are identical; GLN rows do not depend on M.

Measured on the kernels as they stand (MI355X, 256 CUs: walk12 = 3 prompts, 384 tiles; walk23 = 5 prompts, 640 tiles).  Worst
|got - ref| / E of each group, the bound being 1; in brackets the float32 restatement on the CPU against the same E.

  kernel     group                                    f16 plain      f16 split      bf16 plain     bf16 split
  ---------  ---------------------------------------  -------------  -------------  -------------  -------------
  fused      uniform, one tile per block (4 shapes)   0.040 (0.028)  0.000 (0.000)  0.017 (0.011)  0.001 (0.000)
  fused      uniform, persistent walk (walk12 / 23)   0.037 (0.048)  0.000 (0.000)  0.023 (0.032)  0.001 (0.000)
  fused      eps                                      0.023 (0.023)  0.002 (0.002)  0.006 (0.007)  0.010 (0.001)
  fused      bigmean                                  0.022 (0.022)  0.001 (0.002)  0.012 (0.012)  0.001 (0.000)
  fused      tails (arguments in [-13.6, 13.5])       0.013 (0.016)  0.000 (0.000)  0.002 (0.007)  0.001 (0.000)
  fused      zero_hyper / same                        0.012 (0.012)  0.000 (0.000)  0.002 (0.000)  0.001 (0.000)
  fused      probe                                    0.341 (0.371)  0.006 (0.011)  0.214 (0.305)  0.014 (0.001)
  fused      rel L2 / its bound, worst of all cases   0 (nothing beyond one ET step)  split: f16 0.083, bf16 0.116
             plain rel L2 (float32 on the CPU)        1.8e-5 (1.5e-5)  2.5e-7 (3.8e-7)  3.7e-5 (4.0e-5)  2.1e-6 (2.3e-6)
  gemm_gln   uniform, 13 shapes                       0.009 (0.040)  0.042 (0.071)  0.006 (0.024)  0.076 (0.005)
  gemm_gln   eps                                      0.012 (0.014)  0.083 (0.069)  0.001 (0.007)  0.083 (0.069)
  gemm_gln   bigmean                                  0.033 (0.036)  0.059 (0.074)  0.025 (0.036)  0.038 (0.023)
  upscale2   3 grids x 2 n x 3 selections             0.047 (0.081)  0.020 (0.029)  0.042 (0.052)  0.019 (0.001)
  routes     GLN -> upscale2 on the kernel's own U1   0.040          0.020          0.037          0.023
             against the fused kernel: max |diff|     9.7e-4         5.7e-6         2.9e-3         5.7e-5
             (rel L2; elements of 36864 that differ)  6.5e-6; 27175  2.2e-7; 31524  1.1e-5; 22405  8.4e-7; 31640

Every bit-for-bit check held (walk == no walk for every prompt, repeats, same keys, GLN rows independent of M), no case missed a bound
and no kernel was changed; the per-element bound is loose by the factor a sum of absolute values over 64 x 32 terms costs, `probe` and
the split rel L2 are the sharp ends.  255 cases, 15 s on the MI355X.

What the nine one-line mutations of the issue do (each built in a scratch copy, values only with every address in range, run once
against this file and the five old upscaler tests of tests/test_kernels_gpu.py and tests/test_upscaler_tile32_gpu.py; none is committed)
  a fused, the prefetch reads tile `tile`, not `nt`        the 24 walk value cases and the 8 walk bit cases only; old tests: none at their
                                                           old shapes (the (3, 64) shape added to test_upscaler_tile32_gpu.py: all 8)
  b fused, b = blockIdx.x / tiles_per_prompt               the same 24 + 8; old tests: none at their old shapes (the new (3, 64): 8)
  c fused, 1e-6f -> 1e-5f                                  per element: the 8 `eps` cases only (ratio 2.0 .. 15.5); the split rel L2 sees
                                                           it in all 50 split cases too (uniform: 5.5e-6 against 3e-6); old tests: none
  d fused, a.sel0 + c -> c                                 the 72 cases with sel0 > 0; old: the 4 + 8 cases with sel0 = 1
  e fused split, the wl1 x af MFMAs dropped                the 50 split cases only (rel L2 1.9e-4 f16, 1.5e-3 bf16; per element only
                                                           `probe`: 7.1 / 7.0); old: the 4 + 8 split cases
  f fused, hg exchanged in the Out index                   all 100 value cases (the walk bit cases compare the kernel with itself: pass);
                                                           old: all 8 + 16
  g GLN, gamma and beta offsets exchanged                  all 68 gemm_gln cases; old: both tests, both types.  test_routes_gln_then_upscale2
                                                           takes the kernel's own U1 and passes, as designed
  h upscale2, the two sub-pixel-2 bits exchanged           all 72 upscale2 cases and the 4 route cases; old: all 4
  i fused, first GELU in the tanh form (max 4.7e-4 off)    split: all 50 cases by rel L2 (1.6e-4 .. 1.9e-4), per element `probe` f16
                                                           (3.9; bf16 0.41).  Un-split: `probe` alone (4.3 f16, 2.5 bf16), every other
                                                           un-split case passes (ratio <= 0.24); old: 8 of their 12 split cases, no un-split one
"""
import functools
import math
import types

import pytest
import torch
import torch.nn.functional as F

from test_decoder_kernels_gpu import Guarded, dev, et_bits, fp32_bound, gen, rel_l2, round_et64, stream
from test_encoder_attention_gpu import TAU_ET, U_ET

pytestmark = pytest.mark.gpu

DT = {"f16": (1, torch.float16), "bf16": (0, torch.bfloat16)}
MODES = [(name, split) for name in DT for split in (False, True)]
U24 = 2.0 ** -24
GELU_SLOPE = 1.13
ERFC_AS = 1.5e-7
BAD = (-2, -3)                       # SAMRS_ERR_BAD_SHAPE, SAMRS_ERR_BAD_ARG
NS = types.SimpleNamespace


@pytest.fixture(scope="module")
def lib():
    from samrs_amd import engine
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return engine.load_library()


# ------------------------------------------------------------------------------------------------------------------
# operands and the bound's building blocks (CPU, fp64)
# ------------------------------------------------------------------------------------------------------------------
def operand(x, dt, split):
    """fp32 tensor -> v (the exact fp64 value the kernel's operand stands for), hi / lo bit patterns (lo None un-split)"""
    hi, hib = et_bits(x, dt)
    if not split:
        return NS(v=hi.double(), hi=hib, lo=None, lov=None)
    lo, lob = et_bits(x - hi, dt)                  # x - hi is exact in fp32
    return NS(v=hi.double() + lo.double(), hi=hib, lo=lob, lov=lo.double())


def u2_of(dt, split):
    return (U_ET[dt] * (1.0 + U_ET[dt])) ** 2 if split else 0.0


def gemm_bound(a, b, bias, nm, u2):
    """y = a b^T + bias [rows, cols] and E_y; a, b fp64 exact operand values, nm chained MFMA instructions per accumulator"""
    y = a @ b.t() + bias
    s = a.abs() @ b.abs().t()
    return y, ((2 * nm + 2) * U24 + u2) * s + U24 * bias.abs()


def gelu_err(x):
    ax = x.abs()
    h = 0.5 * ax * torch.erfc(ax / math.sqrt(2.0))
    return 0.5 * ERFC_AS * ax + U24 * ((64.0 + 2.0 * x * x) * h + F.gelu(x).abs())


def ln_gelu_bound(y, Ey, gamma, beta, eps):
    """y, E_y [..., 64] -> g = GELU(LN(y) gamma + beta), E_g"""
    m = y.mean(-1, keepdim=True)
    Em = Ey.mean(-1, keepdim=True) + 18 * U24 * y.abs().mean(-1, keepdim=True)
    v = y - m
    Ev = Ey + Em + U24 * v.abs()
    var = (v * v).mean(-1, keepdim=True)
    Evar = (2 * v.abs() * Ev + Ev * Ev).mean(-1, keepdim=True) + 20 * U24 * var
    w = var + eps
    rstd = w.rsqrt()
    rho = (w / (w - Evar).clamp(min=1e-300)).sqrt() - 1.0 + 3 * U24
    z = v * rstd * gamma + beta
    Ez = gamma.abs() * rstd * (Ev + v.abs() * (rho + 2 * U24)) * (1.0 + rho) + U24 * z.abs()
    return F.gelu(z), GELU_SLOPE * Ez + gelu_err(z)


def operand2_bound(g, Eg, dt, split):
    """the operand of ConvT #2 the reference uses, and its E_op"""
    u, tau = U_ET[dt], TAU_ET[dt]
    if split:
        return g, Eg + u2_of(dt, True) * (g.abs() + Eg) + tau
    return round_et64(g, dt), Eg + 2 * u * (g.abs() + Eg) + tau


def stage2_bound(op, Eop, w2, b2, dt, split):
    """op, E_op [rows, 64] -> g2 = GELU(op w2^T + b2) [rows, 128 = (s2, c2)], E_g2, y2"""
    y2, Ey2 = gemm_bound(op, w2, b2, 6 if split else 2, u2_of(dt, split))
    Ey2 = Ey2 + Eop @ w2.abs().t()
    return F.gelu(y2), GELU_SLOPE * Ey2 + gelu_err(y2), y2


def pixels(t, n, grid):
    """[n tokens 4 = (b, y, x, dy, dx), 128 = (dy2, dx2, c)] -> [n, Y, X, c], Y = 4 y + 2 dy + dy2, X = 4 x + 2 dx + dx2: a permutation
    of the axes (as test_mask_product states it), not index arithmetic"""
    return t.view(n, grid, grid, 2, 2, 2, 2, 32).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(n, 4 * grid, 4 * grid, 32)


def rows_of(m, n, grid):
    """inverse of `pixels` for a mask tensor [n, c, Y, X] -> [n tokens 4, c 4]: the 4 c values of each (token, sub-pixel 1)"""
    c = m.shape[1]
    return m.view(n, c, grid, 2, 2, grid, 2, 2).permute(0, 2, 5, 3, 6, 1, 4, 7).reshape(n * grid * grid * 4, c * 4)


def masks(t, sel, n, grid):
    return torch.einsum("bck,byxk->bcyx", sel.to(t.dtype), pixels(t, n, grid))


def mask_bound(g2, Eg2, sel, n, grid):
    """-> ref [n, n_sel, 4 grid, 4 grid], E"""
    return masks(g2, sel, n, grid), masks(Eg2, sel.abs(), n, grid) + 12 * U24 * masks(g2.abs(), sel.abs(), n, grid)


def ratio(got, ref, bound):
    return ((got.double() - ref).abs() / bound.clamp(min=1e-300)).max().item()


def ptr(t, off=0):
    return None if t is None else t.data_ptr() + off


# ------------------------------------------------------------------------------------------------------------------
# 1. samrs_k_upscaler_fused
# ------------------------------------------------------------------------------------------------------------------
SELS = [(1, 0), (3, 1), (1, 3)]                 # (n_sel, sel0) at n_mask_tokens = 4: the engine's two, and the last mask token
SHAPES = [(1, 16), (3, 16), (1, 32), (1, 64), ("walk12", 64), ("walk23", 64)]
ZERO_TOKENS = lambda tokens: [0, 17, tokens - 1]


def walk_n(kind, tiles_per_prompt=128):
    """prompts at grid 64 (128 tiles of 32 tokens each) for which every block walks 1 - 2 (walk12) or 2 - 3 (walk23) tiles; on 256
    CUs n = 3 (384 tiles) and n = 5 (640 tiles)"""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    lo = 1 if kind == "walk12" else 2
    n = lo * cu // tiles_per_prompt + 1
    n_tiles = n * tiles_per_prompt
    assert lo * cu < n_tiles < (lo + 1) * cu, f"{kind}: {n_tiles} tiles on {cu} CUs do not make blocks walk {lo} - {lo + 1} tiles"
    # a block's consecutive tiles t, t + cu lie in different prompts whenever a prompt has no more tiles than there are blocks
    assert cu >= tiles_per_prompt and n > 1
    return n


def shape_of(shape):
    n, grid = shape
    return (walk_n(n), grid) if isinstance(n, str) else (n, grid)


@functools.lru_cache(maxsize=4)
def fused_x(family, n, grid, name, split):
    prec, dt = DT[name]
    g = gen(7000 + 131 * n + grid)
    tokens = grid * grid
    keys = torch.randn(n * tokens, 256, generator=g)
    w1 = torch.randn(256, 256, generator=g) / 16
    b1 = 0.3 * torch.randn(256, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(64, generator=g), 0.2 * torch.randn(64, generator=g)
    w2 = torch.randn(128, 64, generator=g) / 8
    b2 = 0.3 * torch.randn(128, generator=g)
    hyper = torch.randn(n, 4, 32, generator=g)
    zero_rows = []
    if family == "eps":
        zero_rows = [b * tokens + t for b in range(n) for t in ZERO_TOKENS(tokens)]
        keys[zero_rows] = 0.0
        b1[64:128] = 0.5 + 1e-3 * torch.randn(64, generator=g)
        b1[128:192] = 0.25
    elif family == "bigmean":
        b1[192:256] += 50.0
    elif family == "tails":
        w2, b2 = 4.0 * w2, 4.0 * b2
    elif family == "zero_hyper":
        hyper[1] = 0.0
    elif family == "same":
        keys[tokens:2 * tokens] = keys[:tokens]
        keys[2 * tokens:3 * tokens] = keys[:tokens]
        hyper[2] = hyper[0]
    elif family == "probe":
        r = torch.arange(128)
        w2 = torch.zeros(128, 64)
        w2[r, (32 * (r // 32) + r % 32) % 64] = 1.0
        hyper = torch.zeros(n, 4, 32)
        for b in range(n):
            for m in range(4):
                hyper[b, m, (5 * b + 7 * m) % 32] = 1.0
                hyper[b, m, (5 * b + 7 * m + 13) % 32] = 1.0
    else:
        assert family == "uniform"
    return NS(family=family, n=n, grid=grid, tokens=tokens, name=name, prec=prec, dt=dt, split=split, keys=operand(keys, dt, split),
              w1=operand(w1, dt, split), w2=operand(w2, dt, split), b1=b1, gamma=gamma, beta=beta, b2=b2, hyper=hyper,
              zero_rows=zero_rows, d=None)


def fused_chain(x, dtype, eps=1e-6, model=False):
    """the plain restatement of the chain in `dtype` (float64: the reference; float32: the noise measure) -> g2 [rows 4, 128].
    model (split): the kernel's own algebra -- both products without their lo x lo term, g as the two-term split of itself"""
    c = lambda t: t.to(dtype)
    rnd = lambda t: round_et64(t, x.dt) if dtype == torch.float64 else t.to(x.dt).to(dtype)
    model = model and x.split
    y = c(x.keys.v) @ c(x.w1.v).t()
    if model:
        y = y - c(x.keys.lov) @ c(x.w1.lov).t()
    y = (y + c(x.b1)).view(-1, 4, 64)
    v = y - y.mean(-1, keepdim=True)
    g = F.gelu(v * torch.rsqrt((v * v).mean(-1, keepdim=True) + eps) * c(x.gamma) + c(x.beta)).reshape(-1, 64)
    if not x.split:
        g = rnd(g)
    if model:
        hi = rnd(g)
        lo = rnd(g - hi)
        return F.gelu((hi + lo) @ c(x.w2.v).t() - lo @ c(x.w2.lov).t() + c(x.b2))
    return F.gelu(g @ c(x.w2.v).t() + c(x.b2))


@functools.lru_cache(maxsize=1)
def fused_ref(family, n, grid, name, split):
    x = fused_x(family, n, grid, name, split)
    y, Ey = gemm_bound(x.keys.v, x.w1.v, x.b1.double(), 12 if split else 4, u2_of(x.dt, split))
    g, Eg = ln_gelu_bound(y.view(-1, 4, 64), Ey.view(-1, 4, 64), x.gamma.double(), x.beta.double(), 1e-6)
    op, Eop = operand2_bound(g.reshape(-1, 64), Eg.reshape(-1, 64), x.dt, split)
    g2, Eg2, y2 = stage2_bound(op, Eop, x.w2.v, x.b2.double(), x.dt, split)
    g2_32 = fused_chain(x, torch.float32)
    # un-split: what one ET step of every g_k can move an output of ConvT #2 + GELU by (the flip part of E_g2 alone)
    flip2 = None if split else GELU_SLOPE * ((2 * U_ET[x.dt] * g.reshape(-1, 64).abs() + TAU_ET[x.dt]) @ x.w2.v.abs().t())
    return NS(g2=g2, Eg2=Eg2, flip2=flip2, y2min=y2.min().item(), y2max=y2.max().item(), g2_32=g2_32,
              m64=fused_chain(x, torch.float64, model=True) if split else g2, m32=fused_chain(x, torch.float32, model=True) if split else g2_32)


def upload(x):
    if x.d is None:
        o = lambda t: None if t is None else dev(t)
        x.d = NS(keys=dev(x.keys.hi), keys_lo=o(x.keys.lo), w1=dev(x.w1.hi), w1_lo=o(x.w1.lo), w2=dev(x.w2.hi), w2_lo=o(x.w2.lo),
                 b1=dev(x.b1), ln=dev(torch.cat([x.gamma, x.beta])), b2=dev(x.b2), hyper=dev(x.hyper))
    return x.d


def launch_fused(lib, x, n_sel, sel0, b0=0, n=None):
    """prompts b0 .. b0 + n - 1 of the case (all by default) -> (rc, Guarded low)"""
    d = upload(x)
    n = x.n if n is None else n
    S = 4 * x.grid
    out = Guarded((n, n_sel, S, S), torch.float32)
    ko = b0 * x.tokens * 256 * 2
    rc = lib.samrs_k_upscaler_fused(x.prec, ptr(d.keys, ko), ptr(d.keys_lo, ko), ptr(d.w1), ptr(d.w1_lo), ptr(d.b1), ptr(d.ln), ptr(d.w2),
                                    ptr(d.w2_lo), ptr(d.b2), ptr(d.hyper, b0 * 4 * 32 * 4), out.ptr, n, x.grid, 4, sel0, n_sel, stream())
    return rc, out


def fused_expected(family, n, grid, name, split, n_sel, sel0):
    """everything of a case that needs no GPU -> x, ref, E, the float32 restatement's worst error / E (asserted <= 1) and its masks"""
    x, r = fused_x(family, n, grid, name, split), fused_ref(family, n, grid, name, split)
    what = f"upscaler_fused {family} n={n} grid={grid} {name} split={split} n_sel={n_sel} sel0={sel0}"
    sel = x.hyper[:, sel0:sel0 + n_sel].double()
    ref, E = mask_bound(r.g2, r.Eg2, sel, n, grid)
    ref32 = masks(r.g2_32, sel.float(), n, grid).double()
    cpu = ratio(ref32, ref, E)
    assert cpu <= 1.0, f"{what}: the float32 restatement leaves the bound (ratio {cpu:.3f}): the bound is wrong, not the kernel"
    if family == "eps":
        # eps = 1e-5 would leave the bound on every (zero-key token, group 1) row: the case shows the eps VALUE
        off = rows_of((masks(fused_chain(x, torch.float64, 1e-5), sel, n, grid) - ref).abs() / E, n, grid).amax(1)
        rows1 = torch.tensor(x.zero_rows) * 4 + 1
        per_prompt = off[rows1].view(n, -1).amax(1)
        print(f"{what}: reference with eps 1e-5 on the zero-key rows of group 1: |diff| / bound min {off[rows1].min().item():.1f}, "
              f"the least of the prompts' maxima {per_prompt.min().item():.1f}")
        assert bool((per_prompt > 1.0).all())
    if family == "tails":
        print(f"{what}: second GELU arguments in [{r.y2min:.2f}, {r.y2max:.2f}]")
        assert r.y2min <= -6.0 and r.y2max >= 6.0
    flip = torch.zeros_like(ref) if split else masks(r.flip2, sel.abs(), n, grid)
    return x, what, ref, E, cpu, (masks(r.m64, sel, n, grid), masks(r.m32, sel.float(), n, grid).double(), flip)


FUSED_CASES = [(family, shape, name, split, sel)
               for family, shapes, sels in (("uniform", SHAPES, SELS), ("eps", [(3, 16)], [(3, 1), (1, 0)]), ("bigmean", [(3, 16)], [(3, 1)]),
                                            ("tails", [(3, 16)], [(3, 1)]), ("zero_hyper", [(3, 16)], [(3, 1)]),
                                            ("same", [(3, 16)], [(3, 1)]), ("probe", [(3, 16)], [(3, 1)]))
               for shape in shapes for name, split in MODES for sel in sels]


@pytest.mark.parametrize("family,shape,name,split,sel", FUSED_CASES,
                         ids=[f"{f}-{s[0]}x{s[1]}-{n}-{'split' if sp else 'plain'}-sel{c[0]}at{c[1]}" for f, s, n, sp, c in FUSED_CASES])
def test_upscaler_fused(lib, family, shape, name, split, sel):
    n, grid = shape_of(shape)
    n_sel, sel0 = sel
    x, what, ref, E, cpu, (model64, model32, flip) = fused_expected(family, n, grid, name, split, n_sel, sel0)
    rc, out = launch_fused(lib, x, n_sel, sel0)
    assert rc == 0
    got = out.read(what)
    worst = ratio(got, ref, E)
    excess = lambda t: (((t.double() - model64).abs() - flip).clamp(min=0.0).norm() / model64.norm()).item()
    noise = excess(model32)
    bound = max(8.0 * noise, 3e-6)
    rl2 = excess(got)
    line = (f"{what}: worst |err| / bound {worst:.3f} (float32 on the CPU {cpu:.3f}); rel L2 {'' if split else 'beyond one ET step of g '}"
            f"{rl2:.2e} (bound {bound:.2e}, float32 restatement {noise:.2e}); plain rel L2 {rel_l2(got, model64):.2e} (float32 restatement "
            f"{rel_l2(model32, model64):.2e})")
    print(line)
    assert worst <= 1.0, line
    assert rl2 <= bound, line
    if family == "zero_hyper":
        assert bool((got[1] == 0.0).all()), "zero hyper rows must give exactly 0.0"
    if family == "same":
        bits = out.bits()
        assert torch.equal(bits[2], bits[0]), "same keys, same hyper rows: different bits"
        assert not torch.equal(bits[1], bits[0])


@pytest.mark.parametrize("name,split", MODES)
@pytest.mark.parametrize("walk", ["walk12", "walk23"])
def test_upscaler_fused_walk_is_bit_identical_to_one_tile_per_block(lib, walk, name, split):
    """A tile's arithmetic has the same operands and order whichever block runs it (header of upscaler_fused.hip): low[b] of the walk
    launch == an n = 1 launch (128 tiles, one per block) on prompt b's keys and hyper rows; three walk launches agree."""
    n = walk_n(walk)
    x = fused_x("uniform", n, 64, name, split)
    runs = []
    for _ in range(3):
        rc, out = launch_fused(lib, x, 3, 1)
        assert rc == 0
        out.read(f"walk launch n={n}")
        runs.append(out.bits())
    assert torch.equal(runs[1], runs[0]) and torch.equal(runs[2], runs[0]), "repeated walk launches differ"
    for b in range(n):
        rc, one = launch_fused(lib, x, 3, 1, b0=b, n=1)
        assert rc == 0
        one.read(f"n = 1 launch on prompt {b}")
        diff = int((one.bits()[0] != runs[0][b]).sum())
        assert diff == 0, f"{walk} n={n} {name} split={split}: prompt {b}: {diff} elements differ from the launch without a walk"


# ------------------------------------------------------------------------------------------------------------------
# 2. samrs_k_gemm_gln
# ------------------------------------------------------------------------------------------------------------------
GLN_ZERO_ROWS = lambda M: [0, 100, M - 1]


@functools.lru_cache(maxsize=2)
def gln_x(family, M, N, K, name, split):
    prec, dt = DT[name]
    g = gen(9000 + M + 3 * N + 7 * K)
    A = torch.randn(M, K, generator=g)
    B = torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = 0.5 * torch.randn(N, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(64, generator=g), 0.2 * torch.randn(64, generator=g)
    if family == "eps":
        A[GLN_ZERO_ROWS(M)] = 0.0
        bias[64:128] = 0.5 + 1e-3 * torch.randn(64, generator=g)
        bias[128:192] = 0.25
    elif family == "bigmean":
        bias[192:256] += 50.0
    else:
        assert family == "uniform"
    x = NS(M=M, N=N, K=K, prec=prec, dt=dt, split=split, A=operand(A, dt, split), B=operand(B, dt, split), bias=bias, gamma=gamma, beta=beta)
    y, Ey = gemm_bound(x.A.v, x.B.v, bias.double(), (3 if split else 1) * K // 32, u2_of(dt, split))
    g64, Eg = ln_gelu_bound(y.view(M, -1, 64), Ey.view(M, -1, 64), gamma.double(), beta.double(), 1e-6)
    x.ref, x.E = g64.view(M, N), Eg.view(M, N)
    o = lambda t: None if t is None else dev(t)
    x.d = NS(A=dev(x.A.hi), A_lo=o(x.A.lo), B=dev(x.B.hi), B_lo=o(x.B.lo), bias=dev(bias), gb=dev(torch.cat([gamma, beta])))
    return x


def gln_chain(x, dtype, eps=1e-6):
    c = lambda t: t.to(dtype)
    y = (c(x.A.v) @ c(x.B.v).t() + c(x.bias)).view(x.M, -1, 64)
    v = y - y.mean(-1, keepdim=True)
    return F.gelu(v * torch.rsqrt((v * v).mean(-1, keepdim=True) + eps) * c(x.gamma) + c(x.beta)).view(x.M, x.N)


def launch_gln(lib, x, row0=0, M=None):
    M = x.M if M is None else M
    out = Guarded((M, x.N), torch.float32 if x.split else x.dt)
    ao = row0 * x.K * 2
    rc = lib.samrs_k_gemm_gln(x.prec, ptr(x.d.A, ao), ptr(x.d.B), out.ptr, ptr(x.d.bias), ptr(x.d.gb), M, x.N, x.K, ptr(x.d.A_lo, ao),
                              ptr(x.d.B_lo), stream())
    return rc, out


def gln_ratio(x, got, ref, E):
    """split: |err| / E_g.  ET output: (|err| - u |ref| - tau)+ / (E_g (1 + u))"""
    err = (got.double() - ref).abs()
    if x.split:
        return (err / E).max().item()
    u, tau = U_ET[x.dt], TAU_ET[x.dt]
    return ((err - u * ref.abs() - tau).clamp(min=0.0) / (E * (1.0 + u))).max().item()


def gln_expected(family, M, N, K, name, split):
    """what needs no GPU: the case with its reference and bound, the float32 restatement's ratio (asserted <= 1)"""
    x = gln_x(family, M, N, K, name, split)
    what = f"gemm_gln {family} {M}x{N}x{K} {name} split={split}"
    r32 = gln_chain(x, torch.float32)
    cpu = gln_ratio(x, r32 if split else r32.to(x.dt), x.ref, x.E)
    assert cpu <= 1.0, f"{what}: the float32 restatement leaves the bound (ratio {cpu:.3f}): the bound is wrong, not the kernel"
    if family == "eps":
        off = ((gln_chain(x, torch.float64, 1e-5) - x.ref).abs() / x.E)[GLN_ZERO_ROWS(M), 64:128].amax(1)
        print(f"{what}: reference with eps 1e-5 on the zero rows of group 1: |diff| / bound min {off.min().item():.1f}")
        assert bool((off > 1.0).all())
    return x, what, cpu


GLN_CASES = ([("uniform", M, 256, K) for K in (32, 64, 96, 256) for M in (256, 768, 2304)] + [("uniform", 768, 512, 256)] +
             [(f, 768, 256, K) for f in ("eps", "bigmean") for K in (96, 256)])


@pytest.mark.parametrize("name,split", MODES)
@pytest.mark.parametrize("family,M,N,K", GLN_CASES)
def test_gemm_gln(lib, family, M, N, K, name, split):
    """K / 32 = 1, 2, 3, 8 k tiles (x 3 split) against the three-stage ring; M / 256 = 1, 3, 9 m tiles = a partial group, and a full
    group of 8 plus a group of one; 2, 6, 18 (N = 512: 12) blocks, no multiple of 8."""
    x, what, cpu = gln_expected(family, M, N, K, name, split)
    rc, out = launch_gln(lib, x)
    assert rc == 0
    got = out.read(what)
    worst = gln_ratio(x, got, x.ref, x.E)
    print(f"{what}: worst {'|err|' if split else 'excess over the ET rounding'} / bound {worst:.3f} (float32 on the CPU {cpu:.3f})")
    assert worst <= 1.0
    rc, again = launch_gln(lib, x)
    assert rc == 0 and torch.equal(again.bits(), out.bits()), "a second launch differs"
    if M == 2304:                                      # a row's bits do not depend on M: m tile 5 of 9 launched alone
        rc, alone = launch_gln(lib, x, row0=1280, M=256)
        assert rc == 0
        alone.read(what + " rows 1280 .. 1535 alone")
        assert torch.equal(alone.bits(), out.bits()[1280:1536]), "rows 1280 .. 1535 differ between M = 2304 and M = 256"


# ------------------------------------------------------------------------------------------------------------------
# 3. samrs_k_upscale2_masks, and the two-kernel routes end to end
# ------------------------------------------------------------------------------------------------------------------
def u2_expected(u1_64, x_dt, split, w2, b2, hyper_sel, n, grid):
    """u1_64: the exact values of what the kernel reads.  No ET rounding happens inside: un-split E_op = 0, split the in-register
    split of the fp32 u1"""
    Eop = u2_of(x_dt, True) * u1_64.abs() + TAU_ET[x_dt] if split else torch.zeros_like(u1_64)
    g2, Eg2, _ = stage2_bound(u1_64, Eop, w2.v, b2.double(), x_dt, split)
    return mask_bound(g2, Eg2, hyper_sel.double(), n, grid)


@functools.lru_cache(maxsize=2)
def u2_x(n, grid, name, split):
    prec, dt = DT[name]
    g = gen(500 + 10 * grid + n)
    rows = n * grid * grid * 4
    u1 = torch.randn(rows, 64, generator=g)
    if not split:
        u1, u1b = et_bits(u1, dt)
    w2 = operand(torch.randn(128, 64, generator=g) / 8, dt, split)
    b2 = 0.3 * torch.randn(128, generator=g)
    hyper = torch.randn(n, 4, 32, generator=g)
    o = lambda t: None if t is None else dev(t)
    return NS(n=n, grid=grid, prec=prec, dt=dt, split=split, u1=u1, w2=w2, b2=b2, hyper=hyper,
              d=NS(u1=dev(u1 if split else u1b), w=dev(w2.hi), w_lo=o(w2.lo), b2=dev(b2), hyper=dev(hyper)))


def u2_case(n, grid, name, split, n_sel, sel0):
    x = u2_x(n, grid, name, split)
    sel = x.hyper[:, sel0:sel0 + n_sel]
    ref, E = u2_expected(x.u1.double(), x.dt, split, x.w2, x.b2, sel, n, grid)
    ref32 = masks(F.gelu(x.u1 @ x.w2.v.float().t() + x.b2), sel, n, grid)
    cpu = ratio(ref32, ref, E)
    what = f"upscale2_masks n={n} grid={grid} {name} split={split} n_sel={n_sel} sel0={sel0}"
    assert cpu <= 1.0, f"{what}: the float32 restatement leaves the bound (ratio {cpu:.3f}): the bound is wrong, not the kernel"
    return x, what, ref, E, cpu


def launch_u2(lib, prec, u1_ptr, d, n, grid, n_sel, sel0):
    out = Guarded((n, n_sel, 4 * grid, 4 * grid), torch.float32)
    rc = lib.samrs_k_upscale2_masks(prec, u1_ptr, ptr(d.w), ptr(d.w_lo), ptr(d.b2), ptr(d.hyper), out.ptr, n, grid, 4, sel0, n_sel, stream())
    return rc, out


@pytest.mark.parametrize("n_sel,sel0", SELS)
@pytest.mark.parametrize("name,split", MODES)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("grid", [16, 32, 64])
def test_upscale2_masks(lib, grid, n, name, split, n_sel, sel0):
    x, what, ref, E, cpu = u2_case(n, grid, name, split, n_sel, sel0)
    rc, out = launch_u2(lib, x.prec, ptr(x.d.u1), x.d, n, grid, n_sel, sel0)
    assert rc == 0
    worst = ratio(out.read(what), ref, E)
    print(f"{what}: worst |err| / bound {worst:.3f} (float32 on the CPU {cpu:.3f})")
    assert worst <= 1.0


@pytest.mark.parametrize("name,split", MODES)
def test_routes_gln_then_upscale2(lib, name, split):
    """Routes GLN / GLN_SPLIT of engine_decode.hip end to end: the U1 that samrs_k_gemm_gln wrote goes into samrs_k_upscale2_masks and
    into the fp64 reference of stage 2 -- no rounding-flip allowance.  The distance to the fused kernel on the same inputs is
    recorded, not asserted (bit identity of the routes is claimed nowhere)."""
    n, grid, n_sel, sel0 = 3, 16, 3, 1
    x = fused_x("uniform", n, grid, name, split)
    d = upload(x)
    u1 = Guarded((n * x.tokens, 256), torch.float32 if split else x.dt)
    assert lib.samrs_k_gemm_gln(x.prec, ptr(d.keys), ptr(d.w1), u1.ptr, ptr(d.b1), ptr(d.ln), n * x.tokens, 256, 256, ptr(d.keys_lo),
                                ptr(d.w1_lo), stream()) == 0
    u1v = u1.read(f"route U1 {name} split={split}").double().reshape(-1, 64)
    dd = NS(w=d.w2, w_lo=d.w2_lo, b2=d.b2, hyper=d.hyper)
    rc, out = launch_u2(lib, x.prec, u1.ptr, dd, n, grid, n_sel, sel0)
    assert rc == 0
    ref, E = u2_expected(u1v, x.dt, split, x.w2, x.b2, x.hyper[:, sel0:sel0 + n_sel], n, grid)
    got = out.read(f"route low {name} split={split}")
    worst = ratio(got, ref, E)
    rc, fused = launch_fused(lib, x, n_sel, sel0)
    assert rc == 0
    f = fused.read("fused low")
    r = fused_ref("uniform", n, grid, name, split)
    _, Ef = mask_bound(r.g2, r.Eg2, x.hyper[:, sel0:sel0 + n_sel].double(), n, grid)
    print(f"route {'GLN_SPLIT' if split else 'GLN'} {name}: worst |err| / bound {worst:.3f}; against the fused kernel: max |diff| "
          f"{(got - f).abs().max().item():.2e}, rel L2 {rel_l2(got, f):.2e}, worst |diff| / the fused bound {ratio(got, f.double(), Ef):.3f}, "
          f"{int((got != f).sum())} of {got.numel()} elements differ")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------------
# 4. what the hooks refuse, with nothing launched
# ------------------------------------------------------------------------------------------------------------------
def refused(call, args, changes, outs):
    """every entry of `changes` ({position: value}) applied to the valid argument list must be refused with the outputs untouched"""
    for ch in changes:
        a = list(args)
        for k, v in ch.items():
            a[k] = v
        rc = call(*a)
        assert rc in BAD, f"{ch}: returned {rc}"
        assert all(o.untouched() for o in outs), f"{ch}: refused, but the output was written"


def test_upscaler_fused_refusals(lib):
    x = fused_x("uniform", 1, 16, "f16", True)
    d = upload(x)
    out = Guarded((2, 3, 64, 64), torch.float32)
    args = [x.prec, ptr(d.keys), ptr(d.keys_lo), ptr(d.w1), ptr(d.w1_lo), ptr(d.b1), ptr(d.ln), ptr(d.w2), ptr(d.w2_lo), ptr(d.b2),
            ptr(d.hyper), out.ptr, 1, 16, 4, 1, 3, stream()]
    changes = [{0: 2}, {0: -1}] + [{i: None} for i in (1, 3, 5, 6, 7, 9, 10, 11)] + [{i: args[i] + 8} for i in range(1, 12)] + \
              [{11: out.ptr + 4}, {12: 0}, {12: -1}, {13: 0}, {13: 8}, {13: 24}, {13: -16}, {14: 0}, {15: -1}, {15: 2}, {15: 4, 16: 1},
               {14: 3, 15: 1}, {16: 2}, {16: 0}, {16: 4, 15: 0}, {2: None}, {4: None}, {8: None}, {2: None, 4: None}, {4: None, 8: None}]
    refused(lib.samrs_k_upscaler_fused, args, changes, [out])
    plain = list(args)
    plain[2] = plain[4] = plain[8] = None
    refused(lib.samrs_k_upscaler_fused, plain, [{15: 2}, {0: 7}, {13: 8}], [out])
    args[15], args[16] = 3, 1                                                     # the last mask token is still served
    assert lib.samrs_k_upscaler_fused(*args) == 0
    torch.cuda.synchronize()


def test_upscale2_masks_refusals(lib):
    x = u2_x(1, 16, "f16", True)
    out = Guarded((2, 3, 64, 64), torch.float32)
    args = [x.prec, ptr(x.d.u1), ptr(x.d.w), ptr(x.d.w_lo), ptr(x.d.b2), ptr(x.d.hyper), out.ptr, 1, 16, 4, 1, 3, stream()]
    changes = [{0: 2}, {0: -1}] + [{i: None} for i in (1, 2, 4, 5, 6)] + [{i: args[i] + 8} for i in range(1, 7)] + \
              [{6: out.ptr + 4}, {7: 0}, {7: -1}, {8: 0}, {8: 8}, {8: 24}, {9: 0}, {10: -1}, {10: 2}, {10: 4, 11: 1}, {9: 3}, {11: 2}, {11: 0}]
    refused(lib.samrs_k_upscale2_masks, args, changes, [out])


def test_gemm_gln_refusals(lib):
    x = gln_x("uniform", 256, 256, 64, "f16", True)
    out = Guarded((512, 256), torch.float32)
    args = [x.prec, ptr(x.d.A), ptr(x.d.B), out.ptr, ptr(x.d.bias), ptr(x.d.gb), 256, 256, 64, ptr(x.d.A_lo), ptr(x.d.B_lo), stream()]
    changes = [{0: 2}, {0: -1}] + [{i: None} for i in (1, 2, 3, 4, 5)] + [{i: args[i] + 8} for i in (1, 2, 3, 4, 5, 9, 10)] + \
              [{6: 0}, {6: 128}, {6: 384}, {6: -256}, {7: 0}, {7: 64}, {7: 192}, {8: 0}, {8: 16}, {8: 48}, {8: -32}, {9: None}, {10: None}]
    refused(lib.samrs_k_gemm_gln, args, changes, [out])

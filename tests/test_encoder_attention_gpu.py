"""GPU: window_attention_kernel and global_attention_kernel (samrs_amd/csrc/encoder_kernels.hip) alone, per element, against a
float64 CPU statement of image_encoder.py attention with decomposed rel-pos on the same already-rounded operands, at the shapes
the engine runs them at: the persistent walk of the windowed kernel (more items than blocks), the XCD-swizzled block mapping of the
global kernel (images x heads a multiple of 8), several images, out_lo and its per-head mask.

Conventions (those of tests/test_decoder_kernels_gpu.py, whose helpers are imported)
  * qkv, the qkv bias and both rel-pos tables are rounded to the element type on the host; the reference is fp64.
  * Every output (out and out_lo) is [guard | window | guard], pre-filled with the NaN pattern of its type; afterwards every window
    element is finite and both guards are bit-for-bit untouched (`Guarded`).
  * The scale names of the input families refer to q, k, v AFTER the bias (the kernels read the GEMM's output); the k / v of a
    window's padding positions are the bias alone, as in the kernel.

The per-element bound.  Per query, with fp64 scores s_j: p_j = exp(s_j - max s), L = sum_j p_j, ref_d = sum_j p_j v_jd / L, and with
u = 2^-11 (f16) | 2^-8 (bf16), tau = 2^-25 (f16) | 0 (bf16)

    bound_d = ( sum_j max(u p_j, tau) |v_jd| ) / L  +  2 u |ref_d|  +  tau

 -- the probabilities rounded to the element type in front of the PV MFMA (f16: with its subnormal floor), the normaliser (the
ones-row sum of the ROUNDED probabilities at head_dim 80, an fp32 sum at 64), the final rounding of the output.  Every case keeps
|s| <= 200 (asserted), so that what is left of fp32 (score accumulation, exp2) stays a few percent of u.  Asserted: max over every
checked element of |got - ref| / bound <= 1.

Input families (seeded; `make_inputs`)
  uniform     N(0, 1) q / k / v, 0.3 N(0, 1) rel-pos tables, 0.5 N(0, 1) bias
  peaked      uniform, and per (window | image) one key of the LAST key tile that holds a real key scaled x 6 and one of the first
              tile x 4: the running maximum moves late, O and the row sum are rescaled
  peaked_pad  (windowed) uniform with the k bias of head 1 x 6: the padding keys of the edge and corner windows dominate
  negative    per head q = +1.5 sigma (1 + 0.1 U), k = -1.5 sigma (1 + 0.1 U) (the k bias too), sigma a +-1 pattern: every real score
              is about -20 or lower; an unmasked zero key (score 0) would take the whole row
  bigv        uniform with v + 8 (the v bias too): a normaliser error shows
  tie4        BIT-EXACT.  Tables and bias zero; two orthogonal +-1 patterns P1, P2; every query 2 P1 or 2 P2; per (window | image,
              head) four real keys hold 8 P1 and four others 8 P2, each group with a key in the first key tile and one in the last
              tile that holds a real key (the bottom windows' last tiles are all padding); every other key zero; v = multiples of
              2^-7 in [-8, 8].  The winners lead by 16 sqrt(head_dim) >= 128: every other probability is 0 in fp32, the four tie at
              exactly 1, the normaliser is exactly 4, every sum is exact (four multiples of 2^-7 of at most 8: 12 bits):
              out == ET(mean of the four v rows) and out_lo == ET(mean - out), bit for bit.  (On a 2^-6 grid the mean, a multiple
              of 2^-8 of at most 8, has 11 significant bits and is an f16 value: out_lo would be zero everywhere in f16.  On the
              2^-7 grid it is non-zero in 3.7 % of the f16 elements and 55 % of the bf16 ones; asserted to be non-trivial.)

Measured on the kernels as they stand (MI355X, 256 CUs; worst |got - ref| / bound of each group, the bound being 1):

  kernel    group                                                          f16     bf16
  --------  -------------------------------------------------------------  ------  ------
  windowed  persistent walk, 864 items (8 x 9 x 12 | 6 x 9 x 16), uniform   0.698   0.655
  windowed  grid 37, 2 images, 3 heads: peaked                             0.662   0.603
                                        peaked_pad                         0.665   0.603
                                        negative                           0.686   0.591
                                        bigv                               0.425   0.431
  windowed  grid 20, uniform                                               0.575   0.655
  windowed  out_lo call, grid 64, uniform                                  0.622   0.586
            worst |out_lo| / (u |out| + 2^-24 in f16), bound 1             0.997   1.000
  windowed  lo_heads, 5 heads, uniform                                     0.686   0.574
  global    uniform, the four (images, heads, head_dim)                    0.498   0.532
  global    peaked                                                         0.484   0.472
  global    negative                                                       0.466   0.550
  global    out_lo call, (2, 4, 80), uniform                               0.450   0.532
            worst |out_lo| / (u |out| + 2^-24 in f16), bound 1             0.999   1.000
  both      tie4: elements of out / out_lo that differ from the exact      0 / 0   0 / 0
            value (every window, 864 items; global (2, 4, 80), (2, 3, 64))

No case missed its bound and no kernel was changed.  (The fp64 reference merely rounded to the element type sits at 0.33.)

What eight one-line mutations of encoder_kernels.hip do (each built in a scratch copy and run once against this file and the four
existing kernel-level attention tests: test_window_attention, test_global_attention, test_global_attention_online_softmax_rescale of
tests/test_kernels_gpu.py and tests/test_window_dense_gpu.py; values only, every address in range; none is committed).  "every
bounded windowed case" = the 4 uniform walks, 16 families, 4 grid-20, 2 out_lo, 4 lo_heads cases of this file (30).
  1 windowed, BW[r] of the four zero keys of a tile -INFINITY -> 0      every bounded windowed case; existing: test_window_attention
                                                                        (4), the 16 dense-strip cases.  tie4 passes (p = 0 either way)
  2 windowed, the O[dt][r] *= alpha loop of the in-loop rescale dropped  the same 30 + 20
  3 windowed, `t < NGRP && has_next` -> `t < NGRP - 1`: the last V slot  the 8 persistent-walk cases only (uniform: ratio 1.6e4 .. 4.5e5;
    of the NEXT item stays stale                                        tie4: a quarter of the elements).  NO existing test
  4 windowed, padding-key bias Bia + n_head * HD -> Bia                 the same 30 + 20 as 1
  5 windowed, lo_heads ignored                                          the 4 lo_heads cases only.  NO existing test
  6 global, xcd = L % 8 -> L % 4                                        every swizzled case of this file (14: half of the rows are
                                                                        never written, the canary shows it); (2, 3, 64) is unswizzled
                                                                        and passes.  NO existing test
  7 global, vth = vt + P ... -> (P % heads)                             every case with two or more images (20: all pairs of image 1,
                                                                        ratio 6e2 .. 2e4; tie4 half of the elements); (1, 8, 64)
                                                                        passes.  NO existing test
  8 windowed store, O[DT - 1][0] and O[DT - 1][1] exchanged             all 34 windowed cases that check values, tie4 included;
                                                                        existing: the same 20
"""
import functools
import math
import types

import pytest
import torch

from test_decoder_kernels_gpu import NAN_ET, PRECS, Guarded, dev, et_bits, gen, round_et64, stream

pytestmark = pytest.mark.gpu

WIN = 14
U_ET = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
TAU_ET = {torch.float16: 2.0 ** -25, torch.bfloat16: 0.0}
S_LIMIT = 200.0


@pytest.fixture(scope="module")
def lib():
    from samrs_amd import engine
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return engine.load_library()


# ------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------
def regions(kind, grid):
    """the key sets of one image as (y0, x0, real rows, real columns), and the window rows one key tile holds"""
    if kind == "glb":
        return [(0, 0, grid, grid)], 1
    nw = -(-grid // WIN)
    return [(wy * WIN, wx * WIN, min(WIN, grid - wy * WIN), min(WIN, grid - wx * WIN)) for wy in range(nw) for wx in range(nw)], 2


def tile_positions(region, tile_rows):
    """(positions of the first key tile, of the last key tile that holds a real key, of the rest) as [n, 2] (y, x) of real keys"""
    y0, x0, rv, cv = region
    assert rv > tile_rows, "the first and the last real key tile must differ"
    t_last = (rv - 1) // tile_rows
    ys, xs = torch.meshgrid(torch.arange(rv), torch.arange(cv), indexing="ij")
    pos = torch.stack([ys.reshape(-1) + y0, xs.reshape(-1) + x0], 1)
    tile = ys.reshape(-1) // tile_rows
    return pos[tile == 0], pos[tile == t_last], pos[(tile != 0) & (tile != t_last)]


def pick(pos, n, g):
    return pos[torch.randperm(pos.shape[0], generator=g)[:n]]


def finish(kind, dt, x, bias, rel_h, rel_w, **extra):
    n_img, grid, _, _, heads, hd = x.shape
    qkv, bits = et_bits(x.reshape(n_img, grid, grid, 3 * heads * hd), dt)
    return types.SimpleNamespace(kind=kind, dt=dt, n_img=n_img, grid=grid, heads=heads, hd=hd, qkv=qkv, bits=bits,
                                 bias=et_bits(bias.reshape(-1), dt)[0], rel_h=et_bits(rel_h, dt)[0], rel_w=et_bits(rel_w, dt)[0], **extra)


def make_inputs(kind, family, dt, n_img, grid, heads, hd, seed):
    """kind "win" | "glb".  -> qkv [n_img, grid, grid, 3 D] (rounded fp32 values + bits), bias [3 D] (zero for "glb": the global
    kernel has no padding keys), rel_h / rel_w [2 S - 1, hd]"""
    if family == "tie4":
        return make_tie4(kind, dt, n_img, grid, heads, hd, seed)
    g = gen(seed)
    S = WIN if kind == "win" else grid
    x = torch.randn(n_img, grid, grid, 3, heads, hd, generator=g)
    bias = 0.5 * torch.randn(3, heads, hd, generator=g)
    rel_h = 0.3 * torch.randn(2 * S - 1, hd, generator=g)
    rel_w = 0.3 * torch.randn(2 * S - 1, hd, generator=g)
    if family == "peaked":
        regs, tr = regions(kind, grid)
        for im in range(n_img):
            for reg in regs:
                first, last, _ = tile_positions(reg, tr)
                (y1, x1), (y6, x6) = pick(first, 1, g)[0].tolist(), pick(last, 1, g)[0].tolist()
                x[im, y1, x1, 1] *= 4.0
                x[im, y6, x6, 1] *= 6.0
    elif family == "peaked_pad":
        assert kind == "win" and heads > 1
        bias[1, 1] *= 6.0
    elif family == "negative":
        sigma = torch.where(torch.rand(heads, hd, generator=g) < 0.5, -1.0, 1.0)
        x[:, :, :, 0] = 1.5 * sigma * (1.0 + 0.1 * torch.rand(n_img, grid, grid, heads, hd, generator=g))
        x[:, :, :, 1] = -1.5 * sigma * (1.0 + 0.1 * torch.rand(n_img, grid, grid, heads, hd, generator=g))
        bias[1] = -1.5 * sigma * (1.0 + 0.1 * torch.rand(heads, hd, generator=g))
    elif family == "bigv":
        x[:, :, :, 2] += 8.0
        bias[2] += 8.0
    else:
        assert family == "uniform", family
    if kind == "glb":
        bias = torch.zeros_like(bias)
    return finish(kind, dt, x, bias, rel_h, rel_w)


def make_tie4(kind, dt, n_img, grid, heads, hd, seed):
    """-> the inputs, and `mean` [n_img, grid, grid, D] fp64: the exact mean of the four v rows of each query's winning group"""
    g = gen(seed)
    S = WIN if kind == "win" else grid
    p1 = torch.where(torch.rand(hd, generator=g) < 0.5, -1.0, 1.0)
    p2 = p1 * torch.tensor([1.0, -1.0]).repeat(hd // 2)
    assert float(p1 @ p2) == 0.0 and 16.0 * math.sqrt(hd) >= 128.0
    choice = torch.randint(0, 2, (n_img, grid, grid, heads), generator=g)
    x = torch.zeros(n_img, grid, grid, 3, heads, hd)
    x[:, :, :, 0] = torch.where(choice[..., None] == 0, 2.0 * p1, 2.0 * p2)
    v, _ = et_bits(torch.randint(-1024, 1025, (n_img, grid, grid, heads, hd), generator=g).float() / 128.0, dt)
    x[:, :, :, 2] = v                                        # still multiples of 2^-7 in [-8, 8] after the rounding
    mean = torch.zeros(n_img, grid, grid, heads, hd, dtype=torch.float64)
    regs, tr = regions(kind, grid)
    for im in range(n_img):
        for (y0, x0, rv, cv) in regs:
            first, last, rest = tile_positions((y0, x0, rv, cv), tr)
            for h in range(heads):
                f, l, r = pick(first, 2, g), pick(last, 2, g), pick(rest, 4, g)
                grp = [torch.cat([f[:1], l[:1], r[:2]]), torch.cat([f[1:], l[1:], r[2:]])]
                m = []
                for pos, pat in zip(grp, (p1, p2)):
                    x[im, pos[:, 0], pos[:, 1], 1, h] = 8.0 * pat
                    m.append(v[im, pos[:, 0], pos[:, 1], h].double().sum(0) / 4.0)
                c = choice[im, y0:y0 + rv, x0:x0 + cv, h]
                mean[im, y0:y0 + rv, x0:x0 + cv, h] = torch.where(c[..., None] == 0, m[0], m[1])
    zeros = torch.zeros(2 * S - 1, hd)
    return finish(kind, dt, x, torch.zeros(3, heads, hd), zeros, zeros, mean=mean.reshape(n_img, grid, grid, heads * hd))


# ------------------------------------------------------------------------------------------------------------------
# the fp64 reference and its bound
# ------------------------------------------------------------------------------------------------------------------
def ref_and_bound(q, k, v, rel_h, rel_w, S, qh, qw, dt):
    """image_encoder.py:224-240,325-361 in fp64.  q [B, nq, d], k / v [B, S * S, d]; qh / qw [nq]: each query's place on the S x S
    key grid.  -> (ref, bound) [B, nq, d] fp64; asserts |s| <= S_LIMIT."""
    u, tau = U_ET[dt], TAU_ET[dt]
    B, nq, d = q.shape
    N = S * S
    rel_h, rel_w = rel_h.double(), rel_w.double()
    ar = torch.arange(S)
    ih, iw = qh[:, None] - ar[None] + (S - 1), qw[:, None] - ar[None] + (S - 1)          # [nq, S]
    ref = torch.empty(B, nq, d, dtype=torch.float64)
    bnd = torch.empty_like(ref)
    qc = max(1, min(nq, (1 << 23) // N))                     # score blocks of at most 8 M elements
    bc = max(1, (1 << 23) // (N * qc))
    smax = 0.0
    for b0 in range(0, B, bc):
        kt, vv = k[b0:b0 + bc].double().transpose(1, 2), v[b0:b0 + bc].double()
        av = vv.abs()
        for q0 in range(0, nq, qc):
            qq = q[b0:b0 + bc, q0:q0 + qc].double()
            b, n = qq.shape[:2]
            rh = (qq @ rel_h.T).gather(2, ih[q0:q0 + qc].expand(b, -1, -1))             # the UNSCALED q
            rw = (qq @ rel_w.T).gather(2, iw[q0:q0 + qc].expand(b, -1, -1))
            s = (((qq * d ** -0.5) @ kt).view(b, n, S, S) + rh[..., :, None] + rw[..., None, :]).view(b, n, N)
            smax = max(smax, s.abs().max().item())
            p = torch.exp(s - s.amax(-1, keepdim=True))
            L = p.sum(-1, keepdim=True)
            r = (p @ vv) / L
            ref[b0:b0 + bc, q0:q0 + qc] = r
            bnd[b0:b0 + bc, q0:q0 + qc] = ((u * p).clamp(min=tau) @ av) / L + 2.0 * u * r.abs() + tau
    assert smax <= S_LIMIT, f"a score of {smax:.1f}: the bound holds for |s| <= {S_LIMIT:g}"
    return ref, bnd


def window_reference(inp):
    """pad with the bias rows, partition (image_encoder.py:243-264), attend, un-partition + crop -> (ref, bound) [n_img, grid, grid, D]"""
    n_img, grid, heads, hd = inp.n_img, inp.grid, inp.heads, inp.hd
    D = heads * hd
    nw = -(-grid // WIN)
    padded = inp.bias.view(1, 1, 1, -1).expand(n_img, nw * WIN, nw * WIN, 3 * D).clone()
    padded[:, :grid, :grid] = inp.qkv
    xw = padded.view(n_img, nw, WIN, nw, WIN, 3, heads, hd).permute(5, 0, 1, 3, 6, 2, 4, 7).reshape(3, n_img * nw * nw * heads, WIN * WIN, hd)
    pos = torch.arange(WIN * WIN)
    out = []
    for t in ref_and_bound(xw[0], xw[1], xw[2], inp.rel_h, inp.rel_w, WIN, pos // WIN, pos % WIN, inp.dt):
        t = t.view(n_img, nw, nw, heads, WIN, WIN, hd).permute(0, 1, 4, 2, 5, 3, 6).reshape(n_img, nw * WIN, nw * WIN, D)
        out.append(t[:, :grid, :grid])
    return out


def global_reference(inp, seed):
    """Pair by pair.  The first and the last (image, head) pair: all 4096 rows; the others: three seeded rows of each of the 128
    32-query strips.  -> [(image, head, rows, ref, bound)]"""
    n_img, grid, heads, hd = inp.n_img, inp.grid, inp.heads, inp.hd
    N = grid * grid
    g = gen(seed)
    x = inp.qkv.view(n_img, N, 3, heads, hd)
    out = []
    for P in range(n_img * heads):
        im, h = divmod(P, heads)
        if P in (0, n_img * heads - 1):
            rows = torch.arange(N)
        else:
            rows = torch.cat([32 * s + torch.randperm(32, generator=g)[:3] for s in range(N // 32)])
        q, k, v = x[im, rows, 0, h][None], x[im, :, 1, h][None], x[im, :, 2, h][None]
        ref, bnd = ref_and_bound(q, k, v, inp.rel_h, inp.rel_w, grid, rows // grid, rows % grid, inp.dt)
        out.append((im, h, rows, ref[0], bnd[0]))
    return out


def window_case(family, dt, n_img, grid, heads, hd, seed):
    inp = make_inputs("win", family, dt, n_img, grid, heads, hd, seed)
    inp.ref, inp.bnd = (None, None) if family == "tie4" else window_reference(inp)
    return inp


def global_case(family, dt, n_img, heads, hd, seed):
    inp = make_inputs("glb", family, dt, n_img, 64, heads, hd, seed)
    inp.pairs = None if family == "tie4" else global_reference(inp, seed + 1)
    return inp


@functools.lru_cache(maxsize=2)
def global_case_2_4_80(dt):
    """uniform at (2, 4, 80), one per element type: test_global_uniform and test_global_out_lo share it"""
    return global_case("uniform", dt, 2, 4, 80, 5042)


# ------------------------------------------------------------------------------------------------------------------
# launches and checks
# ------------------------------------------------------------------------------------------------------------------
def launch(lib, prec, inp, how="plain", lo_heads=0xFFFFFFFF):
    """how: "plain" the kernel's own entry point, "mx" samrs_k_attention_mx without out_lo, "mx_lo" with it (null MX pointers),
    "lo_heads" samrs_k_window_attention_lo.  -> (out, out_lo | None) as Guarded buffers"""
    rows, D = inp.n_img * inp.grid * inp.grid, inp.heads * inp.hd
    out = Guarded((rows, D), inp.dt)
    lo = Guarded((rows, D), inp.dt) if how in ("mx_lo", "lo_heads") else None
    qd, bd, rhd, rwd = dev(inp.bits), dev(inp.bias), dev(inp.rel_h), dev(inp.rel_w)
    glb = inp.kind == "glb"
    if how == "plain" and glb:
        rc = lib.samrs_k_global_attention(prec, qd.data_ptr(), rhd.data_ptr(), rwd.data_ptr(), out.ptr, inp.n_img, inp.grid, inp.heads, inp.hd, stream())
    elif how == "plain":
        rc = lib.samrs_k_window_attention(prec, qd.data_ptr(), bd.data_ptr(), rhd.data_ptr(), rwd.data_ptr(), out.ptr, inp.n_img, inp.grid, WIN,
                                          inp.heads, inp.hd, stream())
    elif how in ("mx", "mx_lo"):
        rc = lib.samrs_k_attention_mx(prec, int(glb), qd.data_ptr(), bd.data_ptr(), rhd.data_ptr(), rwd.data_ptr(), out.ptr, lo.ptr if lo else None,
                                      inp.n_img, inp.grid, inp.heads, inp.hd, None, None, None, None, stream())
    else:
        assert how == "lo_heads" and not glb
        rc = lib.samrs_k_window_attention_lo(prec, qd.data_ptr(), bd.data_ptr(), rhd.data_ptr(), rwd.data_ptr(), out.ptr, lo.ptr, inp.n_img,
                                             inp.grid, inp.heads, inp.hd, lo_heads, stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out, lo


def read4(buf, what, inp, finite=True):
    return buf.read(what, finite=finite).view(inp.n_img, inp.grid, inp.grid, inp.heads * inp.hd)


def check_bound(what, got, ref, bnd):
    ratio = (got.double() - ref).abs() / bnd.clamp(min=1e-300)
    worst = ratio.max().item()
    print(f"ENCATT {what}: worst |got - ref| / bound {worst:.3f} over {ratio.numel()} elements")
    at = [int(i) for i in torch.unravel_index(ratio.argmax(), ratio.shape)]
    assert worst <= 1.0, f"{what}: |got - ref| / bound = {worst:.3f} at {at} ({int((ratio > 1).sum())} elements beyond the bound)"
    return worst


def check_global(what, got, inp):
    N = inp.grid * inp.grid
    g = got.view(inp.n_img, N, inp.heads, inp.hd)
    worst, bad, n = 0.0, [], 0
    for im, h, rows, ref, bnd in inp.pairs:
        ratio = (g[im, rows, h].double() - ref).abs() / bnd.clamp(min=1e-300)
        w = ratio.max().item()
        worst, n = max(worst, w), n + ratio.numel()
        if w > 1.0:
            bad.append((im, h, round(w, 3), int((ratio > 1).sum())))
    print(f"ENCATT {what}: worst |got - ref| / bound {worst:.3f} over {n} elements")
    assert not bad, f"{what}: (image, head, worst ratio, elements beyond the bound) {bad[:8]}"


def bits_of(x64, dt):
    """fp64 values that ARE element-type values -> their bit patterns"""
    return x64.float().to(dt).view(torch.int16)


def check_tie4(lib, prec, inp, what):
    """out == ET(mean) through the kernel's own entry point; out the same and out_lo == ET(mean - out) through the out_lo call"""
    exp = round_et64(inp.mean, inp.dt)
    exp_lo = round_et64(inp.mean - exp, inp.dt)
    assert bool((exp_lo != 0).any()), "the remainder must not be trivially zero"
    out, _ = launch(lib, prec, inp)
    got = read4(out, f"{what} out", inp)
    d = int((got.view(torch.int16) != bits_of(exp, inp.dt)).sum())
    print(f"ENCATT {what} tie4: out elements differing from ET(mean) {d} of {got.numel()}")
    assert d == 0, f"{what}: {d} elements of out differ from ET(mean of the four winning v rows)"
    out2, lo = launch(lib, prec, inp, "mx_lo")
    assert torch.equal(out2.bits(), out.bits()), f"{what}: out differs between the call with out_lo and the one without"
    out2.read(f"{what} out (out_lo call)")
    got_lo = read4(lo, f"{what} out_lo", inp)
    d = int((got_lo.view(torch.int16) != bits_of(exp_lo, inp.dt)).sum())
    print(f"ENCATT {what} tie4: out_lo elements differing from ET(mean - out) {d} of {got_lo.numel()}")
    assert d == 0, f"{what}: {d} elements of out_lo differ from ET(mean - out)"


def check_out_lo(lib, prec, inp, what):
    """the out_lo call: out bit-identical to the plain call and within the bound; |out_lo| <= u |out| (+ 2^-24 in f16: the subnormal step)"""
    out, _ = launch(lib, prec, inp, "mx")
    out2, lo = launch(lib, prec, inp, "mx_lo")
    got, got2 = read4(out, f"{what} out", inp), read4(out2, f"{what} out (out_lo call)", inp)
    assert torch.equal(got.view(torch.int16), got2.view(torch.int16)), f"{what}: out differs between the call with out_lo and the one without"
    got_lo = read4(lo, f"{what} out_lo", inp).double()
    lim = U_ET[inp.dt] * got.double().abs() + (2.0 ** -24 if inp.dt == torch.float16 else 0.0)
    worst = (got_lo.abs() / lim.clamp(min=1e-300)).max().item()
    print(f"ENCATT {what}: worst |out_lo| / (u |out|) {worst:.3f}, out_lo non-zero in {float((got_lo != 0).double().mean()):.3f} of the elements")
    assert bool((got_lo.abs() <= lim).all()), f"{what}: |out_lo| / (u |out|) = {worst:.3f}"
    assert bool((got_lo != 0).any())
    return got


# ------------------------------------------------------------------------------------------------------------------
# windowed kernel
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,prec,dt,ulp", PRECS)
@pytest.mark.parametrize("family", ["uniform", "tie4"])
@pytest.mark.parametrize("hd,heads", [(64, 12), (80, 16)])
def test_window_persistent_walk(lib, name, prec, dt, ulp, family, hd, heads):
    """Grid 37: 9 windows per image, 4 interior (7 strips), 4 edge (4) and 1 corner (3).  Between 3 and 4 items per block: every
    block walks 3 or 4 items of changing numbering with the next item's loads in flight, and the last walk is partial."""
    cu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    per_image = 9 * heads
    n_img = 3 * cu // per_image + 1
    n_items = n_img * per_image
    assert 3 * cu < n_items < 4 * cu, f"{n_items} items on {cu} CUs: the walk must take more than 3 and fewer than 4 items per block"
    inp = window_case(family, dt, n_img, 37, heads, hd, 4000 + hd)
    what = f"window walk {name} hd={hd} heads={heads} images={n_img} items={n_items} {family}"
    if family == "tie4":
        check_tie4(lib, prec, inp, what)
    else:
        out, _ = launch(lib, prec, inp)
        check_bound(what, read4(out, what, inp), inp.ref, inp.bnd)


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS)
@pytest.mark.parametrize("family", ["peaked", "peaked_pad", "negative", "bigv"])
@pytest.mark.parametrize("hd,heads", [(64, 3), (80, 3)])
def test_window_input_families(lib, name, prec, dt, ulp, family, hd, heads):
    inp = window_case(family, dt, 2, 37, heads, hd, 4100 + hd)
    what = f"window family {name} hd={hd} {family}"
    out, _ = launch(lib, prec, inp)
    check_bound(what, read4(out, what, inp), inp.ref, inp.bnd)


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS)
@pytest.mark.parametrize("hd,heads", [(64, 3), (80, 3)])
def test_window_grid20(lib, name, prec, dt, ulp, hd, heads):
    """edge windows of 6 x 14 real queries (3 strips), a 6 x 6 corner (2): a second row length of the dense numbering"""
    inp = window_case("uniform", dt, 2, 20, heads, hd, 4200 + hd)
    what = f"window grid20 {name} hd={hd} uniform"
    out, _ = launch(lib, prec, inp)
    check_bound(what, read4(out, what, inp), inp.ref, inp.bnd)


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS)
def test_window_out_lo(lib, name, prec, dt, ulp):
    inp = window_case("uniform", dt, 2, 64, 2, 80, 4300)
    what = f"window out_lo {name} hd=80 uniform"
    check_bound(what, check_out_lo(lib, prec, inp, what), inp.ref, inp.bnd)


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS)
@pytest.mark.parametrize("hd", [64, 80])
def test_window_lo_heads(lib, name, prec, dt, ulp, hd):
    """lo_heads, the per-head mask of out_lo: a masked-off head's rows keep the canary, an enabled head's rows equal the all-ones run,
    out is the same whatever the mask"""
    heads, mask = 5, 0b01010
    inp = window_case("uniform", dt, 2, 37, heads, hd, 4400 + hd)
    what = f"window lo_heads {name} hd={hd}"
    runs = {m: launch(lib, prec, inp, "lo_heads", m) for m in (0xFFFFFFFF, mask, 0)}
    outs = {m: read4(o, f"{what} out, mask {m:#x}", inp).view(torch.int16) for m, (o, _) in runs.items()}
    los = {m: read4(l, f"{what} out_lo, mask {m:#x}", inp, finite=(m == 0xFFFFFFFF)).view(torch.int16).reshape(-1, heads, hd) for m, (_, l) in runs.items()}
    plain, _ = launch(lib, prec, inp)
    assert torch.equal(outs[0xFFFFFFFF], read4(plain, what, inp).view(torch.int16)), "out differs from the call without out_lo"
    assert torch.equal(outs[mask], outs[0xFFFFFFFF]) and torch.equal(outs[0], outs[0xFFFFFFFF]), "out depends on lo_heads"
    assert runs[0][1].untouched(), "lo_heads = 0 wrote to out_lo"
    assert bool((los[0xFFFFFFFF] != 0).any())
    canary = NAN_ET[dt]
    for h in range(heads):
        if (mask >> h) & 1:
            assert torch.equal(los[mask][:, h], los[0xFFFFFFFF][:, h]), f"head {h} is enabled: its out_lo rows differ from the all-ones run"
        else:
            assert bool((los[mask][:, h] == canary).all()), f"head {h} is masked off: its out_lo rows were written"
    check_bound(what, outs[mask].view(dt), inp.ref, inp.bnd)


# ------------------------------------------------------------------------------------------------------------------
# global kernel (grid 64)
# ------------------------------------------------------------------------------------------------------------------
# (images, heads, head_dim): images x heads % 8 == 0 takes the XCD-swizzled block mapping
GLB_SWIZZLED_1 = (1, 8, 64)
GLB_SWIZZLED_2 = (2, 4, 80)                     # ... across two images
GLB_PLAIN_2 = (2, 3, 64)                        # unswizzled, two images
GLB_SWIZZLED_24 = (3, 8, 80)                    # 24 pairs: the pair index wraps past one round of eight


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS)
@pytest.mark.parametrize("n_img,heads,hd", [GLB_SWIZZLED_1, GLB_SWIZZLED_2, GLB_PLAIN_2, GLB_SWIZZLED_24])
def test_global_uniform(lib, name, prec, dt, ulp, n_img, heads, hd):
    inp = global_case_2_4_80(dt) if (n_img, heads, hd) == GLB_SWIZZLED_2 else global_case("uniform", dt, n_img, heads, hd, 5000 + 10 * heads + n_img)
    what = f"global uniform {name} images={n_img} heads={heads} hd={hd}"
    out, _ = launch(lib, prec, inp)
    check_global(what, read4(out, what, inp), inp)


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS)
@pytest.mark.parametrize("family", ["peaked", "negative", "tie4"])
@pytest.mark.parametrize("n_img,heads,hd", [GLB_SWIZZLED_2, GLB_PLAIN_2])
def test_global_input_families(lib, name, prec, dt, ulp, family, n_img, heads, hd):
    inp = global_case(family, dt, n_img, heads, hd, 5100 + 10 * heads + n_img)
    what = f"global family {name} images={n_img} heads={heads} hd={hd} {family}"
    if family == "tie4":
        check_tie4(lib, prec, inp, what)
    else:
        out, _ = launch(lib, prec, inp)
        check_global(what, read4(out, what, inp), inp)


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS)
def test_global_out_lo(lib, name, prec, dt, ulp):
    n_img, heads, hd = GLB_SWIZZLED_2
    inp = global_case_2_4_80(dt)                                                           # the case of test_global_uniform
    what = f"global out_lo {name} images={n_img} heads={heads} hd={hd} uniform"
    check_global(what, check_out_lo(lib, prec, inp, what), inp)

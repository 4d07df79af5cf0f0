"""GPU: every prompt-encoder / mask-decoder HIP kernel alone (the decoder half of tests/test_kernels_gpu.py), through the
kernel-level entry points of include/samrs_hip_internal.h, against a float64 CPU statement of the same operation on the
same already-rounded operands.

Conventions
  * Every output buffer is [guard | window | guard], pre-filled with a NaN pattern of its type (0x7E00 f16, 0x7FC0 bf16 --
    0x7E00 is a finite bf16 --, NaN fp32, a sentinel for int32).  After the kernel every window element must be finite and
    both guards bit-for-bit untouched (`Guarded`).
  * Bit-exact where the operation is exact (copies, fp32 adds, ET rounding, the slot table, a second run of the t2i merge).
  * sin / cos kernels: |err| <= c 2^-24 (1 + A), A = 2 pi (|vx g0| + |vy g1|) in fp64 per element, c = 12 (`PE_C`).
  * fp32 outputs with exp or cancellation: rel L2 <= max(8 x the reference's own fp32 noise, 3e-6), the noise being the same
    formula evaluated by torch in float32 on the CPU against float64 on the inputs of the case (`fp32_bound`).
  * ET outputs: what exceeds one ET ulp of the reference value, |err| - ulp |ref| clamped at 0, must meet that same fp32
    rel-L2 bound (`et_excess`).

Measured on the kernels as they stand (MI355X; the worst case of each group; "noise" = the fp32 reference against fp64).
"beyond ulp" = rel L2 of what exceeds one ET ulp (`et_excess`).

  kernel            case (worst of the group)                       measured             bound
  ----------------  ----------------------------------------------  -------------------  ----------------------------------
  prompt_tokens     points, 8 points, n = 64 (T = 14)               err / bound 0.203    1 (c = 12); copied rows bit-exact
  dense_pe          grid 64                                         err / bound 0.215    1; against the oracle 0.098 of 2 x
  mask_embed        N(0, 4) / +-1000 box / constant                 1.6e-7 / 1.9e-7 /    3.0e-6 (noise 1.5e-7 / 1.0e-7 /
                                                                    2.1e-7                8.6e-8)
  fill_slot_table   1, 64, 65, 150 runs                             0 wrong entries      exact
  make_keys         all 32 cases, |values| up to 3e38               0 mismatching bits   exact (fp32 and ET)
  token_self_attn   uniform T = 16 / ascending T = 16, n = 33 /     1.1e-7 / 3.2e-7 /    3.0e-6 (noise 9.2e-8 / 3.4e-7 /
                    dominant T = 14                                 4.3e-8                1.6e-8)
  t2i_attention     uniform 4096 keys / spiky 100 keys, slots /     1.5e-7 / 2.6e-7 /    3.0e-6 / 3.0e-6 / 5.2e-6 (noise
                    wide 1000 keys bf16                             9.0e-7                2.6e-7 / 2.4e-7 / 6.5e-7)
  i2t_attention     f16 peaked T = 9, 4096 tokens                   beyond ulp 1.9e-9    3.0e-6 (noise 1.2e-7); plain rel L2
                                                                                         2.1e-4 f16, 1.6e-3 bf16 = the rounding
  i2t_fused outF    f16: uniform / peaked / bigmean                 2.0e-6 / 5.8e-6 /    1.7e-5 / 3.5e-5 / 1.3e-4 (noise
                                                                    1.4e-5                2.1e-6 / 4.4e-6 / 1.6e-5)
                    bf16: uniform / peaked / bigmean                6.4e-6 / 1.1e-6 /    5.6e-5 / 3.0e-6 / 1.4e-4 (noise
                                                                    2.3e-5                7.0e-6 / 7.9e-8 / 1.8e-5)
                    (the noise is the fp32 reference rounding its attention output to the other ET neighbour than fp64 does)
  i2t_fused outE    bf16 bigmean 4096 tokens                        beyond ulp 3.3e-6    1.4e-4; = ET(outF), outE_lo =
                                                                                         ET(outF - outE) bit for bit
  i2t_fused split   max |err| / max(|ref|, 1e-2), un-rounded ref    f16 9.3e-5 split,    < 1e-4 / >= 1e-4
                                                                    7.2e-2 un-split
                                                                    bf16 9.4e-4 / 4.4e-1 < 2e-3 / >= 2e-3
  group_ln_gelu     N(0, 1) 16387 rows / 1000 +- 1                  beyond ulp 2.4e-10   3.0e-6 / 2.6e-4 (noise 1.1e-7 /
                                                                    / 1.8e-6              3.2e-5)
  mask_product      grid 16, n_sel 1, bf16                          1.1e-7               3.0e-6 (noise 7.4e-8)

No kernel missed a bound.  What the one-line mutations of the issue do to this file (each rebuilt in a scratch copy, in bounds):
corr = 1 in t2i_partial: 56 t2i cases fail (spiky, wide; rel L2 up to O(1)); valid forced true: only the 4 cases with 100 keys
(rel L2 2e-4 .. 4e-2), the one count whose last wave is not a multiple of 8 keys -- 1003, 4093 and 37 were added for that reason
and have not been measured on the device yet, neither against the kernel nor against the mutation; kbat = 0 with a slot table: every "slots" t2i case
(28); fs / fo swapped: 56 t2i cases; r_bstride = 0 in i2t_fused: the 12 batched / slots fused cases and the split-precision pair;
dy / dx exchanged: all 24 mask_product cases; the label == -1 branch dropped: the 24 prompt_tokens cases with points; eps dropped:
the 16 group_ln_gelu cases (NaN in the constant group).  test_decoder_alone_all_prompt_types catches 4 of the 8 (corr, fs / fo
in f16 only, r_bstride, the pad point).
"""
import ctypes
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

PRECS = [("f16", 1, torch.float16, 2.0 ** -10), ("bf16", 0, torch.bfloat16, 2.0 ** -7)]
NAN_ET = {torch.float16: 0x7E00, torch.bfloat16: 0x7FC0}
I32_SENTINEL = -195948557
TWO_PI = 2.0 * math.pi

# sin / cos bound |err| <= PE_C 2^-24 (1 + A).  On the argument a = 2 pi (vx g0 + vy g1): two products and one sum, each
# rounded to 2^-24 of at most |vx g0| + |vy g1|, the product with 2 pi (2^-24 |a|) and the fp32 constant 2 pi itself
# (0.47 2^-24 |a|) -- 3.5 2^-24 A in all, and |d sin| <= |d a|.  sinf / cosf: 2 ulp of a value <= 1 = 4 2^-24.  The add of the
# point embedding rounds once more, 2^-24 |result| with |result| <= 1 + |embedding| <= 6 here.  3.5 A + 4 + 6 <= 12 (1 + A).
PE_C = 12.0
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def lib():
    from samrs_amd import engine
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return engine.load_library()


def dev(t):
    return t.cuda().contiguous()


def stream():
    return torch.cuda.current_stream().cuda_stream


def gen(seed):
    return torch.Generator().manual_seed(seed)


def et_bits(x, dt):
    """fp32 tensor -> (rounded fp32 values, int16 bit patterns); f16 saturates at +-65504 as the kernels do"""
    if dt == torch.float16:
        x = x.clamp(-65504.0, 65504.0)
    r = x.to(dt)
    return r.to(torch.float32), r.view(torch.int16)


def round_et64(x, dt):
    """float64 -> nearest ET value (as float64), rounded ONCE: torch converts double -> half / bfloat16 through float, which
    rounds twice where the float lands exactly on an ET tie."""
    if dt == torch.float16:
        return torch.from_numpy(x.clamp(-65504.0, 65504.0).numpy().astype(np.float16).astype(np.float64))
    f = x.float()
    bits = f.view(torch.int32)
    r = f.to(dt).double()
    fix = ((bits & 0xFFFF) == 0x8000) & (f.double() != x)
    if bool(fix.any()):
        trunc = (bits & ~0xFFFF)
        away = trunc + 0x10000
        pick = torch.where(x.abs() > f.double().abs(), away, trunc).view(torch.float32).double()
        r = torch.where(fix, pick, r)
    return r


def round_et(x, dt):
    return round_et64(x, dt) if x.dtype == torch.float64 else x.to(dt).to(x.dtype)


class Guarded:
    """Device buffer [guard | window | guard] filled with the NaN pattern of `dt` (torch.float32, an ET type, or torch.int32)."""

    def __init__(self, shape, dt, rows=4):
        self.shape, self.dt = tuple(shape), dt
        self.n = math.prod(self.shape)
        self.g = -(-max(64, rows * self.shape[-1]) // 64) * 64
        if dt == torch.float32:
            store, self.fill = torch.int32, 0x7FC00000
        elif dt == torch.int32:
            store, self.fill = torch.int32, I32_SENTINEL
        else:
            store, self.fill = torch.int16, NAN_ET[dt]
        self.buf = torch.full((2 * self.g + self.n,), self.fill, dtype=store, device="cuda")

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.g * self.buf.element_size()

    def bits(self):
        """window as raw integers (CPU)"""
        torch.cuda.synchronize()
        return self.buf[self.g:self.g + self.n].cpu().view(self.shape)

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == self.fill).all())

    def read(self, what, finite=True):
        torch.cuda.synchronize()
        b = self.buf.cpu()
        front, back = b[:self.g], b[self.g + self.n:]
        assert bool((front == self.fill).all()) and bool((back == self.fill).all()), \
            f"{what}: wrote outside its window ({int((front != self.fill).sum())} elements in front, {int((back != self.fill).sum())} behind)"
        w = b[self.g:self.g + self.n].clone()
        if self.dt == torch.int32:
            return w.view(self.shape)
        v = w.view(self.dt).view(self.shape)
        if finite:
            bad = int((~torch.isfinite(v.float())).sum())
            assert bad == 0, f"{what}: {bad} of {self.n} window elements are not finite (not written, or NaN / inf computed)"
        return v


def rel_l2(a, ref):
    a, ref = a.double(), ref.double()
    return ((a - ref).norm() / ref.norm().clamp(min=1e-300)).item()


def fp32_bound(ref32, ref64):
    """(bound, noise): 8 x the rel-L2 error of the float32 evaluation of the reference formula, floor 3e-6.  8: the hardware exp2
    is 1 ulp against libm's 1/2, its pre-scaled argument carries one more rounding, the summation order differs."""
    noise = rel_l2(ref32, ref64)
    return max(8.0 * noise, 3e-6), noise


def et_excess(got, ref64, ulp):
    """rel L2 of what exceeds one ET ulp of the reference value"""
    r = ((got.double() - ref64).abs() - ulp * ref64.abs()).clamp(min=0.0)
    return (r.norm() / ref64.norm().clamp(min=1e-300)).item()


def heads_of(x, d):
    """[B, L, H * d] -> [B, H, L, d]"""
    return x.reshape(x.shape[0], x.shape[1], -1, d).transpose(1, 2)


def attention(q, k, v, d, dtype):
    """softmax(q k^T / sqrt(d)) v per head (transformer.py:218-240); q [B, Lq, C], k / v [B, Lk, C] -> [B, Lq, C]"""
    qh, kh, vh = heads_of(q.to(dtype), d), heads_of(k.to(dtype), d), heads_of(v.to(dtype), d)
    a = torch.softmax((qh @ kh.transpose(2, 3)) / math.sqrt(d), dim=-1)
    return (a @ vh).transpose(1, 2).reshape(q.shape[0], q.shape[1], -1)


# ------------------------------------------------------------------------------------------------------------------
# prompt tokens / dense PE
# ------------------------------------------------------------------------------------------------------------------
def pe64(gauss, x32, y32, size):
    """fp64 positional encoding of the fp32 coordinates (already + 0.5), and the bound's A per element: [..., 256] each.
    vx = 2 x / size - 1 is taken in fp32 as the kernel takes it (x / size is exact for a power-of-two size, 2 c - 1 rounds
    once, fused or not): vx, vy are the operands, the bound covers what follows."""
    vx = (2.0 * (x32 / size) - 1.0).double()[..., None]
    vy = (2.0 * (y32 / size) - 1.0).double()[..., None]
    g0, g1 = gauss[0].double(), gauss[1].double()
    a = TWO_PI * (vx * g0 + vy * g1)
    A = TWO_PI * ((vx * g0).abs() + (vy * g1).abs())
    return torch.cat([torch.sin(a), torch.cos(a)], -1), torch.cat([A, A], -1)


def prompt_weights(seed):
    g = gen(seed)
    return dict(gauss=torch.randn(2, 128, generator=g), point_emb=torch.randn(4, 256, generator=g).clamp(-5, 5),
                not_a_point=torch.randn(256, generator=g), iou_token=torch.randn(256, generator=g),
                mask_tokens=torch.randn(4, 256, generator=g))


@pytest.mark.parametrize("tokens2", [True, False], ids=["tokens2", "no-tokens2"])
@pytest.mark.parametrize("n", [1, 3, 64])
@pytest.mark.parametrize("kind,npts", [("box", 0), ("points", 1), ("points", 3), ("points", 8), ("points+box", 8)])
def test_prompt_tokens(lib, kind, npts, n, tokens2):
    """prompt_encoder.py:73-100 + mask_decoder.py:127-129.  Rows that are copies (output tokens, not-a-point, the pad point)
    are bit-exact, encoded rows meet the sin / cos bound."""
    w = prompt_weights(11)
    g = gen(100 * n + npts)
    has_box, has_pts = "box" in kind, "points" in kind
    T = 5 + (npts + (0 if has_box else 1) if has_pts else 0) + (2 if has_box else 0)
    edge = torch.tensor([0.0, 1023.0, -37.25, 1500.5, 512.0, 2047.0, -1024.0, 1024.0])
    boxes = coords = labels = None
    if has_box:
        boxes = torch.rand(n, 4, generator=g) * 1023
        boxes[0] = torch.tensor([0.0, 1023.0, -12.5, 1100.0])
    if has_pts:
        coords = torch.rand(n, npts, 2, generator=g) * 1023
        coords[0, :, 0] = edge[:npts]
        coords[0, :, 1] = edge.flip(0)[:npts]
        labels = torch.randint(-1, 2, (n, npts), generator=g, dtype=torch.int32)
        labels[0] = torch.tensor([1, 0, -1, 1, 0, 1, -1, 0], dtype=torch.int32)[:npts]
        if n > 1:
            labels[-1] = -1                                      # one prompt with nothing but "not a point"
    # ---- reference
    ref = torch.zeros(n, T, 256, dtype=torch.float64)
    tol = torch.zeros(n, T, 256, dtype=torch.float64)          # 0 = bit-exact
    ref[:, 0] = w["iou_token"].double()
    ref[:, 1:5] = w["mask_tokens"].double()
    j = 5
    if has_pts:
        pe, A = pe64(w["gauss"], coords[..., 0] + 0.5, coords[..., 1] + 0.5, 1024.0)
        lab = labels.long()[..., None]
        emb = torch.where(lab == 0, w["point_emb"][0].double(), torch.where(lab == 1, w["point_emb"][1].double(), torch.zeros((), dtype=torch.float64)))
        ref[:, j:j + npts] = torch.where(lab == -1, w["not_a_point"].double(), pe + emb)
        tol[:, j:j + npts] = torch.where(lab == -1, torch.zeros((), dtype=torch.float64), PE_C * U24 * (1.0 + A))
        j += npts
        if not has_box:
            ref[:, j] = w["not_a_point"].double()
            j += 1
    if has_box:
        bc = boxes.reshape(n, 2, 2)
        pe, A = pe64(w["gauss"], bc[..., 0] + 0.5, bc[..., 1] + 0.5, 1024.0)
        ref[:, j:j + 2] = pe + w["point_emb"][2:4].double()
        tol[:, j:j + 2] = PE_C * U24 * (1.0 + A)
        j += 2
    assert j == T
    # ---- kernel
    wd = {k: dev(v) for k, v in w.items()}
    bd, cd, ld_ = (None if t is None else dev(t) for t in (boxes, coords, labels))
    out, out2 = Guarded((n, T, 256), torch.float32), Guarded((n, T, 256), torch.float32)
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = lib.samrs_k_prompt_tokens(ptr(bd), ptr(cd), ptr(ld_), n, npts, 1024.0, wd["gauss"].data_ptr(), wd["point_emb"].data_ptr(),
                                   wd["not_a_point"].data_ptr(), wd["iou_token"].data_ptr(), wd["mask_tokens"].data_ptr(),
                                   out.ptr, out2.ptr if tokens2 else None, T, stream())
    assert rc == 0
    got = out.read(f"prompt_tokens {kind}")
    err = (got.double() - ref).abs()
    exact = tol == 0
    worst = (err / tol.clamp(min=1e-300))[~exact].max().item() if bool((~exact).any()) else 0.0
    print(f"prompt_tokens {kind} npts={npts} n={n} T={T}: max err {err.max().item():.2e}, worst err / bound {worst:.3f} "
          f"(c = {PE_C:g}), copied rows differing {int((err[exact] != 0).sum())}")
    assert bool((got.double()[exact] == ref[exact]).all()), "a copied row (output token / not-a-point / pad point) is not bit-exact"
    assert bool((err <= tol)[~exact].all()), f"encoded rows: worst err / bound {worst:.3f}"
    if tokens2:
        assert torch.equal(out2.bits(), out.bits()), "tokens2 is not a bit-equal copy of tokens"
        out2.read("prompt_tokens tokens2")
    else:
        assert out2.untouched()
    # a token count that does not belong to the prompt kinds is refused with nothing launched
    out3 = Guarded((n, T + 1, 256), torch.float32)
    assert lib.samrs_k_prompt_tokens(ptr(bd), ptr(cd), ptr(ld_), n, npts, 1024.0, wd["gauss"].data_ptr(), wd["point_emb"].data_ptr(),
                                     wd["not_a_point"].data_ptr(), wd["iou_token"].data_ptr(), wd["mask_tokens"].data_ptr(),
                                     out3.ptr, None, T + 1, stream()) != 0
    assert out3.untouched()


@pytest.mark.parametrize("grid", [64, 16])
def test_dense_pe(lib, grid):
    """prompt_encoder.py:62-71,199-209; also against the project's oracle on the same matrix (an fp32 evaluation with the
    same error class: twice the bound)."""
    from oracle import sam_oracle as so
    gauss = torch.randn(2, 128, generator=gen(grid))
    t = (torch.arange(grid, dtype=torch.float32) + 0.5) / grid
    yy, xx = torch.meshgrid(t, t, indexing="ij")
    ref, A = pe64(gauss, xx.reshape(-1), yy.reshape(-1), 1.0)
    out = Guarded((grid * grid, 256), torch.float32)
    gd = dev(gauss)
    assert lib.samrs_k_dense_pe(gd.data_ptr(), out.ptr, grid, stream()) == 0
    got = out.read("dense_pe").double()
    tol = PE_C * U24 * (1.0 + A)
    err = (got - ref).abs()
    orc = so.dense_pe({"prompt_encoder.pe_layer.positional_encoding_gaussian_matrix": gauss}, types.SimpleNamespace(grid=grid))
    orc = orc[0].permute(1, 2, 0).reshape(grid * grid, 256).double()
    eo = (got - orc).abs()
    print(f"dense_pe grid={grid}: max err {err.max().item():.2e}, worst err / bound {(err / tol).max().item():.3f}; "
          f"against the oracle: max {eo.max().item():.2e}, worst / (2 x bound) {(eo / (2 * tol)).max().item():.3f}")
    assert bool((err <= tol).all())
    assert bool((eo <= 2 * tol).all())


# ------------------------------------------------------------------------------------------------------------------
# mask prompt embedding
# ------------------------------------------------------------------------------------------------------------------
def ln_channels(x, w, b, eps):
    """LayerNorm2d over dim 1 of [B, C, H, W] (common.py:31-43)"""
    u = x.mean(1, keepdim=True)
    s = ((x - u) ** 2).mean(1, keepdim=True)
    return (x - u) / torch.sqrt(s + eps) * w[None, :, None, None] + b[None, :, None, None]


def mask_embed_ref(p, m, dtype):
    """prompt_encoder.py:51-59: conv 2x2/2 -> LN2d -> GELU -> conv 2x2/2 -> LN2d -> GELU -> conv 1x1; [n, tokens, 256]"""
    q = {k: v.to(dtype) for k, v in p.items()}
    y = F.conv2d(m.to(dtype)[:, None], q["w0"], q["b0"], stride=2)
    y = F.gelu(ln_channels(y, q["ln1w"], q["ln1b"], 1e-6))
    y = F.conv2d(y, q["w3"], q["b3"], stride=2)
    y = F.gelu(ln_channels(y, q["ln4w"], q["ln4b"], 1e-6))
    y = F.conv2d(y, q["w6"], q["b6"])
    return y.flatten(2).permute(0, 2, 1)


def box_mask_prompt(n, S, seed):
    """+-1000 plateaus with a bilinear-looking edge a few pixels wide, along the sides of a rotated rectangle (what
    samrs_rbox_mask_prompt writes): the edge runs through the 4 x 4 pixel blocks of many tokens at every phase."""
    g = gen(seed)
    yy, xx = torch.meshgrid(torch.arange(S, dtype=torch.float32), torch.arange(S, dtype=torch.float32), indexing="ij")
    out = []
    for i in range(n):
        cx, cy = (0.3 + 0.4 * torch.rand(2, generator=g)) * S
        hw, hh = (0.1 + 0.25 * torch.rand(2, generator=g)) * S
        th = float(torch.rand((), generator=g)) * math.pi
        u = (xx - cx) * math.cos(th) + (yy - cy) * math.sin(th)
        v = -(xx - cx) * math.sin(th) + (yy - cy) * math.cos(th)
        d = torch.minimum(hw - u.abs(), hh - v.abs())          # > 0 inside
        out.append((d * 600.0).clamp(-1000.0, 1000.0))
    return torch.stack(out)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("kind", ["gauss", "rbox", "constant"])
def test_mask_embed(lib, kind, n):
    grid = 64
    S = 4 * grid
    g = gen(7)
    p = dict(w0=torch.randn(4, 1, 2, 2, generator=g) * 0.5, b0=torch.randn(4, generator=g) * 0.5,
             ln1w=1 + 0.2 * torch.randn(4, generator=g), ln1b=0.2 * torch.randn(4, generator=g),
             w3=torch.randn(16, 4, 2, 2, generator=g) * 0.25, b3=torch.randn(16, generator=g) * 0.5,
             ln4w=1 + 0.2 * torch.randn(16, generator=g), ln4b=0.2 * torch.randn(16, generator=g),
             w6=torch.randn(256, 16, 1, 1, generator=g) * 0.25, b6=torch.randn(256, generator=g) * 0.5)
    if kind == "gauss":
        m = torch.randn(n, S, S, generator=g) * 2.0            # N(0, 4)
    elif kind == "rbox":
        m = box_mask_prompt(n, S, 5)
    else:
        m = torch.randn(n, S, S, generator=g) * 2.0
        m[0] = -1000.0                                          # one all-constant prompt
    ref = mask_embed_ref(p, m, torch.float64)
    bound, noise = fp32_bound(mask_embed_ref(p, m, torch.float32), ref)
    pd = {k: dev(v) for k, v in p.items()}
    out = Guarded((n, grid * grid, 256), torch.float32)
    args = [pd[k].data_ptr() for k in ("w0", "b0", "ln1w", "ln1b", "w3", "b3", "ln4w", "ln4b", "w6", "b6")]
    md = dev(m)
    assert lib.samrs_k_mask_embed(*args, md.data_ptr(), out.ptr, n, grid, stream()) == 0
    got = out.read(f"mask_embed {kind}")
    r = rel_l2(got, ref)
    print(f"mask_embed {kind} n={n}: rel L2 {r:.2e} (bound {bound:.2e}, fp32 noise {noise:.2e}), max abs {(got.double() - ref).abs().max().item():.2e}")
    assert r <= bound
    out2 = Guarded((n, 25, 256), torch.float32)
    assert lib.samrs_k_mask_embed(*args, md.data_ptr(), out2.ptr, n, 5, stream()) != 0       # 25 tokens: not 16 per block
    assert out2.untouched()


# ------------------------------------------------------------------------------------------------------------------
# slot table / keys
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_runs", [1, 64, 65, 150])
def test_fill_slot_table(lib, n_runs):
    """out[p] = slot[k] for start[k] <= p < start[k + 1]: the launcher walks the runs in chunks of 64; empty runs write nothing;
    one run is longer than the block that writes it."""
    rng = np.random.default_rng(n_runs)
    lens = rng.integers(0, 6, n_runs)
    if n_runs > 1:
        lens[0] = 0
        lens[-1] = 0
    lens[0 if n_runs == 1 else int(rng.integers(1, n_runs - 1))] = 150
    base = 3                                                    # the first run need not start at 0: entries in front stay untouched
    start = np.concatenate([[base], base + np.cumsum(lens)]).astype(np.int32)
    slot = rng.integers(0, 1000, n_runs).astype(np.int32)
    total = int(start[-1])
    out = Guarded((total,), torch.int32)
    ip = ctypes.POINTER(ctypes.c_int32)
    assert lib.samrs_k_fill_slot_table(start.ctypes.data_as(ip), slot.ctypes.data_as(ip), n_runs, out.ptr, stream()) == 0
    got = out.read("fill_slot_table").numpy()
    ref = np.full(total, I32_SENTINEL, dtype=np.int32)
    for k in range(n_runs):
        ref[start[k]:start[k + 1]] = slot[k]
    print(f"fill_slot_table {n_runs} runs ({int((lens == 0).sum())} empty), {total - base} prompts: {int((got != ref).sum())} wrong entries")
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS)
@pytest.mark.parametrize("tokens,n_batches", [(1001, 5), (4096, 1), (1001, 1), (4096, 5)])
@pytest.mark.parametrize("slots", [False, True], ids=["shared", "slot_of"])
@pytest.mark.parametrize("addend", ["dense", "vec"])
def test_make_keys(lib, name, prec, dt, ulp, tokens, n_batches, slots, addend):
    """keys = image embedding (of the prompt's slot) + dense prompt embedding (per prompt, or the broadcast no-mask vector):
    one fp32 add and one rounding to the operand type, both bit-exact; f16 saturates at +-65504."""
    C = 256
    g = gen(tokens + n_batches)
    n_slots = 4 if slots else 1
    emb = torch.randn(n_slots, tokens, C, generator=g) * torch.logspace(-4, 5, C)
    slot_of = torch.tensor([3, 1, 3, 0, 0], dtype=torch.int32)[:n_batches] if slots else None      # repeated and descending
    dense = torch.randn(n_batches, tokens, C, generator=g) * 30 if addend == "dense" else None
    vec = torch.randn(C, generator=g) * 30
    emb[0, 0, :8] = torch.tensor([65504.0, 65519.0, 65520.0, -65520.0, 7e4, -7e4, 3e38, 1e-8])
    e = emb[slot_of.long()] if slots else emb[:1].expand(n_batches, -1, -1)
    ref32 = e + (dense if dense is not None else vec)           # one IEEE fp32 add: exact statement
    _, ref_bits = et_bits(ref32, dt)
    of, oe = Guarded((n_batches, tokens, C), torch.float32), Guarded((n_batches, tokens, C), dt)
    ed, vd = dev(emb), dev(vec)
    dd = None if dense is None else dev(dense)
    sd = None if slot_of is None else dev(slot_of)
    rc = lib.samrs_k_make_keys(prec, ed.data_ptr(), None if dd is None else dd.data_ptr(), vd.data_ptr() if dd is None else None,
                               of.ptr, oe.ptr, n_batches, tokens, C, None if sd is None else sd.data_ptr(), stream())
    assert rc == 0
    gf = of.read("make_keys fp32")
    ge = oe.read("make_keys ET")
    nf = int((gf.view(torch.int32) != ref32.contiguous().view(torch.int32)).sum())
    ne = int((ge.view(torch.int16) != ref_bits).sum())
    print(f"make_keys {name} tokens={tokens} n={n_batches} {addend} slots={slots}: fp32 mismatches {nf}, ET mismatches {ne}, "
          f"|values| up to {ref32.abs().max().item():.3g}")
    assert nf == 0 and ne == 0


# ------------------------------------------------------------------------------------------------------------------
# token self attention
# ------------------------------------------------------------------------------------------------------------------
def self_attn_inputs(kind, n, T, seed):
    g = gen(seed)
    q, k, v = (torch.randn(n, T, 8, 32, generator=g) for _ in range(3))
    if kind == "uniform":
        q, k = q * 0.1, k * 0.1
    else:
        d = torch.randn(n, 1, 8, 32, generator=g)
        d = d / d.norm(dim=-1, keepdim=True) * math.sqrt(32.0)           # d . d / sqrt(32) = 5.66
        sign = torch.where(torch.arange(T) % 3 == 2, -1.0, 1.0).view(1, T, 1, 1)   # every third query sees descending scores
        q = sign * d + 0.05 * q
        if kind == "ascending":                                           # every key beats the running maximum: each step rescales
            alpha = 0.5 * torch.arange(T, dtype=torch.float32).view(1, T, 1, 1)
        else:                                                             # one dominant late key
            alpha = torch.zeros(T)
            alpha[max(T - 2, 0)] = 5.0
            alpha = alpha.view(1, T, 1, 1)
        k = alpha * d + 0.05 * k
    return q.reshape(n, T, 256), k.reshape(n, T, 256), v.reshape(n, T, 256)


@pytest.mark.parametrize("kind", ["uniform", "ascending", "dominant"])
@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("T", [5, 7, 8, 9, 14, 15, 16])
def test_token_self_attn(lib, T, n, kind):
    q, k, v = self_attn_inputs(kind, n, T, 1000 * T + n)
    ref = attention(q, k, v, 32, torch.float64)
    bound, noise = fp32_bound(attention(q, k, v, 32, torch.float32), ref)
    out = Guarded((n, T, 256), torch.float32)
    qd, kd, vd = dev(q), dev(k), dev(v)
    assert lib.samrs_k_token_self_attn(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.ptr, n, T, 256, 8, stream()) == 0
    r = rel_l2(out.read(f"token_self_attn T={T}"), ref)
    print(f"token_self_attn {kind} T={T} n={n}: rel L2 {r:.2e} (bound {bound:.2e}, fp32 noise {noise:.2e})")
    assert r <= bound


def test_token_self_attn_refuses_17_tokens(lib):
    q = dev(torch.randn(1, 17, 256, generator=gen(0)))
    out = Guarded((1, 17, 256), torch.float32)
    assert lib.samrs_k_token_self_attn(q.data_ptr(), q.data_ptr(), q.data_ptr(), out.ptr, 1, 17, 256, 8, stream()) != 0
    assert out.untouched()


# ------------------------------------------------------------------------------------------------------------------
# tokens -> image attention
# ------------------------------------------------------------------------------------------------------------------
SLOT_TABLE = [2, 0, 2, 1, 0]          # repeated and descending


def image_side(mode, n):
    """(batches stored, batch stride in rows as a factor of tokens, slot table or None, stored batch of prompt b)"""
    if mode == "shared":
        return 1, 0, None, [0] * n
    if mode == "batched":
        return n, 1, None, list(range(n))
    return 3, 1, SLOT_TABLE[:n], SLOT_TABLE[:n]


def t2i_inputs(kind, n, T, tokens, nb, ld, dt, seed):
    g = gen(seed)
    q = torch.randn(n, T, 8, 16, generator=g)
    K = torch.randn(nb, tokens, 8, 16, generator=g)
    V = torch.randn(nb, tokens, 128, generator=g)
    if kind == "uniform":
        q = q * 0.1
    elif kind == "wide":                                  # scores = q . k / 4 ~ N(0, 16^2): +-60 over 4096 keys
        q = q * 16.0
    else:                                                 # spiky: the dominant key sits in the last (partial) wave of the last split,
        d = torch.randn(8, 16, generator=g)               # the runner-up in the first wave of the first split
        d = d / d.norm(dim=-1, keepdim=True) * 4.0        # d . d / 4 = 4
        s = 0.5 + torch.rand(n, T, 8, 1, generator=g)
        q = s * d + 0.05 * q
        K = K * 0.3
        K[:, tokens - 3] = 4.0 * d                        # score 16 s
        K[:, 5] = 3.6 * d                                 # score 14.4 s
    kv = torch.randn(nb, tokens, ld, generator=g)         # columns behind K | V hold other data (the i2t queries in the engine)
    kv[..., :128] = K.reshape(nb, tokens, 128)
    kv[..., 128:256] = V
    kvr, kvb = et_bits(kv, dt)
    return q.reshape(n, T, 128), kvr[..., :128], kvr[..., 128:256], kvb


def t2i_cases():
    Ts, kinds, modes = [5, 7, 8, 9, 15, 16], ["uniform", "spiky", "wide"], ["shared", "batched", "slots"]
    out, i = [], 0
    for tokens in [4096, 1024, 1000, 200, 100, 40]:
        for kind in kinds:
            out.append((Ts[i % 6], tokens, [1, 5][(i // 2) % 2], [384, 256][i % 2], modes[(i // 3 + i) % 3], kind))
            i += 1
    # every T on the partial last wave with the slot table, every mode at 16 tokens on the full geometry
    out += [(T, 1000, 5, 384, "slots", "spiky") for T in Ts]
    out += [(16, 4096, 5, 384, m, "spiky") for m in modes] + [(15, 4096, 5, 256, "slots", "wide"), (9, 40, 5, 256, "slots", "uniform")]
    # the counts above leave every wave a multiple of 8 keys except 100: an iteration of the key loop takes 2 groups of 4 keys, and only
    # a wave whose share is not a multiple of 8 (of 4) has masked keys INSIDE an iteration (a group).  1003 -> 43 keys in the last
    # wave, 4093 -> 61, 37 -> 5, 100 -> 4
    for tokens, T, n, mode in [(1003, 9, 5, "slots"), (4093, 16, 1, "shared"), (37, 7, 5, "batched"), (100, 15, 5, "shared")]:
        out += [(T, tokens, n, 384, mode, kind) for kind in ("uniform", "spiky")]
    return sorted(set(out))


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS)
@pytest.mark.parametrize("T,tokens,n,ld,mode,kind", t2i_cases())
def test_t2i_attention(lib, name, prec, dt, ulp, T, tokens, n, ld, mode, kind):
    """transformer.py:163-169 / :98-104, head dim 16: fp32 queries, ET keys / values read in place from the rows of the projection
    GEMM's output (K | V | ... of `ld` columns).  tokens below 4096 leave the last wave partial (1000, 200, 100, 40) or without
    keys (40); T above 8 runs the second token group.  The merge order is fixed: a second run is bit-identical."""
    nb, bs, slot_of, idx = image_side(mode, n)
    q, K, V, kvb = t2i_inputs(kind, n, T, tokens, nb, ld, dt, 7 * T + tokens + n)
    ref = attention(q, K[idx], V[idx], 16, torch.float64)
    bound, noise = fp32_bound(attention(q, K[idx], V[idx], 16, torch.float32), ref)
    kvd, qd = dev(kvb), dev(q)
    sd = None if slot_of is None else dev(torch.tensor(slot_of, dtype=torch.int32))
    nws = lib.samrs_k_t2i_workspace_floats(n, T)
    runs = []
    for _ in range(2):
        out, ws = Guarded((n, T, 128), torch.float32), Guarded((nws,), torch.float32, rows=1)
        rc = lib.samrs_k_t2i_attention(prec, qd.data_ptr(), kvd.data_ptr(), kvd.data_ptr() + 128 * 2, ld, bs * tokens, out.ptr, ws.ptr,
                                       n, T, tokens, 128, 8, None if sd is None else sd.data_ptr(), stream())
        assert rc == 0
        ws.read("t2i workspace", finite=False)
        runs.append(out)
    got = runs[0].read(f"t2i_attention T={T} tokens={tokens}")
    r = rel_l2(got, ref)
    print(f"t2i_attention {name} {kind} T={T} tokens={tokens} n={n} ld={ld} {mode}: rel L2 {r:.2e} (bound {bound:.2e}, "
          f"fp32 noise {noise:.2e}), max abs {(got.double() - ref).abs().max().item():.2e}")
    assert r <= bound
    assert torch.equal(runs[0].bits(), runs[1].bits()), "two runs differ: the merge order is not fixed"


def test_t2i_attention_refusals(lib):
    q = dev(torch.zeros(1, 17, 128))
    kv = dev(torch.zeros(64, 256, dtype=torch.int16))
    out, ws = Guarded((1, 17, 128), torch.float32), Guarded((lib.samrs_k_t2i_workspace_floats(1, 17),), torch.float32, rows=1)
    a = (q.data_ptr(), kv.data_ptr(), kv.data_ptr() + 256, 256, 0, out.ptr)
    assert lib.samrs_k_t2i_attention(1, *a, ws.ptr, 1, 17, 64, 128, 8, None, stream()) != 0       # 17 tokens
    assert lib.samrs_k_t2i_attention(1, *a, None, 1, 16, 64, 128, 8, None, stream()) != 0         # no workspace
    assert lib.samrs_k_t2i_attention(1, *a, ws.ptr, 1, 16, 64, 256, 8, None, stream()) != 0       # head dim 32
    assert out.untouched() and ws.untouched()


# ------------------------------------------------------------------------------------------------------------------
# image -> tokens attention
# ------------------------------------------------------------------------------------------------------------------
def i2t_inputs(kind, n, T, tokens, nb, dt, seed, big_mean=False):
    g = gen(seed)
    rows = torch.randn(nb, tokens, 384, generator=g)      # K | V | Q rows of the projection GEMM: the queries are columns 256 ..
    rr, rb = et_bits(rows, dt)
    kt = torch.randn(n, T, 128, generator=g) * (3.0 if kind == "peaked" else 0.1)
    vt = torch.randn(n, T, 128, generator=g)
    return rr[..., 256:], rb, kt, vt


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS)
@pytest.mark.parametrize("kind", ["uniform", "peaked"])
@pytest.mark.parametrize("tokens,T,n,mode", [(4096, 5, 3, "batched"), (4096, 7, 1, "shared"), (4096, 8, 3, "shared"), (4096, 9, 1, "batched"),
                                             (4096, 15, 3, "batched"), (4096, 16, 3, "shared"), (1000, 5, 3, "shared"), (1000, 7, 3, "batched"),
                                             (1000, 8, 1, "batched"), (1000, 9, 3, "shared"), (1000, 15, 1, "shared"), (1000, 16, 3, "batched")])
def test_i2t_attention(lib, name, prec, dt, ulp, kind, tokens, T, n, mode):
    """transformer.py:176-181 without the projection: ET queries at column 256 of 384-column rows, fp32 token keys / values, ET
    output.  1000 tokens leave the last block of 32 partly empty."""
    nb, bs, _, idx = image_side(mode, n)
    q, rb, kt, vt = i2t_inputs(kind, n, T, tokens, nb, dt, 13 * T + tokens + n)
    ref = attention(q[idx], kt, vt, 16, torch.float64)
    bound, noise = fp32_bound(attention(q[idx], kt, vt, 16, torch.float32), ref)
    rd, kd, vd = dev(rb), dev(kt), dev(vt)
    out = Guarded((n, tokens, 128), dt)
    assert lib.samrs_k_i2t_attention(prec, rd.data_ptr() + 256 * 2, 384, bs * tokens, kd.data_ptr(), vd.data_ptr(), out.ptr,
                                     n, T, tokens, 128, 8, stream()) == 0
    got = out.read(f"i2t_attention T={T} tokens={tokens}").float()
    x = et_excess(got, ref, ulp)
    print(f"i2t_attention {name} {kind} T={T} tokens={tokens} n={n} {mode}: beyond one ET ulp: rel L2 {x:.2e} (bound {bound:.2e}, "
          f"fp32 noise {noise:.2e}); plain rel L2 {rel_l2(got, ref):.2e}")
    assert x <= bound


# ------------------------------------------------------------------------------------------------------------------
# fused image -> tokens attention + out-projection + residual + LayerNorm
# ------------------------------------------------------------------------------------------------------------------
def fused_ref(dtype, q, kt, vt, w, w_hi, w_lo, bias, resid, gamma, beta, dt, split, rounded=True):
    """The composite the kernel states: attention -> ET (split: hi + lo) -> x ET weights (split: hi + lo, hi hi + lo hi + hi lo)
    -> + bias + residual -> LayerNorm(1e-5).  rounded=False: the un-rounded attention output times the fp32 weights."""
    o = attention(q, kt, vt, 16, dtype)
    if rounded:
        oh = round_et(o, dt)
        y = oh @ w_hi.to(dtype).t()
        if split:
            y = y + round_et(o - oh, dt) @ w_hi.to(dtype).t() + oh @ w_lo.to(dtype).t()
    else:
        y = o @ w.to(dtype).t()
    y = y + bias.to(dtype) + resid.to(dtype)
    return F.layer_norm(y, (256,), gamma.to(dtype), beta.to(dtype), 1e-5)


FUSED_CASES = [
    # tokens, T, n, mode, kind, split, outF, outE_lo
    (4096, 5, 3, "batched", "uniform", False, True, False),
    (4096, 9, 2, "shared", "peaked", True, True, True),
    (4096, 16, 3, "slots", "peaked", True, False, True),
    (4096, 16, 1, "shared", "bigmean", False, True, False),
    (192, 5, 3, "shared", "peaked", True, True, False),
    (192, 9, 5, "slots", "uniform", False, False, False),
    (192, 16, 3, "batched", "bigmean", True, True, True),
    (160, 5, 1, "batched", "peaked", False, True, True),
    (160, 9, 3, "batched", "bigmean", True, False, False),
    (160, 16, 5, "slots", "peaked", False, True, False),
    (160, 16, 3, "shared", "uniform", True, True, True),
]


def fused_inputs(kind, n, T, tokens, nb, dt, seed):
    g = gen(seed + 1)
    q, rb, kt, vt = i2t_inputs("peaked" if kind != "uniform" else "uniform", n, T, tokens, nb, dt, seed)
    w = torch.randn(256, 128, generator=g) / math.sqrt(128.0)
    w_hi, w_hib = et_bits(w, dt)
    w_lo, w_lob = et_bits(w - w_hi, dt)
    bias = torch.randn(256, generator=g) * 0.5
    gamma, beta = 1 + 0.2 * torch.randn(256, generator=g), 0.2 * torch.randn(256, generator=g)
    resid = torch.randn(nb, tokens, 256, generator=g)
    if kind == "bigmean":                                 # mean >> spread: the LayerNorm's subtraction cancels
        resid = resid + 300.0
    return q, rb, kt, vt, w, w_hi, w_hib, w_lo, w_lob, bias, gamma, beta, resid


def run_fused(lib, prec, dt, rd, q_bs, kt, vt, w_hib, w_lob, bias, resid, r_bs, gamma, beta, n, T, tokens, sd, outF, outE_lo):
    oF, oE, oL = (Guarded((n, tokens, 256), t) for t in (torch.float32, dt, dt))
    keep = [dev(t) for t in (kt, vt, w_hib, bias, resid, gamma, beta)] + ([dev(w_lob)] if w_lob is not None else [])
    rc = lib.samrs_k_i2t_fused(prec, rd.data_ptr() + 256 * 2, 384, q_bs, keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(),
                               keep[7].data_ptr() if w_lob is not None else None, keep[3].data_ptr(), keep[4].data_ptr(), r_bs,
                               keep[5].data_ptr(), keep[6].data_ptr(), 1e-5, oF.ptr if outF else None, oE.ptr, oL.ptr if outE_lo else None,
                               n, T, tokens, 128, 256, None if sd is None else sd.data_ptr(), stream())
    torch.cuda.synchronize()
    return rc, oF, oE, oL


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS)
@pytest.mark.parametrize("tokens,T,n,mode,kind,split,outF,outE_lo", FUSED_CASES)
def test_i2t_fused(lib, name, prec, dt, ulp, tokens, T, n, mode, kind, split, outF, outE_lo):
    """transformer.py:176-181 in one kernel.  4096 tokens = 4 groups of 32 per block, 192 = 2, 160 = 1.  The image side (queries,
    residual) is shared (strides 0), per prompt, or per slot through the table; "bigmean" puts the residual rows at 300 +- 1.
    outF against the fp64 composite; outE bit-equal to ET(outF) and outE_lo to ET(outF - outE) on the kernel's own output; where
    outF is not written (the last layer), outE must be bit-equal to the run that writes it."""
    nb, bs, slot_of, idx = image_side(mode, n)
    q, rb, kt, vt, w, w_hi, w_hib, w_lo, w_lob, bias, gamma, beta, resid = fused_inputs(kind, n, T, tokens, nb, dt, 17 * T + tokens + n)
    a = (q[idx], kt, vt, w, w_hi, w_lo, bias, resid[idx], gamma, beta, dt, split)
    ref = fused_ref(torch.float64, *a)
    bound, noise = fp32_bound(fused_ref(torch.float32, *a), ref)
    rd = dev(rb)
    sd = None if slot_of is None else dev(torch.tensor(slot_of, dtype=torch.int32))
    common = (lib, prec, dt, rd, bs * tokens, kt, vt, w_hib, w_lob if split else None, bias, resid, bs * tokens, gamma, beta, n, T, tokens, sd)
    rc, oF, oE, oL = run_fused(*common, True, True)
    assert rc == 0
    gF = oF.read(f"i2t_fused outF tokens={tokens} T={T}")
    gE, gL = oE.read("i2t_fused outE"), oL.read("i2t_fused outE_lo")
    r = rel_l2(gF, ref)
    x = et_excess(gE.float(), ref, ulp)
    print(f"i2t_fused {name} {kind} tokens={tokens} T={T} n={n} {mode} split={split}: outF rel L2 {r:.2e} (bound {bound:.2e}, fp32 noise "
          f"{noise:.2e}); outE beyond one ET ulp {x:.2e}")
    assert r <= bound
    assert x <= bound
    eF, eFb = et_bits(gF, dt)
    assert torch.equal(gE.view(torch.int16), eFb), "outE is not ET(outF)"
    assert torch.equal(gL.view(torch.int16), et_bits(gF - eF, dt)[1]), "outE_lo is not ET(outF - outE)"
    if not (outF and outE_lo):                       # the variant the case names: absent outputs stay untouched, present ones are the same bits
        rc, pF, pE, pL = run_fused(*common, outF, outE_lo)
        assert rc == 0
        assert torch.equal(pE.read("i2t_fused outE (variant)").view(torch.int16), gE.view(torch.int16))
        if outF:
            assert torch.equal(pF.read("outF (variant)").view(torch.int32), gF.view(torch.int32))
        else:
            assert pF.untouched()
        if outE_lo:
            assert torch.equal(pL.read("outE_lo (variant)").view(torch.int16), gL.view(torch.int16))
        else:
            assert pL.untouched()


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS)
def test_i2t_fused_split_precision(lib, name, prec, dt, ulp):
    """The split out-projection against the fp64 composite of the UN-rounded attention output and the fp32 weights
    (test_gemm_gln_split_precision's criterion: max |err| / max(|ref|, 1e-2) an order of magnitude under one operand ulp:
    1e-4 f16, 2e-3 bf16): the split meets it, the un-split product does not."""
    tokens, T, n = 192, 9, 2
    q, rb, kt, vt, w, w_hi, w_hib, w_lo, w_lob, bias, gamma, beta, resid = fused_inputs("peaked", n, T, tokens, n, dt, 99)
    ref = fused_ref(torch.float64, q, kt, vt, w, w_hi, w_lo, bias, resid, gamma, beta, dt, True, rounded=False)
    crit = 1e-4 if name == "f16" else 2e-3
    errs = {}
    for split in (True, False):
        rc, oF, _, _ = run_fused(lib, prec, dt, dev(rb), tokens, kt, vt, w_hib, w_lob if split else None, bias, resid, tokens, gamma, beta,
                                 n, T, tokens, None, True, False)
        assert rc == 0
        got = oF.read("i2t_fused outF").double()
        errs[split] = ((got - ref).abs() / ref.abs().clamp(min=1e-2)).max().item()
    print(f"i2t_fused split precision {name}: max rel err split {errs[True]:.2e}, un-split {errs[False]:.2e} (criterion {crit:.0e}, "
          f"one operand ulp {ulp:.1e})")
    assert errs[True] < crit
    assert errs[False] >= crit


def test_i2t_fused_refuses_what_it_does_not_cover(lib):
    name, prec, dt, ulp = PRECS[0]
    for tokens, T in ((100, 9), (160, 17), (160, 0)):
        q, rb, kt, vt, w, w_hi, w_hib, w_lo, w_lob, bias, gamma, beta, resid = fused_inputs("uniform", 1, max(T, 1), max(tokens, 128), 1, dt, 3)
        rc, oF, oE, oL = run_fused(lib, prec, dt, dev(rb), 0, kt, vt, w_hib, None, bias, resid, 0, gamma, beta, 1, T, tokens, None, True, True)
        assert rc != 0, (tokens, T)
        assert oF.untouched() and oE.untouched() and oL.untouched()


# ------------------------------------------------------------------------------------------------------------------
# upscaler pieces of the un-fused path
# ------------------------------------------------------------------------------------------------------------------
def group_ln_gelu_ref(x, gamma, beta, dtype):
    """mask_decoder.py:55-56 on rows of 4 x 64: LayerNorm2d(64), eps 1e-6, exact-erf GELU"""
    y = x.to(dtype).view(x.shape[0], 4, 64)
    u = y.mean(-1, keepdim=True)
    s = ((y - u) ** 2).mean(-1, keepdim=True)
    return F.gelu((y - u) / torch.sqrt(s + 1e-6) * gamma.to(dtype) + beta.to(dtype)).view(x.shape[0], 256)


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS)
@pytest.mark.parametrize("kind", ["normal", "bigmean"])
@pytest.mark.parametrize("rows", [1, 4, 5, 16387])
def test_group_ln_gelu(lib, name, prec, dt, ulp, rows, kind):
    """One wave per row, four rows per block: 1, 5 and 16387 rows leave the last block partly empty.  Group 1 of row 0 (and of
    every 1000th row) is all-constant: variance 0, the eps path, output GELU(beta)."""
    g = gen(rows)
    x = torch.randn(rows, 256, generator=g)
    if kind == "bigmean":
        x = x + 1000.0
    x.view(rows, 4, 64)[::1000, 1] = 1000.0 if kind == "bigmean" else 3.0       # sums of 64 equal values are exact in fp32
    gamma, beta = 1 + 0.2 * torch.randn(64, generator=g), 0.2 * torch.randn(64, generator=g)
    ref = group_ln_gelu_ref(x, gamma, beta, torch.float64)
    bound, noise = fp32_bound(group_ln_gelu_ref(x, gamma, beta, torch.float32), ref)
    out = Guarded((rows, 256), dt)
    xd, gd, bd = dev(x), dev(gamma), dev(beta)
    assert lib.samrs_k_group_ln_gelu(prec, xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), 1e-6, out.ptr, rows, 4, 64, stream()) == 0
    got = out.read(f"group_ln_gelu rows={rows} {kind}").float()
    e = et_excess(got, ref, ulp)
    const = (got.view(rows, 4, 64)[::1000, 1].double() - ref.view(rows, 4, 64)[::1000, 1]).abs().max().item()
    print(f"group_ln_gelu {name} {kind} rows={rows}: beyond one ET ulp: rel L2 {e:.2e} (bound {bound:.2e}, fp32 noise {noise:.2e}); "
          f"constant groups: max abs err {const:.2e}")
    assert e <= bound
    out2 = Guarded((4, 256), dt)
    assert lib.samrs_k_group_ln_gelu(prec, xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), 1e-6, out2.ptr, 1, 8, 32, stream()) != 0
    assert out2.untouched()


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("n_sel,sel0", [(1, 0), (3, 1), (4, 0)])
@pytest.mark.parametrize("grid", [64, 16])
def test_mask_product(lib, name, prec, dt, ulp, grid, n_sel, sel0, n):
    """mask_decoder.py:154-167: low[b, c, Y, X] = hyper[b, sel0 + c] . up2[b, pixel(Y, X)].  up2 rows run over (token y, x), the
    sub-pixel of ConvT #1 (dy, dx), the sub-pixel of ConvT #2 (dy2, dx2); Y = 4 y + 2 dy + dy2, X = 4 x + 2 dx + dx2 -- stated
    here as a permutation of the axes, not as index arithmetic."""
    g = gen(grid + n_sel + n)
    up2, up2b = et_bits(torch.randn(n, grid, grid, 2, 2, 2, 2, 32, generator=g), dt)
    hyper = torch.randn(n, 4, 32, generator=g)
    img = up2.permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(n, 4 * grid, 4 * grid, 32)      # (y, dy, dy2) -> Y, (x, dx, dx2) -> X
    sel = hyper[:, sel0:sel0 + n_sel]
    ref = torch.einsum("bck,byxk->bcyx", sel.double(), img.double())
    bound, noise = fp32_bound(torch.einsum("bck,byxk->bcyx", sel, img), ref)
    out = Guarded((n, n_sel, 4 * grid, 4 * grid), torch.float32)
    ud, hd = dev(up2b), dev(hyper)
    assert lib.samrs_k_mask_product(prec, ud.data_ptr(), hd.data_ptr(), out.ptr, n, grid, 4, sel0, n_sel, stream()) == 0
    r = rel_l2(out.read(f"mask_product grid={grid}"), ref)
    print(f"mask_product {name} grid={grid} n={n} n_sel={n_sel} sel0={sel0}: rel L2 {r:.2e} (bound {bound:.2e}, fp32 noise {noise:.2e})")
    assert r <= bound
    out2 = Guarded((n, 5, 4 * grid, 4 * grid), torch.float32)
    assert lib.samrs_k_mask_product(prec, ud.data_ptr(), hd.data_ptr(), out2.ptr, n, grid, 4, 0, 5, stream()) != 0
    assert lib.samrs_k_mask_product(prec, ud.data_ptr(), hd.data_ptr(), out2.ptr, n, grid, 4, 2, 3, stream()) != 0
    assert out2.untouched()

"""GPU: the fused upscaler's 32-token tile (samrs_amd/csrc/upscaler_fused.hip).

A tile is two 16-token groups; after the K halves of ConvT #1 have met in LDS each wave of a column group takes ONE group through
LayerNorm2d, GELU, ConvT #2, GELU and the hypernetwork dot.  Checked here:
  * against the fp64 chain of tests/test_kernels_gpu.py::test_upscaler_fused_one_kernel, with its tolerances, on a NaN-filled
    `low`, at n = 3, grid = 16 (8 tiles per prompt, a tile spans two grid rows), n = 1, grid = 32 (a tile is one grid row) and
    n = 3, grid = 64 (the persistent walk: more tiles than blocks);
  * byte for byte against the 16-token tile (SAMRS_UPSCALER_TILE=16): the switch is read once per process, so the same seeded
    calls run in two fresh child processes.

Run as a script (`python tests/test_upscaler_tile32_gpu.py OUT.npz`) this file is that child: it runs every case and saves `low`.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from test_kernels_gpu import PRECS, dev, rel_err, split_bits, stream  # noqa: E402

pytestmark = pytest.mark.gpu

# (prompts, grid).  (3, 64): 384 tiles of 32 tokens / 768 of 16 -- more tiles than a 256-CU device has blocks, so both tile shapes walk
# (1 - 2 and 3 tiles per block), prefetch the next tile's keys and cross prompt boundaries (tests/test_upscaler_kernels_gpu.py)
SHAPES = [(3, 16), (1, 32), (3, 64)]
SELS = [(1, 0), (3, 1)]              # (n_sel, sel0)
TOL = {("f16", False): 4e-4, ("f16", True): 1e-5, ("bf16", False): 3e-3, ("bf16", True): 2e-4}
CHILD_TIMEOUT_S = 240             # a child takes 2 - 3 s on the MI355X: the import, 24 cases, the largest 12288 tokens


@pytest.fixture(scope="module")
def lib():
    from samrs_amd import engine
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return engine.load_library()


def make_inputs(dt, split, n, grid, n_sel):
    g = torch.Generator().manual_seed(3000 + 100 * grid + n_sel + 10 * split)
    keys = torch.randn(n * grid * grid, 256, generator=g)
    w1 = torch.randn(256, 256, generator=g) / 16
    b1 = 0.3 * torch.randn(256, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(64, generator=g), 0.2 * torch.randn(64, generator=g)
    w2 = torch.randn(128, 64, generator=g) / 8
    b2 = 0.3 * torch.randn(128, generator=g)
    hyper = torch.randn(n, 4, 32, generator=g)
    if not split:
        keys, w1, w2 = keys.to(dt).float(), w1.to(dt).float(), w2.to(dt).float()
    return keys, w1, b1, gamma, beta, w2, b2, hyper


def reference(inputs, dt, split, n, grid, n_sel, sel0):
    """mask_decoder.py:53-59,154-167 in fp64: the two transposed convolutions as per-token GEMMs"""
    keys, w1, b1, gamma, beta, w2, b2, hyper = inputs
    y = (keys.double() @ w1.double().t() + b1.double()).view(-1, 4, 64)                        # (token, s1, c)
    mu = y.mean(-1, keepdim=True)
    u1 = F.gelu((y - mu) / torch.sqrt(((y - mu) ** 2).mean(-1, keepdim=True) + 1e-6) * gamma.double() + beta.double())
    u1r = u1 if split else u1.float().to(dt).double()                                             # the un-split kernel rounds here
    up2 = F.gelu(u1r.reshape(-1, 64) @ w2.double().t() + b2.double())                            # rows (token, s1), cols (s2, c2)
    up2 = up2.view(n, grid, grid, 2, 2, 2, 2, 32)                                                # b, y, x, dy, dx, dy2, dx2, c
    S = 4 * grid
    return torch.einsum("byxijklc,bsc->bsyikxjl", up2, hyper[:, sel0:sel0 + n_sel].double()).reshape(n, n_sel, S, S)


def run_kernel(lib, prec, dt, split, n, grid, n_sel, sel0, inputs):
    """-> low [n][n_sel][4 grid][4 grid] fp32 on the host; every element starts as NaN"""
    keys, w1, b1, gamma, beta, w2, b2, hyper = inputs
    S = 4 * grid
    low = torch.full((n, n_sel, S, S), float("nan"), device="cuda")
    if split:
        kh, kl = split_bits(lib, prec, keys)
        w1h, w1l = split_bits(lib, prec, w1)
        w2h, w2l = split_bits(lib, prec, w2)
        ptrs = (kh.data_ptr(), kl.data_ptr(), w1h.data_ptr(), w1l.data_ptr(), w2h.data_ptr(), w2l.data_ptr())
    else:
        kh, w1h, w2h = dev(keys.to(dt).view(torch.int16)), dev(w1.to(dt).view(torch.int16)), dev(w2.to(dt).view(torch.int16))
        ptrs = (kh.data_ptr(), None, w1h.data_ptr(), None, w2h.data_ptr(), None)
    gb = dev(torch.cat([gamma, beta]))
    assert lib.samrs_k_upscaler_fused(prec, ptrs[0], ptrs[1], ptrs[2], ptrs[3], dev(b1).data_ptr(), gb.data_ptr(), ptrs[4], ptrs[5],
                                      dev(b2).data_ptr(), dev(hyper).data_ptr(), low.data_ptr(), n, grid, 4, sel0, n_sel, stream()) == 0
    torch.cuda.synchronize()
    return low.cpu()


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS)
@pytest.mark.parametrize("n_sel,sel0", SELS)
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("n,grid", SHAPES)
def test_upscaler_fused_32_token_tile(lib, name, prec, dt, ulp, n_sel, sel0, split, n, grid):
    inputs = make_inputs(dt, split, n, grid, n_sel)
    low = run_kernel(lib, prec, dt, split, n, grid, n_sel, sel0, inputs)
    assert not torch.isnan(low).any(), "some low-res pixels were never written"
    r, mx = rel_err(low, reference(inputs, dt, split, n, grid, n_sel, sel0))
    print(f"fused upscaler, 32-token tile {name} split={split} n_sel={n_sel} n={n} grid={grid}: rel {r:.2e} max {mx:.2e}")
    assert r < TOL[(name, split)]


def _child(out_path):
    from samrs_amd import engine
    lib = engine.load_library()
    outs = {}
    for name, prec, dt, _ in PRECS:
        for split in (False, True):
            for n_sel, sel0 in SELS:
                for n, grid in SHAPES:
                    low = run_kernel(lib, prec, dt, split, n, grid, n_sel, sel0, make_inputs(dt, split, n, grid, n_sel))
                    outs[f"{name}_split{int(split)}_sel{n_sel}_n{n}_g{grid}"] = low.numpy()
    np.savez(out_path, **outs)


def _run_child(out_path, env_extra):
    env = dict(os.environ)
    env.pop("SAMRS_UPSCALER_TILE", None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out_path], env=env, cwd=ROOT, timeout=CHILD_TIMEOUT_S,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, f"child with {env_extra} ended with {r.returncode}:\n{r.stdout[-2000:]}"
    return np.load(out_path)


def test_32_token_tile_is_bit_identical_to_16_token_tile(tmp_path):
    """Same seeded calls, default (32 tokens) against SAMRS_UPSCALER_TILE=16, each in a fresh process under its own time limit; the
    second one starts only after the first ended clean (the assert in _run_child and a TimeoutExpired both end the test)."""
    t32 = _run_child(str(tmp_path / "tile32.npz"), {})
    t16 = _run_child(str(tmp_path / "tile16.npz"), {"SAMRS_UPSCALER_TILE": "16"})
    assert sorted(t32.files) == sorted(t16.files) and len(t32.files) == len(PRECS) * 2 * len(SELS) * len(SHAPES)
    for k in t32.files:
        assert not np.isnan(t32[k]).any() and t32[k].tobytes() == t16[k].tobytes(), f"{k}: the two tile shapes differ"


if __name__ == "__main__":
    _child(sys.argv[1])

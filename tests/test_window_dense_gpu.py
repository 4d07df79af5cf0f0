"""GPU: the windowed attention kernel's dense query numbering (samrs_amd/csrc/encoder_kernels.hip).

A bottom / right window holds fewer than 196 real queries; the kernel numbers them densely and only the waves whose 32-query
strip holds a real query run the key-tile loop.  Checked here:
  * against the fp64 statement of tests/test_kernels_gpu.py, with its tolerances, on grids whose edge windows need 1, 2, 3 and 4
    strips (each grid has full interior windows too), on an output filled with NaN so that a row no strip wrote fails;
  * byte for byte against the window-order numbering (SAMRS_WIN_DENSE=0): the switch is read once per process, so the same seeded
    calls run in two fresh child processes.

Run as a script (`python tests/test_window_dense_gpu.py OUT.npz`) this file is that child: it runs every case and saves the raw
output bits.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from test_kernels_gpu import PRECS, _attention_ref, dev, et_bits, rel_err, stream  # noqa: E402

pytestmark = pytest.mark.gpu

WIN = 14
HEADS = [(80, 2), (64, 2)]
# grid: real queries of an edge window -> strips | of the corner window -> strips
#   64: 8 x 14 = 112 -> 4 (the last one half full) | 8 x 8 = 64 -> 2
#   30: 2 x 14 = 28 -> 1                           | 2 x 2 = 4 -> 1
#   20: 6 x 14 = 84 -> 3                           | 6 x 6 = 36 -> 2
#   37: 9 x 14 = 126 -> 4                          | 9 x 9 = 81 -> 3
GRIDS = [64, 30, 20, 37]
N_IMG = 2
CHILD_TIMEOUT_S = 240


@pytest.fixture(scope="module")
def lib():
    from samrs_amd import engine
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return engine.load_library()


def make_inputs(dt, hd, heads, grid):
    g = torch.Generator().manual_seed(1000 * grid + hd)
    D = hd * heads
    qkv, qkvb = et_bits(torch.randn(N_IMG, grid, grid, 3 * D, generator=g), dt)
    bias, _ = et_bits(0.5 * torch.randn(3 * D, generator=g), dt)       # pre-rounded: the GEMM epilogue rounds too
    rel_h, _ = et_bits(0.3 * torch.randn(2 * WIN - 1, hd, generator=g), dt)
    rel_w, _ = et_bits(0.3 * torch.randn(2 * WIN - 1, hd, generator=g), dt)
    return qkv, qkvb, bias, rel_h, rel_w


def run_kernel(lib, prec, dt, hd, heads, grid, inputs):
    """-> the raw output [n_img * grid * grid][D] as int16 bits; every element starts as a NaN of the element type"""
    _, qkvb, bias, rel_h, rel_w = inputs
    D = hd * heads
    out = torch.full((N_IMG * grid * grid, D), float("nan"), dtype=dt, device="cuda").view(torch.int16)
    qd, bd, rhd, rwd = dev(qkvb), dev(bias), dev(rel_h), dev(rel_w)
    assert lib.samrs_k_window_attention(prec, qd.data_ptr(), bd.data_ptr(), rhd.data_ptr(), rwd.data_ptr(), out.data_ptr(),
                                        N_IMG, grid, WIN, heads, hd, stream()) == 0
    torch.cuda.synchronize()
    return out.cpu()


def reference(inputs, hd, heads, grid):
    """pad with the bias rows, partition (image_encoder.py:243-264), attend in fp64, un-partition + crop"""
    qkv, _, bias, rel_h, rel_w = inputs
    D = hd * heads
    nw = (grid + WIN - 1) // WIN
    padded = bias.view(1, 1, 1, -1).expand(N_IMG, nw * WIN, nw * WIN, 3 * D).clone()
    padded[:, :grid, :grid] = qkv
    xw = padded.view(N_IMG, nw, WIN, nw, WIN, 3 * D).permute(0, 1, 3, 2, 4, 5).reshape(N_IMG * nw * nw, WIN * WIN, 3 * D)
    ref_w = _attention_ref(xw, rel_h, rel_w, heads, WIN)
    return ref_w.view(N_IMG, nw, nw, WIN, WIN, D).permute(0, 1, 3, 2, 4, 5).reshape(N_IMG, nw * WIN, nw * WIN, D)[:, :grid, :grid]


@pytest.mark.parametrize("name,prec,dt,ulp", PRECS)
@pytest.mark.parametrize("hd,heads", HEADS)
@pytest.mark.parametrize("grid", GRIDS)
def test_window_attention_dense_strips(lib, name, prec, dt, ulp, hd, heads, grid):
    inputs = make_inputs(dt, hd, heads, grid)
    got = run_kernel(lib, prec, dt, hd, heads, grid, inputs).view(dt).float().view(N_IMG, grid, grid, hd * heads)
    assert torch.isfinite(got).all(), "some output rows were never written"
    r, mx = rel_err(got, reference(inputs, hd, heads, grid))
    print(f"window attention dense {name} hd={hd} grid={grid}: rel {r:.2e} max {mx:.2e}")
    assert r < (3e-3 if name == "f16" else 2e-2)


def _child(out_path):
    from samrs_amd import engine
    lib = engine.load_library()
    outs = {}
    for name, prec, dt, _ in PRECS:
        for hd, heads in HEADS:
            for grid in GRIDS:
                outs[f"{name}_hd{hd}_g{grid}"] = run_kernel(lib, prec, dt, hd, heads, grid, make_inputs(dt, hd, heads, grid)).numpy()
    np.savez(out_path, **outs)


def _run_child(out_path, env_extra):
    env = dict(os.environ)
    env.pop("SAMRS_WIN_DENSE", None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out_path], env=env, cwd=ROOT, timeout=CHILD_TIMEOUT_S,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, f"child with {env_extra} ended with {r.returncode}:\n{r.stdout[-2000:]}"
    return np.load(out_path)


def test_dense_numbering_is_bit_identical_to_window_order(tmp_path):
    """Same seeded calls, default (dense) against SAMRS_WIN_DENSE=0, each in a fresh process under its own time limit; the second
    one starts only after the first ended clean (the assert in _run_child and a TimeoutExpired both end the test)."""
    dense = _run_child(str(tmp_path / "dense.npz"), {})
    plain = _run_child(str(tmp_path / "window_order.npz"), {"SAMRS_WIN_DENSE": "0"})
    assert sorted(dense.files) == sorted(plain.files) and len(dense.files) == len(PRECS) * len(HEADS) * len(GRIDS)
    for k in dense.files:
        assert dense[k].tobytes() == plain[k].tobytes(), f"{k}: the two query numberings differ"


if __name__ == "__main__":
    _child(sys.argv[1])

"""Generic kernels above 64 KiB of dynamic LDS: the only regime in which the library's ensure_dyn_lds (e3_common.h) acts.

Shape: lmax_sh = 1, in1 = out = 256x0e + 256x1o (D1 = Dout = 1024, Dy = 4), B = 33.  LDS of the launches, from the launchers'
own formulas (R rows per block, A = accumulate type); each must lie above 64 KiB and within the 160 KiB the launchers refuse at:
  SHTensorProduct fp64   forward   R = 16: 16 (D1 + Dy) 8             = 131 584 B   (two full tiles + one row)
                         rows bwd  R = 4:  4 (2 D1 + Dy + Dout + 9) 8 =  98 720 B   (eight tiles + one row)
                         weights   R = 8:  8 (D1 + Dy + Dout) 8       = 131 328 B
  L1TensorProduct fp64   forward   R = 16: 16 (D1 + 4) 8              = 131 584 B
                         backward  R = 16: 16 (D1 + Dout + 4) 8       = 262 656 B: above 160 KiB, refused -- not run
  L1TensorProduct fp32   forward   (generic kernel forced)            =  65 792 B
                         rows / weights backward 16 (D1 + Dout + 4) 4 = 131 328 B
Elsewhere in the suite only tp_fwd_generic_kernel<float> gets there (tests/test_tp_r16_table_gpu.py runs the exact fp32 forward
of message product #1 and update #1 at hidden 64, l_max 2: 16 (1153 + 9) 4 = 74 368 B), so there is no fp32 SHTensorProduct case.

Order: large plan, small plan (hidden 16, under 64 KiB: no attribute call), large plan again, in one process.  Every result
meets the fp64 oracle at the bounds of tests/test_tp_backward_gpu.py and the two large results are bit-equal where the kernel
has a fixed summation order (out, grad_in1).  No threads: this covers the path, it does not try to provoke a race."""
import pytest
import torch

import models  # noqa: F401
from models.segnn.l1_tensor_prod import L1TensorProduct
from oracle import tp_oracle as T
from scalable_e3_gnn_amd import Irreps
from scalable_e3_gnn_amd.tensor_product import SHTensorProduct

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 33
LARGE, SMALL = "256x0e+256x1o", "16x0e+16x1o"
D1 = Dout = 4 * 256
Dy = 4
KiB = 1024
LDS = {"sh64 forward": 16 * (D1 + Dy) * 8, "sh64 rows": 4 * (2 * D1 + Dy + Dout + 9) * 8, "sh64 weights": 8 * (D1 + Dy + Dout) * 8,
       "l1 fp64 forward": 16 * (D1 + 4) * 8, "l1 fp32 forward": 16 * (D1 + 4) * 4, "l1 fp32 backward": 16 * (D1 + Dout + 4) * 4}


def test_lds_sizes_are_in_the_regime():
    assert LDS["sh64 forward"] == 131584 and LDS["sh64 rows"] == 98720
    for name, b in LDS.items():
        assert 64 * KiB < b <= 160 * KiB, (name, b)
    assert 16 * (D1 + Dout + 4) * 8 > 160 * KiB   # the fp64 L1 backward is refused at this shape


def rel(a, b):
    return float((a.double().cpu() - b.double()).abs().max() / b.double().abs().max())


def oracle_grads(mod, irreps, x, y, gout):
    """oracle/tp_oracle.forward_torch_cpu in fp64 on the module's own weights and norms (either module class) and the inputs
    promoted to fp64, and autograd over it"""
    W = {c: getattr(mod, "weights_" + c).detach().cpu().double().requires_grad_(True) for c in T.CLASSES
         if hasattr(mod, "weights_" + c)}
    N = {c: getattr(mod, "norm_" + c).detach().cpu().double() for c in T.CLASSES if hasattr(mod, "norm_" + c)}
    xc, yc = x.clone().double().requires_grad_(True), y.clone().double().requires_grad_(True)
    out = T.forward_torch_cpu(irreps, irreps, 1, xc, yc, W, N)
    out.backward(gout.double())
    return out.detach(), xc.grad, yc.grad, {c: W[c].grad for c in W}


def run(mod, irreps, dt, backward, seed):
    """forward (+ rows / weights backward) of `mod` against the oracle -> (out, grad_in1) for the bit comparison"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, mod.in1_dim, generator=g, dtype=dt)
    y = torch.randn(B, 4, generator=g, dtype=dt)
    gout = torch.randn(B, mod.in1_dim, generator=g, dtype=dt)   # out irreps = in1 irreps
    want_out, want_gx, want_gy, want_gw = oracle_grads(mod, irreps, x, y, gout)
    f64 = dt == torch.float64
    tol = 1e-11 if f64 else 2e-5
    xd, yd = x.to(DEV).requires_grad_(backward), y.to(DEV).requires_grad_(backward)
    for p in mod.parameters():
        p.grad = None
        p.requires_grad_(backward)
    out = mod(xd, yd)
    assert rel(out.detach(), want_out) < (1e-12 if f64 else 1e-5)
    if not backward:
        return out.detach().clone(), None
    out.backward(gout.to(DEV))
    assert rel(xd.grad, want_gx) < tol and rel(yd.grad, want_gy) < tol
    for c, gw in want_gw.items():
        assert rel(getattr(mod, "weights_" + c).grad, gw) < tol, c
    return out.detach().clone(), xd.grad.clone()


@pytest.mark.parametrize("case", ["sh fp64", "l1 fp64 forward", "l1 fp32"])
def test_large_small_large(case, monkeypatch):
    from scalable_e3_gnn_amd import tensor_product as TPM
    monkeypatch.setattr(TPM, "_BWD_GEMM_MIN_ROWS", 1 << 30)   # the rows / weights kernels whatever B
    dt = torch.float32 if "fp32" in case else torch.float64
    backward = "forward" not in case
    torch.manual_seed(0)
    mods = {}
    for irreps in (LARGE, SMALL):
        ir = Irreps(irreps)
        m = (SHTensorProduct(ir, ir, 1) if case.startswith("sh") else L1TensorProduct(ir, ir)).to(dt).to(DEV)
        if dt == torch.float32:
            m.kernel = 1   # generic forward (the default would be the MFMA kernel)
        mods[irreps] = m
    first = run(mods[LARGE], LARGE, dt, backward, 1)
    run(mods[SMALL], SMALL, dt, backward, 2)
    again = run(mods[LARGE], LARGE, dt, backward, 1)
    assert torch.equal(first[0], again[0])
    if backward:
        assert torch.equal(first[1], again[1])

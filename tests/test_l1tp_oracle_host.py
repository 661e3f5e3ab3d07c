"""The references of tests/test_l1tp_table_gpu.py checked on the host.

* bwd_cases.oracle_autograd (fp64 autograd over oracle/tp_oracle.forward_torch_cpu), fed the state dict, inputs and grad_out of
  every golden case of the reference, reproduces the reference's own out, grad_in1, grad_in2 and every grad_weights_*: 1e-12
  relative to scale for the fp64 cases, 1e-5 for the fp32 cases, 2e-2 for bf16_module (the reference rounds every intermediate
  to bf16).  Measured: fp64 <= 1.3e-15, fp32 <= 5.0e-7, bf16_module 5.8e-3.  empty_batch is left out: the oracle cannot reshape
  B = 0.
* The blocks of tests/l1tp_cases.py tile every in1 column, every out column and every row of every weight matrix of p0-p6.
* The seeded norm overwrite leaves pairwise distinct values inside each class, in [0.5, 1.5], exact in bf16.
* The refusals of e3_l1tp_forward / e3_l1tp_backward that need no device (they are decided before the first HIP call)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import bwd_cases as C
import l1tp_cases as L
from conftest import GOLDEN, load_case
from oracle import l1tp_oracle as O

META = json.load(open(os.path.join(GOLDEN, "l1tp_meta.json")))["cases"]
TOL = {"float64": 1e-12, "float32": 1e-5, "bfloat16": 2e-2}
LEFT_OUT = ("empty_batch",)


def test_only_the_empty_batch_is_left_out():
    assert len(META) == 19 and [n for n in META if META[n]["B"] == 0] == list(LEFT_OUT)


@pytest.mark.parametrize("name", sorted(n for n in META if n not in LEFT_OUT))
def test_backward_oracle_reproduces_reference_golden(name):
    c, z = META[name], load_case(name)
    W = {k: z["sd_weights_" + k] for k in O.CLASSES if "sd_weights_" + k in z.files}
    N = {k: z["sd_norm_" + k] for k in O.CLASSES}
    x, y, go = (torch.as_tensor(np.asarray(z[k], np.float64)) for k in ("in1", "in2", "grad_out"))
    out, gx, gy, gw = C.oracle_autograd(c["in1"], c["out"] or c["in1"], 1, W, N, x, y, go)
    pairs = [("out", out, z["out"]), ("grad_in1", gx, z["grad_in1"]), ("grad_in2", gy, z["grad_in2"])]
    pairs += [("grad_weights_" + k, gw[k], z["grad_weights_" + k]) for k in W]
    assert sorted(k for k in z.files if k.startswith("grad_weights_")) == sorted("grad_weights_" + k for k in W)
    for what, got, want in pairs:
        got, want = got.numpy(), np.asarray(want, np.float64)
        assert got.shape == want.shape, (what, got.shape, want.shape)
        err = float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))
        print(f"{name} {c['dtype']} {what}: {err:.2e}")
        assert err <= TOL[c["dtype"]], (name, what, err)


@pytest.mark.parametrize("pid", sorted(L.PLANS))
def test_blocks_tile_columns_and_weight_rows(pid):
    in1, out = L.PLANS[pid]
    lay = O.make_layout(in1, out)
    for blocks, dim in ((C.in1_blocks(in1), lay.in1_dim), (L.out_blocks(pid), lay.out_dim)):
        col = 0
        for n, s in blocks:
            assert s.start == col and s.stop > s.start, (n, s)
            col = s.stop
        assert col == dim and len({n for n, _ in blocks}) == len(blocks)
    seen = 0
    for c in O.CLASSES:
        blocks = L.weight_blocks(pid, c)
        if lay.wshape[c] is None:
            continue
        seen += 1
        row = 0
        for n, s in blocks:
            assert s.start == row and s.stop > s.start, (c, n, s)
            row = s.stop
        assert row == lay.wshape[c][0], (c, row, lay.wshape[c])
        assert len({n for n, _ in blocks}) == len(blocks)
        assert tuple(getattr(L.host_module(pid), "weights_" + c).shape) == lay.wshape[c]
    assert seen == sum(hasattr(L.host_module(pid), "weights_" + c) for c in O.CLASSES) >= 2


@pytest.mark.parametrize("pid", sorted(L.PLANS))
def test_seeded_norms_are_distinct_inside_each_class(pid):
    mod = L.host_module(pid)
    lay = O.make_layout(*L.PLANS[pid])
    ctor = O.normalisation(*L.PLANS[pid]).norms
    for c in O.CLASSES:
        n = getattr(mod, "norm_" + c)
        assert n.numel() == len(lay.o[c]) == len(ctor[c])
        if n.numel() == 0:
            continue
        assert len(set(n.tolist())) == n.numel(), c
        assert float(n.min()) >= 0.5 and float(n.max()) <= 1.5
        assert torch.equal(n.bfloat16().float(), n), c          # every storage type holds the same norms
        assert not np.array_equal(n.numpy(), ctor[c]), c         # the constructor's (constant per irreps block) are gone
    W, N = L.weights_norms(pid, rounded=True)
    assert all(np.array_equal(N[c], getattr(mod, "norm_" + c).double().numpy()) for c in O.CLASSES)


def test_plan_thresholds_the_cases_rely_on():
    """B_WRAP is past the second tile of every wave of the MFMA forward at its caps (256 blocks, 8 waves, 32 rows) and wraps the
    2048-tile grid of the 16-row kernels twice with a ragged last tile in both tilings"""
    assert L.B_WRAP == 256 * 8 * 32 + 37 and L.B_WRAP % 32 == 5 and L.B_WRAP % 16 == 5
    assert (L.B_WRAP + 15) // 16 > 2 * 2048
    assert L.B_WRAP > 65536           # the column sum's 256 blocks x 256 rows


# ---- refusals decided on the host ----
def test_stride_refusals_need_no_device():
    """ld_out < Dout, ld_in2 in {1, 2, 3} (forward and backward) and ld_gin1 < D1 answer E3_ERR_INVALID_ARG before any HIP call:
    host buffers stand in for the operands and stay untouched"""
    from scalable_e3_gnn_amd import _lib
    lib = _lib.load()
    mod = L.host_module("p0")
    h = mod._get_plan().handle(None)
    D1, Dout, B = mod.in1_dim, mod.iro.dim, 5
    assert lib.e3_l1tp_in1_dim(h) == D1 and lib.e3_l1tp_out_dim(h) == Dout
    x, y, go = np.zeros((B, D1), np.float32), np.zeros((B, 4), np.float32), np.zeros((B, Dout), np.float32)
    packed, work = np.zeros(1 << 16, np.uint8), np.zeros(1 << 16, np.uint8)
    out = np.full((B, Dout), L.SENTINEL, np.float32)
    gin1, gin2 = np.full((B, D1), L.SENTINEL, np.float32), np.full((B, 4), L.SENTINEL, np.float32)
    ws = [w.detach().numpy() if w is not None else None for w in mod._weights()]
    p = lambda a: a.ctypes.data
    P4 = ctypes.c_void_p * 4
    wp = P4(*[p(w) if w is not None else None for w in ws])
    none4 = P4(None, None, None, None)
    for dtype in (0, 1, 2):
        for kernel in (0, 1, 2):
            assert lib.e3_l1tp_forward(h, p(x), D1, p(y), 4, p(packed), p(out), Dout - 1, B, dtype, kernel, None) == 1
            for ld2 in (1, 2, 3, -4):
                assert lib.e3_l1tp_forward(h, p(x), D1, p(y), ld2, p(packed), p(out), Dout, B, dtype, kernel, None) == 1
        assert lib.e3_l1tp_backward(h, p(x), D1, p(y), 4, wp, none4, p(go), Dout, p(gin1), D1 - 1, p(gin2), none4, p(work), B,
                                    dtype, None) == 1
        assert lib.e3_l1tp_backward(h, p(x), D1, p(y), 4, wp, none4, p(go), Dout - 1, p(gin1), D1, p(gin2), none4, p(work), B,
                                    dtype, None) == 1
        for ld2 in (1, 2, 3, -4):
            assert lib.e3_l1tp_backward(h, p(x), D1, p(y), ld2, wp, none4, p(go), Dout, p(gin1), D1, p(gin2), none4, p(work), B,
                                        dtype, None) == 1, ld2
    assert (out == L.SENTINEL).all() and (gin1 == L.SENTINEL).all() and (gin2 == L.SENTINEL).all()

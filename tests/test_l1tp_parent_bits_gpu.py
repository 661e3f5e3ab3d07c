"""The pinned operator's own kernels (csrc/e3_l1tp*.hip) give THE SAME BITS as the commit before their class table, W-mix
helpers and plan header were introduced: where the text of a kernel lives may change, the sequence of operations on every
accumulator may not.

Four plans, the smallest on which each branch of the class table can go wrong, at B = 33 (two full 16-row tiles plus one
row; one 32-row MFMA tile plus one row):
  p0  all four classes on both sides, odd counts (the odd tail of the MFMA runs)
  p1  absent input classes: the 1o output has only its cross slot
  p2  interleaved blocks, several runs per class
  p3  an output class wider than one 32-channel MFMA tile; more weights than one 2048-element chunk of the dW kernel
Per plan: the generic forward (kernel = 1) in fp32 / fp64 / bf16, the MFMA forward (kernel = 2) in fp32, the packed weight
buffer per dtype (packed into a buffer pre-filled with 0xA5, so the bytes no kernel writes are compared as well), and
e3_l1tp_backward (grad_in1, grad_in2, every grad_W) per dtype, once with per-row in2 and once with in2 of shape [1, 4] (the
two-stage column sum).  All of these launches sum in a fixed order.  The SHA-256 of the raw bytes is compared
with the digest recorded from the parent commit on an MI355X (tests/golden/l1tp_parent_digests.json, written by
tests/golden/make_l1tp_digests.py).  Inputs are seeded on the CPU, weights come from the constructor under
torch.manual_seed."""
import contextlib
import hashlib
import json
import os

import pytest
import torch

from models.segnn.l1_tensor_prod import L1TensorProduct
from scalable_e3_gnn_amd import Irreps, _lib
from scalable_e3_gnn_amd.l1_tensor_prod import _CLS
from scalable_e3_gnn_amd import tensor_product as TPM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 33
PLANS = (
    ("5x0e+3x0o+7x1o+2x1e", "9x0e+1x0o+4x1e+6x1o"),
    ("3x1e", "2x0o+2x1e+3x1o"),
    ("2x1o+3x0e+1x1e+2x0e+2x1o+1x0o", "1x1e+2x0e+2x1o+1x0o+3x1o+2x0e"),
    ("40x0e+40x1o", "40x0e+40x1o"),
)
DTYPES = {"fp32": torch.float32, "fp64": torch.float64, "bf16": torch.bfloat16}
IN2 = ("rows", "bcast")   # in2 [B, 4] / [1, 4]
DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "l1tp_parent_digests.json")


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def module(i, dtype):
    torch.manual_seed(100 + i)
    return L1TensorProduct(Irreps(PLANS[i][0]), Irreps(PLANS[i][1])).to(dtype).to(DEV)


def inputs(i, mod, dtype):
    g = torch.Generator().manual_seed(200 + i)
    x = torch.randn(B, mod.in1_dim, generator=g)
    y = torch.randn(B, 4, generator=g)
    go = torch.randn(B, mod.iro.dim, generator=g)
    return tuple(t.to(dtype).to(DEV) for t in (x, y, go))


@contextlib.contextmanager
def own_backward():
    """every backward through e3_l1tp_backward, whatever B"""
    old = TPM._BWD_GEMM_MIN_ROWS
    TPM._BWD_GEMM_MIN_ROWS = 1 << 30
    try:
        yield
    finally:
        TPM._BWD_GEMM_MIN_ROWS = old


def packed_bytes(mod, dtype):
    """e3_l1tp_pack_weights into a buffer of e3_l1tp_packed_bytes pre-filled with 0xA5"""
    lib, code = _lib.load(), _lib.dtype_code(dtype)
    with torch.cuda.device(DEV):
        h = mod._get_plan().handle(torch.device(DEV))
        buf = torch.full((int(lib.e3_l1tp_packed_bytes(h, code)),), 0xA5, dtype=torch.uint8, device=DEV)
        ws = [w.detach().contiguous() if w is not None else None for w in mod._weights()]
        ns = [n.detach().contiguous() if n is not None else None for n in mod._norms()]
        _lib.call("e3_l1tp_pack_weights", h, _lib.ptr4(ws), _lib.ptr4(ns), code, buf.data_ptr(),
                  torch.cuda.current_stream(DEV).cuda_stream)
        torch.cuda.synchronize()
    return buf


def plan_digests(i):
    """{key: digest} of everything recorded for plan i"""
    out = {}
    for name, dtype in DTYPES.items():
        mod = module(i, dtype)
        x, y, go = inputs(i, mod, dtype)
        with torch.no_grad():
            for kernel in ((1, 2) if name == "fp32" else (1,)):
                mod.kernel = kernel
                got = mod(x, y)
                assert got.dtype == dtype and tuple(got.shape) == (B, mod.iro.dim)
                out[f"p{i}-fwd-k{kernel}-{name}"] = digest(got)
            out[f"p{i}-packed-{name}"] = digest(packed_bytes(mod, dtype))
            with own_backward():
                for how in IN2:
                    yy = y if how == "rows" else y[:1].contiguous()
                    g1, g2, gw = mod._hip_backward(x, yy, go, True, True, True)
                    assert g1.shape == x.shape and g2.shape == yy.shape
                    out[f"p{i}-bwd-{name}-{how}-grad_in1"] = digest(g1)
                    out[f"p{i}-bwd-{name}-{how}-grad_in2"] = digest(g2)
                    for c, w in zip(_CLS, mod._weights()):
                        assert (gw[c] is None) == (w is None), c
                        if w is not None:
                            out[f"p{i}-bwd-{name}-{how}-grad_W{c}"] = digest(gw[c])
    return out


def all_digests():
    """what make_l1tp_digests.py records"""
    out = {}
    for i in range(len(PLANS)):
        out.update(plan_digests(i))
    return out


def recorded():
    with open(DIGESTS) as f:
        return json.load(f)["digests"]


@pytest.mark.parametrize("i", range(len(PLANS)), ids=[f"p{i}" for i in range(len(PLANS))])
def test_same_bits_as_the_parent(i):
    want = {k: v for k, v in recorded().items() if k.startswith(f"p{i}-")}
    got = plan_digests(i)
    for k in sorted(got):
        print(f"L1TP {k}: {got[k]}")
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    # 4 forwards, 3 packed buffers and 3 dtypes x 2 forms of in2 x (grad_in1, grad_in2, one grad_W per weight) each
    nw = sum(w is not None for w in module(i, torch.float32)._weights())
    assert len(got) == 4 + 3 + 3 * 2 * (2 + nw)
    bad = [k for k in sorted(got) if got[k] != want[k]]
    assert not bad, bad


def test_no_key_outside_the_plans():
    assert all(k.split("-")[0] in {f"p{i}" for i in range(len(PLANS))} for k in recorded())

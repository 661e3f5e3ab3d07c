"""Helpers of tests/test_tp_backward_table_gpu.py and tests/test_tp_backward_oracle_host.py: the fp64 autograd reference of one
tensor product (oracle/tp_oracle.forward_torch_cpu), the blocks the error is taken over (in1 irreps blocks, in2 degrees, the
weight rows of every path) and the four ways a module's backward is driven.  The products, their plans and their weights come
from tests/r16_cases.py.  TEST INFRASTRUCTURE ONLY."""
import contextlib
import functools

import numpy as np
import torch

import r16_cases as R
from oracle import tp_oracle as T
from oracle.l1tp_oracle import parse_blocks

DEV = R.DEV
BOUND = {"fp32": 2e-5, "fp64": 1e-11}            # the bounds of tests/test_tp_backward_gpu.py, here per block
FWD_BOUND = {"fp32": 1e-5, "fp64": 1e-12}        # its forward bounds (whole output)
TORCH_DTYPE = {"fp32": torch.float32, "fp64": torch.float64}
SYNTHETIC = ("128x0e+128x1o", "128x1o", 1)       # K = 256, M = 128: 32 output tiles of the fused weight gradient
PATHS = ("rows", "gemm", "wgrad", "wgrad_gemm", "dual")


# ---- irreps of the products without a device (the host test and the block helpers) ----
def hid(H, lmax):
    return f"{H}x0e+{H}x1o" + (f"+{H}x2e" if lmax == 2 else "")


def gated(H, lmax):
    return f"{H}x0e+{lmax * H}x0e+{H}x1o" + (f"+{H}x2e" if lmax == 2 else "")


def product_irreps(name, H, lmax):
    """(in1 irreps, out irreps) of the six products a SEGNN(1x0e+1x1o, H, 1x1o, l_max) builds"""
    h, g = hid(H, lmax), gated(H, lmax)
    return {"embed": ("1x0e+1x1o", h), "msg1": (h + "+" + h + "+1x0e", g), "msg2": (h, g), "upd1": (h + "+" + h, g),
            "upd2": (h, h), "readout": (h, "1x1o")}[name]


def irreps_dim(irreps):
    return sum((2 * l + 1) * m for l, _, m in parse_blocks(irreps))


# ---- blocks ----
def in1_blocks(in1_irreps):
    """[(name, column slice)]: every contiguous irreps block of in1 as written (equal irreps are not merged)"""
    out, c = [], 0
    for i, (l, p, mul) in enumerate(parse_blocks(str(in1_irreps))):
        w = (2 * l + 1) * mul
        out.append((f"in1[{i}]:{mul}x{l}{'e' if p == 1 else 'o'}", slice(c, c + w)))
        c += w
    return out


def in2_blocks(lmax_sh):
    return [(f"in2:l{l}", slice(l * l, (l + 1) * (l + 1))) for l in range(lmax_sh + 1)]


def path_row_blocks(in1_irreps, lmax_sh, c3):
    """[(name, row slice)] of the weight matrix of output class c3.  The paths follow tp_oracle.paths, n_in[c1] rows each; inside a
    path the rows are the channels of class c1 in order of appearance, so each path is cut once more at the in1 irreps blocks it
    draws from (message product #1: first hidden copy, second hidden copy, and in the scalar paths the single distance row)."""
    blocks = parse_blocks(str(in1_irreps))
    ic = T.class_columns(blocks)
    n_in = {c: len(ic[c]) for c in range(6)}
    out, row = [], 0
    for c1, l1, l2 in T.paths(c3, n_in, lmax_sh):
        for i, (l, p, mul) in enumerate(blocks):
            if T.cls_of(l, p) == c1:
                out.append((f"W_{T.CLASSES[c3]}[{T.CLASSES[c1]} x Y{l2}]/in1[{i}]", slice(row, row + mul)))
                row += mul
    return out


def block_errors(got, want, blocks, axis=1):
    """per block: max |got - want| / max |want| over the block (columns for axis = 1, rows for axis = 0)"""
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    want = want.detach().double().cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    res = []
    for n, s in blocks:
        g, w = (got[:, s], want[:, s]) if axis == 1 else (got[s], want[s])
        assert w.size > 0, n
        res.append((n, float(np.abs(g - w).max() / max(np.abs(w).max(), 1e-300))))
    return res


# ---- modules ----
@functools.lru_cache(maxsize=None)
def module(key, dtype="fp32"):
    """key = (product, H, l_max) of a model or ("synthetic",); the fp64 module is a copy with the same (fp32-valued) parameters"""
    if dtype == "fp64":
        src = module(key)
        new = type(src)(src.iri1, src.iro) if is_l1tp(src) else type(src)(src.iri1, src.iro, src.lmax_sh)
        new.load_state_dict(src.state_dict())
        return new.double().to(DEV)
    if key[0] == "synthetic":
        from scalable_e3_gnn_amd.tensor_product import SHTensorProduct
        torch.manual_seed(77)
        return SHTensorProduct(*SYNTHETIC).to(DEV)
    return R.product(key[0], key[1], key[2], "fp32")


def lmax_sh_of(mod):
    return int(round(mod.in2_dim ** 0.5)) - 1


def classes_of(mod):
    return [c for c in T.CLASSES if hasattr(mod, "weights_" + c)]


def is_l1tp(mod):
    return hasattr(mod, "_hip_backward")


def paths_of(mod):
    return PATHS if is_l1tp(mod) else PATHS[:4]


# ---- reference ----
class Ref:
    """x [B, D1], y [B or 1, Dy], gout [B, Dout] (fp32, drawn on the host) and the oracle's fp64 out, gx, gy, gw[class]"""


def oracle_autograd(in1_irreps, out_irreps, lmax_sh, W, N, x, y, gout):
    """forward_torch_cpu under autograd in fp64 -> out, grad x, grad y (shape of y), {class: grad W}"""
    dtype = torch.float64
    Wt = {c: torch.as_tensor(w).to(dtype).requires_grad_(True) for c, w in W.items()}
    Nt = {c: torch.as_tensor(n).to(dtype) for c, n in N.items()}
    xc, yc = x.to(dtype).requires_grad_(True), y.to(dtype).requires_grad_(True)
    B = xc.shape[0]
    out = T.forward_torch_cpu(str(in1_irreps), str(out_irreps), lmax_sh, xc, yc if yc.shape[0] == B else yc.expand(B, -1), Wt, Nt)
    out.backward(gout.to(dtype))
    return out.detach(), xc.grad, yc.grad, {c: Wt[c].grad for c in Wt}


def draw(mod, B, seed, bcast=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, mod.in1_dim, generator=g)
    y = torch.randn(1 if bcast else B, mod.in2_dim, generator=g)
    gout = torch.randn(B, irreps_dim(str(mod.iro)), generator=g)
    return x, y, gout


@functools.lru_cache(maxsize=None)
def reference(key, B, seed, bcast=False):
    """One evaluation per (product, H, l_max, B, seed): every path and both storage types of a case compare with it.  The cache
    is unbounded; a test with a large B empties it when it is done (``reference.cache_clear()``)."""
    mod = module(key)
    r = Ref()
    r.x, r.y, r.gout = draw(mod, B, seed, bcast)
    W, N = R.weights_norms(mod)
    r.out, r.gx, r.gy, r.gw = oracle_autograd(mod.iri1, mod.iro, lmax_sh_of(mod), W, N, r.x, r.y, r.gout)
    return r


# ---- driving a module's backward ----
@contextlib.contextmanager
def requesting(mod, classes):
    """Only the weights of ``classes`` require grad inside the block; afterwards every parameter does again and holds no grad."""
    try:
        for c in classes_of(mod):
            p = getattr(mod, "weights_" + c)
            p.requires_grad_(c in classes)
            p.grad = None
        yield
    finally:
        for p in mod.parameters():
            p.requires_grad_(True)
            p.grad = None


def spy_fused_wgrad(monkeypatch):
    """-> list that receives the status of every e3_tp_backward_weights call made from now on (0 = the fused kernels ran, 4 =
    refused: the caller takes the GEMM path); what a module call really did is read here, not predicted"""
    from scalable_e3_gnn_amd import _lib
    lib = _lib.load()
    real, seen = lib.e3_tp_backward_weights, []

    def spy(*args):
        st = real(*args)
        seen.append(st)
        return st
    monkeypatch.setattr(lib, "e3_tp_backward_weights", spy)
    return seen


def configure(monkeypatch, path):
    from scalable_e3_gnn_amd import tensor_product as TPM
    monkeypatch.setattr(TPM, "_BWD_GEMM_MIN_ROWS", 1 << 30 if path == "rows" else 0)
    monkeypatch.setattr(TPM, "_BWD_FUSED_WGRAD", path != "wgrad_gemm")


def wanted(path, mod):
    """(in1, in2, weight classes) that ask for a gradient on ``path``"""
    allc = tuple(classes_of(mod))
    return {"rows": (True, True, allc), "gemm": (True, True, allc), "wgrad": (False, False, allc),
            "wgrad_gemm": (False, False, allc), "dual": (True, False, allc)}[path]


class Got:
    pass


def run(mod, x, y, gout, need1, need2, classes):
    """forward + backward through module autograd on device tensors (used as given: strides and alignment are the caller's)"""
    with requesting(mod, classes):
        xd = x.detach().requires_grad_(True) if need1 else x.detach()
        yd = y.detach().requires_grad_(True) if need2 else y.detach()
        out = mod(xd, yd)
        out.backward(gout)
        g = Got()
        g.out, g.gx, g.gy = out.detach(), xd.grad, yd.grad
        g.gw = {c: getattr(mod, "weights_" + c).grad for c in classes_of(mod)}
        for c in classes_of(mod):
            assert (g.gw[c] is not None) == (c in classes), c
    return g


def run_spied(monkeypatch, mod, x, y, gout, need1, need2, classes):
    """``run`` -> Got whose ``wgrad_status`` holds what e3_tp_backward_weights answered during the call ([] = not called)"""
    seen = getattr(monkeypatch, "_wgrad_seen", None)
    if seen is None:
        seen = monkeypatch._wgrad_seen = spy_fused_wgrad(monkeypatch)
    del seen[:]
    got = run(mod, x, y, gout, need1, need2, classes)
    got.wgrad_status = list(seen)
    return got


def run_path(mod, ref, path, monkeypatch, dtype="fp32", classes=None, need=None):
    configure(monkeypatch, path)
    dt = TORCH_DTYPE[dtype]
    n1, n2, cl = wanted(path, mod)
    if need is not None:
        n1, n2 = need
    if classes is not None:
        cl = classes
    return run_spied(monkeypatch, mod, ref.x.to(dt).to(DEV), ref.y.to(dt).to(DEV), ref.gout.to(dt).to(DEV), n1, n2, cl)


def errors(mod, got, ref):
    """[(block name, error)] of every gradient ``got`` holds, per block; the forward output as one block "out"."""
    errs = block_errors(got.out, ref.out, [("out", slice(None))])
    lm = lmax_sh_of(mod)
    if got.gx is not None:
        errs += block_errors(got.gx, ref.gx, in1_blocks(mod.iri1))
    if got.gy is not None:
        assert tuple(got.gy.shape) == tuple(ref.gy.shape), (got.gy.shape, ref.gy.shape)
        errs += block_errors(got.gy, ref.gy, in2_blocks(lm))
    for c, gw in got.gw.items():
        if gw is not None:
            c3 = T.CLASSES.index(c)
            errs += block_errors(gw, ref.gw[c], path_row_blocks(mod.iri1, lm, c3), axis=0)
    return errs

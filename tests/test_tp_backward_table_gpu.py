"""Every backward path of the tensor products a SEGNN builds (csrc/e3_tp.hip, csrc/e3_l1tp_bwd.hip, tensor_product.tp_backward,
L1TensorProduct._hip_backward), one product at a time, against fp64 torch autograd over oracle/tp_oracle.forward_torch_cpu on the
product's own weights and norms and the fp32 inputs promoted to fp64 (helpers: tests/bwd_cases.py, products: tests/r16_cases.py).

The error is taken PER BLOCK, max |got - want| over the block / max |want| over the block: grad_in1 per contiguous irreps block of
in1 (message product #1: the blocks of both hidden copies and the 1-column distance channel), grad_in2 per degree, grad_W per path
(the rows of one path of tp_oracle.paths, cut once more at the in1 irreps blocks they come from).  Bounds: 2e-5 (fp32) and
1e-11 (fp64), the whole-tensor bounds of tests/test_tp_backward_gpu.py; the forward output is asserted with that file's forward bounds.

Paths (``tensor_product._BWD_GEMM_MIN_ROWS`` / ``_BWD_FUSED_WGRAD`` monkeypatched):
  rows        threshold 1 << 30, everything wanted: e3_tp_backward (SHTensorProduct) / e3_l1tp_backward (L1TensorProduct = every
              l_max = 1 product)
  gemm        threshold 0, everything wanted: operands -> library GEMMs -> contract
  wgrad       threshold 0, only parameters: e3_tp_backward_weights, or the GEMM path where that call answers "unsupported".
              What the call answered is read by a spy on the library entry (bwd_cases.spy_fused_wgrad), asserted against the
              pinned table, and every figure is filed under "[fused]" or "[refused -> gemm]" accordingly
  wgrad_gemm  the same with _BWD_FUSED_WGRAD = False
  dual        L1TensorProduct only: threshold 0, in1 and parameters: the dual forward + the weight-gradient call
Every figure of a failing block is printed; the worst block per (path, dtype) is printed when the module ends."""
import ctypes

import pytest
import torch

import bwd_cases as C
import models  # noqa: F401
import r16_cases as R
from bwd_cases import BOUND, DEV, FWD_BOUND
from oracle import tp_oracle as T
from r16_cases import HIDDEN, LMAX, PRODUCTS

pytestmark = pytest.mark.gpu

ALL = [(p, H, l) for p in PRODUCTS for H in HIDDEN for l in LMAX]
# what e3_tp_backward_weights answers with every class requested (0 = E3_OK, 4 = E3_ERR_UNSUPPORTED: the caller falls back as a
# whole).  Unsupported: message #1 at hidden 64 (l_max 1: class l0e has K 257 x M 128 = 36 tiles; l_max 2: every class), message
# #2 at hidden 64, l_max 2 (l0e, 36 tiles) and update #1 at hidden 64, l_max 2 (every class)
WGRAD_STATUS = {k: 0 for k in ALL}
WGRAD_STATUS.update({("msg1", 64, 1): 4, ("msg1", 64, 2): 4, ("msg2", 64, 2): 4, ("upd1", 64, 2): 4})

_WORST = {}    # (path, dtype) -> (error, block, case id)


@pytest.fixture(scope="module", autouse=True)
def _print_worst():
    yield
    print("\nworst block per (path, dtype):")
    for (path, dtype), (e, blk, cid) in sorted(_WORST.items()):
        print(f"  {path:26s} {dtype}  {e:.2e}  {blk}  [{cid}]")


def _note(path, dtype, e, blk, cid):
    if e > _WORST.get((path, dtype), (-1.0,))[0]:
        _WORST[(path, dtype)] = (e, blk, cid)


def _check(mod, got, ref, dtype, path, cid, fails):
    """every block of every gradient ``got`` holds against its bound; misses are appended to ``fails`` (asserted by the caller
    once all cases of the test have been measured)"""
    st = got.wgrad_status
    assert st in ([], [0], [4]), st
    if st:   # the call went to e3_tp_backward_weights: file the figure under what that call really did
        path += " [fused]" if st == [0] else " [refused -> gemm]"
    for blk, e in C.errors(mod, got, ref):
        bound = FWD_BOUND[dtype] if blk == "out" else BOUND[dtype]
        if blk != "out":
            _note(path, dtype, e, blk, cid)
        if not e < bound:
            print(f"MISS {cid} {path} {dtype} {blk}: {e:.3e} (bound {bound:.0e})")
            fails.append((cid, path, dtype, blk, e))


def _run_all_paths(key, B, seed, monkeypatch, fails, dtypes=("fp32",), paths=None, cid=None):
    ref = C.reference(key, B, seed)
    cid = cid or f"{'-'.join(map(str, key))}-B{B}"
    for dtype in dtypes:
        mod = C.module(key, dtype)
        for path in (paths or C.paths_of(mod)):
            if dtype == "fp64" and path not in ("rows", "gemm"):
                continue
            if path == "dual" and not C.is_l1tp(mod):
                continue
            got = C.run_path(mod, ref, path, monkeypatch, dtype)
            if path in ("wgrad", "dual"):   # every class is requested: the module meets the kernel's own answer
                assert got.wgrad_status == [WGRAD_STATUS[key]], (key, path, got.wgrad_status)
            else:
                assert got.wgrad_status == [], (key, path, got.wgrad_status)
            _check(mod, got, ref, dtype, path, cid, fails)


def _wgrad_direct(key, B, seed, classes=None):
    """lib.e3_tp_backward_weights on the product's plan and packed weights -> (status, [grad_W buffer | None] * 6, ref)"""
    from scalable_e3_gnn_amd import _lib
    mod = C.module(key)
    plan, ws, ns = R.plan_of(mod)
    ws, ns = list(ws), list(ns)
    ref = C.reference(key, B, seed)
    x, y, go = ref.x.to(DEV), ref.y.to(DEV), ref.gout.to(DEV)
    dev = x.device
    with torch.cuda.device(dev):
        packed = plan.packed(ws, ns, torch.float32, dev)
        gws = [torch.zeros(w.shape, dtype=torch.float32, device=dev)
               if (w is not None and (classes is None or T.CLASSES[c] in classes)) else None for c, w in enumerate(ws)]
        P6 = ctypes.c_void_p * 6
        st = _lib.load().e3_tp_backward_weights(plan.handle(dev), x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0),
                                                packed.data_ptr(), go.data_ptr(), go.stride(0),
                                                P6(*[g.data_ptr() if g is not None else None for g in gws]), B, 0,
                                                torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
    return st, gws, ref


# ---- 1. the table ----
@pytest.mark.parametrize("lmax", LMAX)
@pytest.mark.parametrize("H", HIDDEN)
def test_table_every_product_every_path(H, lmax, monkeypatch):
    """six products x every applicable path, fp32, B = 137; fp64 on rows and gemm at hidden 16 / 32"""
    fails = []
    for name in PRODUCTS:
        mod = C.module((name, H, lmax))
        assert C.is_l1tp(mod) == (lmax == 1), name
        assert C.parse_blocks(str(mod.iri1)) == C.parse_blocks(C.product_irreps(name, H, lmax)[0])
        _run_all_paths((name, H, lmax), 137, 100, monkeypatch, fails, dtypes=("fp32", "fp64") if H < 64 else ("fp32",))
    assert not fails, fails


# ---- 2. what the fused weight gradient supports ----
@pytest.mark.parametrize("lmax", LMAX)
@pytest.mark.parametrize("H", HIDDEN)
def test_fused_weight_gradient_support_table(H, lmax):
    """the status of e3_tp_backward_weights is pinned; a refused call leaves every zero-filled grad_W buffer untouched
    (tp_backward reuses the buffers in the fallback), an accepted one meets the oracle per path block"""
    fails = []
    for name in PRODUCTS:
        key = (name, H, lmax)
        st, gws, ref = _wgrad_direct(key, 137, 100)
        assert st == WGRAD_STATUS[key], (key, st)
        mod = C.module(key)
        for c, g in enumerate(gws):
            if g is None:
                continue
            if st == 4:
                assert not bool(g.any()), (key, T.CLASSES[c])
            else:
                for blk, e in C.block_errors(g, ref.gw[T.CLASSES[c]], C.path_row_blocks(mod.iri1, lmax, c), axis=0):
                    _note("wgrad direct call [fused]", "fp32", e, blk, f"{name}-{H}-{lmax}-B137")
                    if not e < BOUND["fp32"]:
                        fails.append((key, blk, e))
    assert not fails, fails


# ---- 3. instantiations no product reaches with every class requested ----
@pytest.mark.parametrize("B", [137, 2061])
@pytest.mark.parametrize("case", ["msg1-H64-l1-only-l1o", "synthetic"])
def test_weight_gradient_instantiations_6x8_and_8x8(case, B, monkeypatch):
    """<6,8>: message #1 at hidden 64, l_max 1 with class l1o alone (K 257 x M 64 = 18 tiles, 8-row tiles); <8,8>:
    128x0e+128x1o -> 128x1o (K 256 x M 128 = 32 tiles).  The library call with l1o alone must be accepted and meet the oracle.
    Through the MODULE only <8,8> is reached: L1TensorProduct asks tp_backward for every present class as soon as one weight
    wants a gradient, so message #1 at (64, 1) is refused because of l0e (36 tiles) even when only weights_l1o requires grad, and
    its module runs below are GEMM runs (pinned: status [4]).  <6,8> is exercised by the direct call alone."""
    key = ("msg1", 64, 1) if case != "synthetic" else ("synthetic",)
    classes = ("l1o",)
    st, gws, ref = _wgrad_direct(key, B, 300, classes)
    assert st == 0, st
    mod = C.module(key)
    assert tuple(c for c in C.classes_of(mod) if c in classes) == classes
    fails = []
    for blk, e in C.block_errors(gws[3], ref.gw["l1o"], C.path_row_blocks(mod.iri1, 1, 3), axis=0):
        _note("wgrad direct call [fused]", "fp32", e, blk, f"{case}-B{B}")
        if not e < BOUND["fp32"]:
            fails.append(("direct", blk, e))
    for path in ("wgrad", "wgrad_gemm"):
        got = C.run_path(mod, ref, path, monkeypatch, classes=classes)
        assert got.wgrad_status == ([] if path == "wgrad_gemm" else [0] if case == "synthetic" else [4]), (path, got.wgrad_status)
        _check(mod, got, ref, "fp32", path, f"{case}-B{B}", fails)
    assert not fails, fails


# ---- 4. row-tile edges ----
@pytest.mark.parametrize("B", [1, 7, 8, 9, 15, 16, 17, 33])
@pytest.mark.parametrize("key", [("msg1", 16, 2), ("msg1", 32, 1)], ids=["msg1-H16-l2", "msg1-H32-l1"])
def test_row_tile_edges(key, B, monkeypatch):
    fails = []
    _run_all_paths(key, B, 400 + B, monkeypatch, fails)
    assert not fails, fails


@pytest.mark.parametrize("key", [("msg1", 16, 2), ("msg1", 32, 1)], ids=["msg1-H16-l2", "msg1-H32-l1"])
def test_empty_batch_every_path(key, monkeypatch):
    mod = C.module(key)
    x = torch.empty(0, mod.in1_dim, device=DEV)
    y = torch.empty(0, mod.in2_dim, device=DEV)
    for path in C.paths_of(mod):
        C.configure(monkeypatch, path)
        n1, n2, cl = C.wanted(path, mod)
        got = C.run(mod, x, y, torch.empty(0, C.irreps_dim(str(mod.iro)), device=DEV), n1, n2, cl)
        assert tuple(got.out.shape) == (0, C.irreps_dim(str(mod.iro))), path
        if n1:
            assert tuple(got.gx.shape) == (0, mod.in1_dim), path
        if n2:
            assert tuple(got.gy.shape) == (0, mod.in2_dim), path
        for c in cl:
            w = getattr(mod, "weights_" + c)
            assert got.gw[c].shape == w.shape and got.gw[c].dtype == w.dtype and not bool(got.gw[c].any()), (path, c)


# ---- 5. grid wrap with a ragged last tile ----
@pytest.mark.parametrize("key", [("upd2", 64, 2), ("msg2", 16, 2), ("msg1", 32, 1)],
                         ids=["upd2-H64-l2", "msg2-H16-l2", "msg1-H32-l1"])
def test_grid_wrap_ragged_last_tile(key, monkeypatch):
    """B = 16403 = 16384 + 19: above every grid-stride wrap (rows / w kernels 4096 rows, operands / contract 16384 / 8192, the
    weight gradient 256 x per_cu x R <= 16384), last tile ragged for R = 8 and R = 16.  Every block, all rows."""
    fails = []
    try:
        _run_all_paths(key, 16403, 500, monkeypatch, fails, paths=("rows", "gemm", "wgrad", "dual"))
    finally:
        C.reference.cache_clear()   # a reference of this size is some hundred MB of host memory
    assert not fails, fails


# ---- 6. workspace chunks ----
@pytest.mark.parametrize("bcast", [False, True], ids=["per-row-in2", "broadcast-in2"])
def test_workspace_chunks(bcast, monkeypatch):
    """_BWD_WORKSPACE_BYTES = 1: chunks of the floor of 256 rows, B = 517 = 256 + 256 + 5.  Broadcast in2: grad_in2 is [1, Dy] and
    accumulates over the three e3_tp_backward_contract calls; the same case on the generic kernels."""
    from scalable_e3_gnn_amd import tensor_product as TPM
    key = ("upd1", 16, 2)
    mod = C.module(key)
    ref = C.reference(key, 517, 600, bcast)
    assert tuple(ref.gy.shape) == ((1, 9) if bcast else (517, 9))
    fails = []
    monkeypatch.setattr(TPM, "_BWD_WORKSPACE_BYTES", 1)
    for path in ("gemm", "rows") if bcast else ("gemm",):
        got = C.run_path(mod, ref, path, monkeypatch)
        assert tuple(got.gy.shape) == tuple(ref.gy.shape)
        _check(mod, got, ref, "fp32", path, f"chunks-{'bcast' if bcast else 'rows'}-B517", fails)
    assert not fails, fails


# ---- 7. partial requests, values checked ----
@pytest.mark.parametrize("B", [137, 600])
@pytest.mark.parametrize("request_", ["in1", "in2", "one-class", "in1+one-class"])
def test_partial_requests_values(request_, B, monkeypatch):
    """default thresholds: B = 137 on the generic kernels, B = 600 on operands / GEMMs / contract (one class alone: the fused
    weight gradient)"""
    key = ("msg2", 32, 2)
    mod = C.module(key)
    ref = C.reference(key, B, 700)
    n1 = "in1" in request_
    n2 = request_ == "in2"
    classes = ("l1o",) if "one-class" in request_ else ()
    got = C.run_spied(monkeypatch, mod, ref.x.to(DEV), ref.y.to(DEV), ref.gout.to(DEV), n1, n2, classes)
    assert got.wgrad_status == ([0] if (request_ == "one-class" and B == 600) else []), got.wgrad_status
    assert (got.gx is not None) == n1 and (got.gy is not None) == n2
    assert [c for c, g in got.gw.items() if g is not None] == list(classes)
    fails = []
    _check(mod, got, ref, "fp32", "partial", f"partial-{request_}-B{B}", fails)
    assert not fails, fails


# ---- 8. strides ----
def _strided(x, go):
    xm = R.misaligned_copy(x)
    wide = torch.zeros(go.shape[0], go.shape[1] + 3, device=DEV)
    gs = wide[:, 2:2 + go.shape[1]]
    gs.copy_(go)
    assert xm.data_ptr() % 16 and xm.stride(0) == x.shape[1] + 2 and gs.stride(0) == go.shape[1] + 3 and not gs.is_contiguous()
    return xm, gs


def _assert_bit_identical(a, b, classes, what, gy=True):
    assert torch.equal(a.out, b.out), what
    assert a.gx is None or torch.equal(a.gx, b.gx), what
    assert not gy or a.gy is None or torch.equal(a.gy, b.gy), what
    for c in classes:
        assert torch.equal(a.gw[c], b.gw[c]), (what, c)


@pytest.mark.parametrize("key", [("upd1", 16, 2), ("msg1", 32, 1)], ids=["upd1-H16-l2", "msg1-H32-l1"])
def test_misaligned_in1_and_row_strided_grad_out(key, monkeypatch):
    """in1 at a 4-byte-aligned base with a leading dimension of D1 + 2, grad_out as a column slice of a wider tensor, B = 137, every
    path: within the bound against the oracle, and bit-identical to the contiguous call wherever the result has one summation
    order -- everything on gemm / wgrad_gemm, everything of e3_l1tp_backward, out / grad_in1 of e3_tp_backward.
    Two sums of e3_tp_backward have no fixed order and are held to the bound against the oracle instead, as on wgrad:
      grad_W   (tp_bwd_w_kernel) is added by global atomics from one workgroup per 8 rows, 18 workgroups at B = 137: two identical
               contiguous calls already differ in the last bit.  Bit identity is asserted at B = 8, where one workgroup adds
               every element once.
      grad_in2 (tp_bwd_rows_kernel) is reduced over the out channels by float LDS atomics from several waves of a workgroup: it
               was bit-equal in every run made, but nothing in the kernel fixes the order.
    What reaches the kernels: SHTensorProduct hands the row-strided grad_out on with its leading dimension.  L1TensorProduct
    (message #1 at (32, 1)) makes grad_out contiguous before any kernel sees it, so for that operator only the misaligned in1 is
    exercised and the strided grad_out checks the copy."""
    mod = C.module(key)
    ref = C.reference(key, 137, 100)
    x, y, go = ref.x.to(DEV), ref.y.to(DEV), ref.gout.to(DEV)
    xm, gs = _strided(x, go)
    fails = []
    for path in C.paths_of(mod):
        C.configure(monkeypatch, path)
        n1, n2, cl = C.wanted(path, mod)
        got = C.run_spied(monkeypatch, mod, xm, y, gs, n1, n2, cl)
        _check(mod, got, ref, "fp32", path, f"strided-{'-'.join(map(str, key))}", fails)
        if path in ("rows", "gemm", "wgrad_gemm"):
            atomics = path == "rows" and not C.is_l1tp(mod)
            _assert_bit_identical(got, C.run(mod, x, y, go, n1, n2, cl), () if atomics else cl, path, gy=not atomics)
    if not C.is_l1tp(mod):
        ref8 = C.reference(key, 8, 101)
        x, y, go = ref8.x.to(DEV), ref8.y.to(DEV), ref8.gout.to(DEV)
        xm, gs = _strided(x, go)
        C.configure(monkeypatch, "rows")
        n1, n2, cl = C.wanted("rows", mod)
        got = C.run_spied(monkeypatch, mod, xm, y, gs, n1, n2, cl)
        _check(mod, got, ref8, "fp32", "rows", f"strided-{'-'.join(map(str, key))}-B8", fails)
        _assert_bit_identical(got, C.run(mod, x, y, go, n1, n2, cl), cl, "rows B=8", gy=False)
    assert not fails, fails


# ---- 9. bf16 ----
def test_bf16_backward_is_refused():
    mod = R.product("upd2", 16, 2, "bf16")
    x = torch.randn(5, mod.in1_dim, device=DEV).bfloat16().requires_grad_(True)
    with pytest.raises(NotImplementedError):
        mod(x, torch.randn(5, mod.in2_dim, device=DEV))

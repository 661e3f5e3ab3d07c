"""The pinned operator's own kernels (csrc/e3_l1tp.hip generic forward and pack, csrc/e3_l1tp_mfma.hip fp32 MFMA forward,
csrc/e3_l1tp_bwd.hip rows / weights / column-sum kernels) against fp64 at mixed parity, past every grid wrap and through the
strides of the C boundary.  tests/test_l1tp_parent_bits_gpu.py holds these kernels to the parent's bits; this file holds them to
an oracle.  Helpers: tests/l1tp_cases.py (plans p0-p6, references) on top of tests/bwd_cases.py (error norm, blocks, the ways a
module's backward is driven).

Plans: weights from the constructor under torch.manual_seed; EVERY NORM BUFFER IS THEN OVERWRITTEN with seeded values in
[0.5, 1.5], pairwise distinct inside a class (the constructor's are constant within an irreps block, so a norm read from the
wrong column or component of the same class would go unseen).

Reference: oracle/l1tp_oracle.forward_closed_form (forward) and bwd_cases.oracle_autograd (backward; pinned to the reference's
golden gradients in tests/test_l1tp_oracle_host.py), fp64, on the storage-rounded inputs, weights, norms and grad_out.

Error PER BLOCK, max |got - want| over the block / max |want| over the block: the forward output per out irreps block, grad_in1
per in1 irreps block, grad_in2 per degree, grad_W per path block.  Bounds: fp32 1e-5 forward / 2e-5 backward, fp64 1e-12 / 1e-11,
bf16 2^-8 (fp32 accumulation, every result rounded once to nearest: 2^-9 of the element, hence of the block maximum; the factor 2
covers the accumulation).  One exception: at B = 65 573 fp32 arithmetic on the host already shows up to 1.2e-5 on grad_W blocks
of one or two rows whose maximum is small by chance, so at that B, for grad_W blocks and for the broadcast grad_in2 only, the fp32
bound is max(2e-5, 4 x the error of tp_oracle.forward_torch_cpu run in fp32 under autograd on the same inputs and block); the
factor 4 because the chunked summation order of the kernels is not the host's.  Both figures are printed per block.

The worst block per (test, dtype) is printed when the module ends."""
import pytest
import torch

import bwd_cases as C
import l1tp_cases as L
import models  # noqa: F401
from l1tp_cases import B_WRAP, BWD_BOUND, DEV, FWD_BOUND, SENTINEL
from oracle import l1tp_oracle as O

pytestmark = pytest.mark.gpu

E3_ERR_INVALID_ARG, E3_ERR_UNSUPPORTED = 1, 4
_WORST = {}    # (test, dtype) -> (error, block, case id)


@pytest.fixture(scope="module", autouse=True)
def _print_worst():
    yield
    L.clear_references()
    print("\nworst block per (test, dtype):")
    for (test, dtype), (e, blk, cid) in sorted(_WORST.items()):
        print(f"  {test:34s} {dtype}  {e:.2e}  {blk}  [{cid}]")


def _judge(test, dtype, errs, cid, fails, bound_of=None):
    """every (block, error) against its bound: the forward bound for out blocks, the backward bound for the gradients, or what
    ``bound_of(block)`` returns; misses go to ``fails``, asserted by the caller once the whole case has been measured"""
    for blk, e in errs:
        bound = (FWD_BOUND if blk.startswith("out[") else BWD_BOUND)[dtype]
        if bound_of is not None:
            bound = bound_of(blk, bound)
        if e > _WORST.get((test, dtype), (-1.0,))[0]:
            _WORST[(test, dtype)] = (e, blk, cid)
        if not e < bound:
            print(f"MISS {test} {cid} {dtype} {blk}: {e:.3e} (bound {bound:.2e})")
            fails.append((cid, dtype, blk, e))


def _forward(pid, B, seed, dtype, kernel, bcast):
    """-> (got, want) of one forward launch"""
    x, y, want = L.forward_reference(pid, B, seed, bcast, dtype == "bf16")
    dt = L.TORCH_DTYPE[dtype]
    got = L.forward(L.module(pid, dtype), x.to(dt).to(DEV), y.to(dt).to(DEV), kernel)
    assert got.dtype == dt and tuple(got.shape) == want.shape and got.is_contiguous()
    return got, want


# ---- 1. forward, tile edges ----
FWD_RUNS = (("fp32", 1), ("fp64", 1), ("bf16", 1), ("fp32", 2))   # kernel 1 = generic (16-row tiles), 2 = MFMA (32-row tiles)


@pytest.mark.parametrize("B", [1, 15, 16, 17, 31, 32, 33, 63, 64, 65])
@pytest.mark.parametrize("pid", ["p0", "p2", "p6"])
def test_forward_tile_edges(pid, B):
    fails = []
    for bcast in (False, True):
        for dtype, kernel in FWD_RUNS:
            got, want = _forward(pid, B, 1000 + B, dtype, kernel, bcast)
            cid = f"{pid}-B{B}-{'bcast' if bcast else 'rows'}"
            _judge(f"forward edges k{kernel}", dtype, C.block_errors(got, want, L.out_blocks(pid)), cid, fails)
    assert not fails, fails


# ---- 2. forward, every wave past its first tile ----
WRAP_FWD = {   # plan -> [(dtype, kernel, broadcast in2)]
    "p0": [("fp32", 2, False), ("fp32", 1, False), ("fp64", 1, False), ("bf16", 1, False)],
    "p3": [("fp32", 2, False)],
    "p4": [("fp32", 2, False), ("fp32", 1, False), ("fp32", 2, True), ("fp32", 1, True)],
    "p5": [("fp32", 2, False)],
}


@pytest.mark.parametrize("pid", sorted(WRAP_FWD))
def test_forward_every_wave_past_its_first_tile(pid):
    """B = 65 573 = 256 blocks x 8 waves x 32 rows + 37: whatever nwaves a plan has, some wave of the MFMA kernel restages its
    in-tile buffer for a second tile and the last tile has 5 rows; the generic grid (2048 tiles of 16 rows) wraps twice.  Every
    row and every block against the oracle; where both kernels ran in fp32 they agree within 1e-5."""
    fails, fp32 = [], {}
    try:
        for dtype, kernel, bcast in WRAP_FWD[pid]:
            got, want = _forward(pid, B_WRAP, 2000, dtype, kernel, bcast)
            cid = f"{pid}-B{B_WRAP}-{'bcast' if bcast else 'rows'}"
            _judge(f"forward wrap k{kernel}", dtype, C.block_errors(got, want, L.out_blocks(pid)), cid, fails)
            if dtype == "fp32":
                fp32[(kernel, bcast)] = got
        for bcast in (False, True):
            if (1, bcast) in fp32 and (2, bcast) in fp32:
                for blk, e in C.block_errors(fp32[(2, bcast)], fp32[(1, bcast)].double().cpu().numpy(), L.out_blocks(pid)):
                    if not e < 1e-5:
                        fails.append((pid, "k2 vs k1", bcast, blk, e))
        assert pid not in ("p0", "p4") or (1, False) in fp32 and (2, False) in fp32
    finally:
        L.clear_references()
    assert not fails, fails


# ---- 3..5. backward ----
def _backward(pid, B, seed, dtype, bcast, path, monkeypatch, test, fails, need=None, classes=None):
    """one module backward on ``path`` (bwd_cases.configure) against the reference, per block -> bwd_cases.Got"""
    ref = L.reference(pid, B, seed, bcast, dtype == "bf16")
    mod = L.module(pid, dtype)
    C.configure(monkeypatch, path)
    n1, n2, cl = C.wanted(path, mod)
    if need is not None:
        n1, n2 = need
    if classes is not None:
        cl = classes
    x, y, go = L.on_device(ref, dtype)
    got = C.run_spied(monkeypatch, mod, x, y, go, n1, n2, cl)
    assert (got.gx is not None) == n1 and (got.gy is not None) == n2
    cid = f"{pid}-B{B}-{'bcast' if bcast else 'rows'}"
    bound_of = None
    if B == B_WRAP and dtype == "fp32":
        cpu_gy, cpu_gw = L.cpu_fp32_backward(pid, ref)
        cpu = {}
        for c, gw in got.gw.items():
            if gw is not None:
                cpu.update(C.block_errors(cpu_gw[c], ref.gw[c], L.weight_blocks(pid, c), axis=0))
        if bcast and got.gy is not None:
            cpu.update(C.block_errors(cpu_gy, ref.gy, C.in2_blocks(L.LMAX_SH)))
        errs = dict(L.errors(pid, got, ref))
        for blk in sorted(cpu):
            print(f"{test} {cid} {blk}: gpu {errs[blk]:.2e}  host fp32 {cpu[blk]:.2e}  bound {max(2e-5, 4 * cpu[blk]):.2e}")

        def bound_of(blk, bound):
            return max(bound, 4 * cpu[blk]) if blk in cpu else bound
    _judge(test, dtype, L.errors(pid, got, ref), cid, fails, bound_of)
    return got


@pytest.mark.parametrize("dtype", ["fp32", "fp64", "bf16"])
@pytest.mark.parametrize("pid", ["p0", "p1", "p2", "p3", "p6"])
def test_own_backward_every_plan(pid, dtype, monkeypatch):
    """e3_l1tp_backward at B = 137 (below 256: the column sum of the broadcast case stays in one block), in2 per row and [1, 4]"""
    fails = []
    for bcast in (False, True):
        got = _backward(pid, 137, 3000, dtype, bcast, "rows", monkeypatch, "own backward", fails)
        assert got.wgrad_status == [], got.wgrad_status
        assert tuple(got.gy.shape) == ((1, 4) if bcast else (137, 4))
    assert not fails, fails


@pytest.mark.parametrize("B", [1, 15, 16, 17, 33])
@pytest.mark.parametrize("pid", ["p0", "p2"])
def test_own_backward_row_tile_edges(pid, B, monkeypatch):
    fails = []
    got = _backward(pid, B, 3100 + B, "fp32", False, "rows", monkeypatch, "own backward edges", fails)
    assert got.wgrad_status == [], got.wgrad_status
    assert not fails, fails


@pytest.mark.parametrize("bcast", [False, True], ids=["per-row-in2", "broadcast-in2"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("pid", ["p0", "p2"])
def test_own_backward_wraps(pid, dtype, bcast, monkeypatch):
    """B = 65 573: the rows kernel past its 2048-tile grid, the weights kernel at 9 tiles per chunk with a short last chunk,
    colsum4_stage1 at 256 blocks with 37 rows on its second pass"""
    fails = []
    try:
        got = _backward(pid, B_WRAP, 4000, dtype, bcast, "rows", monkeypatch, "own backward wrap", fails)
        assert got.wgrad_status == [], got.wgrad_status
        assert tuple(got.gy.shape) == ((1, 4) if bcast else (B_WRAP, 4))
    finally:
        L.clear_references()
    assert not fails, fails


def test_own_backward_two_column_sum_blocks(monkeypatch):
    """B = 300 with broadcast in2: two blocks of colsum4_stage1 (256 + 44 rows), no wrap"""
    fails = []
    got = _backward("p0", 300, 4100, "fp32", True, "rows", monkeypatch, "own backward colsum", fails)
    assert tuple(got.gy.shape) == (1, 4)
    assert not fails, fails


# what e3_tp_backward_weights answered for the plan with every class requested, as observed on an MI355X (0 = the fused
# kernels ran, 4 = refused: the caller takes the GEMM path); read by bwd_cases.spy_fused_wgrad, not predicted.  Mixed parity is
# NOT refused: on ``wgrad`` and ``dual`` the grad_W of these plans, 0o and 1e classes included, comes from the fused kernels
WGRAD_STATUS = {"p0": 0, "p2": 0, "p6": 0}


@pytest.mark.parametrize("path", ["gemm", "wgrad", "wgrad_gemm", "dual"])
@pytest.mark.parametrize("pid", ["p0", "p2", "p6"])
def test_other_backward_paths_at_mixed_parity(pid, path, monkeypatch):
    fails = []
    got = _backward(pid, 137, 5000, "fp32", False, path, monkeypatch, f"path {path}", fails)
    print(f"e3_tp_backward_weights answered {got.wgrad_status} for {pid} on {path}")
    assert got.wgrad_status == ([WGRAD_STATUS[pid]] if path in ("wgrad", "dual") else []), (pid, path, got.wgrad_status)
    assert not fails, fails


def test_dual_at_mixed_parity_past_the_wrap(monkeypatch):
    """p0 at B = 65 573 on ``dual``: grad_in1 is the MFMA forward loop on the transposed operator, second tile per wave"""
    fails = []
    try:
        got = _backward("p0", B_WRAP, 5100, "fp32", False, "dual", monkeypatch, "path dual wrap", fails)
        print(f"e3_tp_backward_weights answered {got.wgrad_status} for p0 on dual at B = {B_WRAP}")
        assert got.wgrad_status == [WGRAD_STATUS["p0"]], got.wgrad_status
    finally:
        L.clear_references()
    assert not fails, fails


# ---- 6. partial requests on the operator's own kernels ----
@pytest.mark.parametrize("request_", ["in1", "in2", "one-class", "in1+one-class"])
def test_partial_requests_own_kernels(request_, monkeypatch):
    n1, n2 = "in1" in request_, request_ == "in2"
    classes = ("l1e",) if "one-class" in request_ else ()
    fails = []
    got = _backward("p0", 137, 6000, "fp32", False, "rows", monkeypatch, "partial requests", fails, need=(n1, n2), classes=classes)
    assert got.wgrad_status == [], got.wgrad_status
    assert (got.gx is not None) == n1 and (got.gy is not None) == n2
    assert [c for c, g in got.gw.items() if g is not None] == list(classes)   # nothing that was not asked for
    assert not fails, fails


# ---- 7. strides through the C ABI ----
def _abi_operands(pid, dtype, B=37):
    ref = L.reference(pid, B, 7000, False, dtype == "bf16")
    mod = L.module(pid, dtype)
    x, y, go = L.on_device(ref, dtype)
    return ref, mod, x, y, go, mod.in1_dim, mod.iro.dim


@pytest.mark.parametrize("dtype,kernel", [("fp32", 1), ("fp32", 2), ("fp64", 1), ("bf16", 1)])
@pytest.mark.parametrize("pid", ["p0", "p4"])
def test_abi_forward_strides(pid, dtype, kernel):
    """in1 at a 4-byte-aligned, not 16-byte-aligned base with ld_in1 = D1 + 2, out inside a sentinel-filled buffer with
    ld_out = Dout + 3: the rows equal the contiguous call bit for bit (one summation order), every sentinel is intact"""
    B = 37
    ref, mod, x, y, _, D1, Dout = _abi_operands(pid, dtype)
    off = L.aligned4_offset(dtype)
    _, xv = L.inside(B, D1, 2, off, dtype)
    xv.copy_(x)
    assert xv.data_ptr() % 4 == 0 and xv.data_ptr() % 16 != 0 and xv.stride(0) == D1 + 2
    plain = torch.full((B, Dout), SENTINEL, dtype=x.dtype, device=DEV)
    assert L.forward_call(mod, x, D1, y, 4, plain, Dout, B, dtype, kernel) == 0
    fails = []
    _judge(f"abi forward k{kernel}", dtype, C.block_errors(plain, ref.out, L.out_blocks(pid)), f"{pid}-B{B}", fails)
    assert not fails, fails
    buf, ov = L.inside(B, Dout, 3, off, dtype, SENTINEL, guard_rows=1)
    assert L.forward_call(mod, xv, D1 + 2, y, 4, ov, Dout + 3, B, dtype, kernel) == 0
    assert torch.equal(ov, plain)
    assert L.untouched_outside(buf, B, Dout, off, 1)


@pytest.mark.parametrize("dtype", ["fp32", "fp64", "bf16"])
@pytest.mark.parametrize("pid", ["p0", "p4"])
def test_abi_backward_strides(pid, dtype):
    """grad_out with ld_gout = Dout + 3, grad_in1 into a sentinel-filled buffer with ld_gin1 = D1 + 5: bit for bit the contiguous
    call, every sentinel intact"""
    B = 37
    ref, mod, x, y, go, D1, Dout = _abi_operands(pid, dtype)
    off = L.aligned4_offset(dtype)
    g1 = torch.full((B, D1), SENTINEL, dtype=x.dtype, device=DEV)
    g2 = torch.full((B, 4), SENTINEL, dtype=x.dtype, device=DEV)
    gw = L.weight_grad_buffers(mod)
    assert L.backward_call(mod, x, D1, y, 4, go, Dout, g1, D1, g2, gw, B, dtype) == 0
    got = C.Got()
    got.out, got.gx, got.gy, got.gw = torch.as_tensor(ref.out), g1, g2, gw
    fails = []
    _judge("abi backward", dtype, L.errors(pid, got, ref), f"{pid}-B{B}", fails)
    assert not fails, fails
    _, gov = L.inside(B, Dout, 3, 2, dtype)
    gov.copy_(go)
    assert gov.stride(0) == Dout + 3 and not gov.is_contiguous()
    buf, g1v = L.inside(B, D1, 5, off, dtype, SENTINEL, guard_rows=1)
    g2s = torch.full((B, 4), SENTINEL, dtype=x.dtype, device=DEV)
    gws = L.weight_grad_buffers(mod)
    assert L.backward_call(mod, x, D1, y, 4, gov, Dout + 3, g1v, D1 + 5, g2s, gws, B, dtype) == 0
    assert torch.equal(g1v, g1) and torch.equal(g2s, g2)
    for c in gw:
        assert torch.equal(gws[c], gw[c]), c
    assert L.untouched_outside(buf, B, D1, off, 1)


@pytest.mark.parametrize("pid", ["p0", "p4"])
def test_abi_refusals_leave_the_outputs_untouched(pid):
    B = 37
    _, mod, x, y, go, D1, Dout = _abi_operands(pid, "fp32")
    out = torch.full((B + 2, Dout + 3), SENTINEL, device=DEV)
    for kernel in (1, 2):
        assert L.forward_call(mod, x, D1, y, 4, out, Dout - 1, B, "fp32", kernel) == E3_ERR_INVALID_ARG
        for ld2 in (1, 2, 3):
            assert L.forward_call(mod, x, D1, y, ld2, out, Dout, B, "fp32", kernel) == E3_ERR_INVALID_ARG
    assert bool((out == SENTINEL).all())
    for dtype in ("fp64", "bf16"):   # the MFMA kernel is fp32 only
        _, m, xs, ys, _, _, _ = _abi_operands(pid, dtype)
        o = torch.full((B + 2, Dout + 3), SENTINEL, dtype=xs.dtype, device=DEV)
        assert L.forward_call(m, xs, D1, ys, 4, o, Dout, B, dtype, 2) == E3_ERR_UNSUPPORTED
        assert bool((o == SENTINEL).all())
    g1 = torch.full((B + 2, D1 + 5), SENTINEL, device=DEV)
    g2 = torch.full((B, 4), SENTINEL, device=DEV)
    gw = L.weight_grad_buffers(mod)
    assert L.backward_call(mod, x, D1, y, 4, go, Dout, g1, D1 - 1, g2, gw, B, "fp32") == E3_ERR_INVALID_ARG
    for ld2 in (1, 2, 3):
        assert L.backward_call(mod, x, D1, y, ld2, go, Dout, g1, D1, g2, gw, B, "fp32") == E3_ERR_INVALID_ARG
    assert bool((g1 == SENTINEL).all()) and bool((g2 == SENTINEL).all())
    assert all(bool((g == SENTINEL).all()) for g in gw.values())
    assert sorted(gw) == [c for c in O.CLASSES if hasattr(mod, "weights_" + c)]

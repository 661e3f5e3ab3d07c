"""Helpers of tests/test_l1tp_table_gpu.py and tests/test_l1tp_oracle_host.py: the seven plans of the pinned operator
(L1TensorProduct), their modules with every norm buffer overwritten by pairwise distinct seeded values, the fp64 references
(forward: oracle/l1tp_oracle.forward_closed_form; backward: bwd_cases.oracle_autograd) on the storage-rounded inputs, weights,
norms and grad_out, the blocks the error is taken over, and direct calls of e3_l1tp_forward / e3_l1tp_backward through ctypes.
The error norm, the block helpers and the ways a module's backward is driven are those of tests/bwd_cases.py.
TEST INFRASTRUCTURE ONLY."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

import bwd_cases as C
from oracle import l1tp_oracle as O
from oracle import tp_oracle as T

DEV = C.DEV
PLANS = {
    "p0": ("5x0e+3x0o+7x1o+2x1e", "9x0e+1x0o+4x1e+6x1o"),                        # all four classes, odd run counts
    "p1": ("3x1e", "2x0o+2x1e+3x1o"),                                            # absent input classes; 1o = cross slot only
    "p2": ("2x1o+3x0e+1x1e+2x0e+2x1o+1x0o", "1x1e+2x0e+2x1o+1x0o+3x1o+2x0e"),    # interleaved, several runs per class
    "p3": ("40x0e+40x1o", "40x0e+40x1o"),                                        # two channel tiles; > 2048 weights
    "p4": ("32x0e+32x1o", "32x0e+32x1o"),                                        # 4 waves per block, weights in LDS
    "p5": ("64x0e+64x1o", "64x0e+64x1o"),                                        # weights not in LDS, 3 waves
    "p6": ("33x0o+35x1e+3x0e+2x1o", "34x0o+33x1e+2x0e+1x1o"),                    # second tile of a 0o and a 1e class
}
TORCH_DTYPE = {"fp32": torch.float32, "fp64": torch.float64, "bf16": torch.bfloat16}
# the project's bounds (bwd_cases); bf16: fp32 accumulation, each result rounded once to nearest = 2^-9 of the element, hence
# of the block maximum, and a factor 2 for the accumulation
FWD_BOUND = dict(C.FWD_BOUND, bf16=2.0 ** -8)
BWD_BOUND = dict(C.BOUND, bf16=2.0 ** -8)
B_WRAP = 65573    # 256 blocks x 8 waves x 32 rows + 37: every wave of the MFMA forward meets a second tile, whatever the plan
LMAX_SH = 1
FWD_CHUNK = 2048     # rows per evaluation of the forward oracle
SENTINEL = -4096.0   # exact in bf16; no result comes near it

# every value of [0.5, 1.5] that bf16 holds exactly: the norms survive every storage type unrounded
NORM_GRID = [0.5 + k / 256.0 for k in range(128)] + [1.0 + k / 128.0 for k in range(65)]


def irreps_of(pid):
    return PLANS[pid]


def seeded_norms(mod, seed):
    """Overwrite every norm buffer in place: per class a seeded draw without replacement from NORM_GRID, so no two elements of
    a class (neither two channels nor two components of one channel) share a norm."""
    g = torch.Generator().manual_seed(seed)
    grid = torch.tensor(NORM_GRID, dtype=torch.float32)
    with torch.no_grad():
        for c in O.CLASSES:
            n = getattr(mod, "norm_" + c)
            assert n.numel() <= len(NORM_GRID), (c, n.numel())
            n.copy_(grid[torch.randperm(len(NORM_GRID), generator=g)[:n.numel()]])


@functools.lru_cache(maxsize=None)
def host_module(pid):
    """fp32 on the host: weights from the constructor under torch.manual_seed, norms from ``seeded_norms``.  Shared: read only."""
    from models.segnn.l1_tensor_prod import L1TensorProduct
    from scalable_e3_gnn_amd import Irreps
    i = list(PLANS).index(pid)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(100 + i)
        mod = L1TensorProduct(Irreps(PLANS[pid][0]), Irreps(PLANS[pid][1]))
    seeded_norms(mod, 300 + i)
    return mod


@functools.lru_cache(maxsize=None)
def module(pid, dtype="fp32"):
    """the plan's module on the device in ``dtype``: fp64 holds the fp32 values, bf16 the weights rounded to bf16"""
    import copy
    return copy.deepcopy(host_module(pid)).to(TORCH_DTYPE[dtype]).to(DEV)


def weights_norms(pid, rounded=False):
    """({class: W}, {class: norm}) in fp64 numpy, as the storage type holds them (``rounded``: bf16)"""
    mod = host_module(pid)

    def f64(t):
        t = t.detach()
        return (t.bfloat16().float() if rounded else t).double().numpy()
    W = {c: f64(getattr(mod, "weights_" + c)) for c in O.CLASSES if hasattr(mod, "weights_" + c)}
    N = {c: f64(getattr(mod, "norm_" + c)) for c in O.CLASSES}
    return W, N


# ---- blocks ----
def out_blocks(pid):
    return [(n.replace("in1", "out", 1), s) for n, s in C.in1_blocks(PLANS[pid][1])]


def weight_blocks(pid, c):
    return C.path_row_blocks(PLANS[pid][0], LMAX_SH, T.CLASSES.index(c))


# ---- references ----
def draw(pid, B, seed, bcast=False, rounded=False):
    """x [B, D1], y [B or 1, 4], gout [B, Dout]: fp32 on the host, holding what the storage type holds"""
    x, y, gout = C.draw(host_module(pid), B, seed, bcast)
    if rounded:
        x, y, gout = (t.bfloat16().float() for t in (x, y, gout))
    return x, y, gout


@functools.lru_cache(maxsize=None)
def forward_reference(pid, B, seed, bcast=False, rounded=False):
    """-> (x, y, out): forward_closed_form in fp64, evaluated in row chunks.  Unbounded cache: clear it after a large B."""
    x, y, _ = draw(pid, B, seed, bcast, rounded)
    lay = O.make_layout(*PLANS[pid])
    W, N = weights_norms(pid, rounded)
    xn, yn = x.double().numpy(), y.double().numpy()
    out = np.empty((B, lay.out_dim))

    def chunk(lo):
        hi = min(lo + FWD_CHUNK, B)
        out[lo:hi] = O.forward_closed_form(lay, xn[lo:hi], yn if yn.shape[0] == 1 else yn[lo:hi], W, N)
    if B <= FWD_CHUNK:
        chunk(0)
    else:   # the oracle's einsum is one thread of plain loops that release the GIL: 65 573 rows of p5 take 12 s in one piece
        with ThreadPoolExecutor(max_workers=16) as pool:
            list(pool.map(chunk, range(0, B, FWD_CHUNK)))
    return x, y, out


@functools.lru_cache(maxsize=None)
def reference(pid, B, seed, bcast=False, rounded=False):
    """bwd_cases.Ref of the plan: x, y, gout and the fp64 autograd out, gx, gy, gw.  Unbounded cache, as above."""
    r = C.Ref()
    r.x, r.y, r.gout = draw(pid, B, seed, bcast, rounded)
    W, N = weights_norms(pid, rounded)
    r.out, r.gx, r.gy, r.gw = C.oracle_autograd(PLANS[pid][0], PLANS[pid][1], LMAX_SH, W, N, r.x, r.y, r.gout)
    return r


def clear_references():
    forward_reference.cache_clear()
    reference.cache_clear()


def cpu_fp32_backward(pid, ref):
    """The same oracle (tp_oracle.forward_torch_cpu) run in fp32 under autograd on the inputs of ``ref`` -> (gy, {class: gW}):
    what plain fp32 arithmetic on the host gives, the yardstick of the sums over B_WRAP rows"""
    W, N = weights_norms(pid)
    Wt = {c: torch.as_tensor(w).float().requires_grad_(True) for c, w in W.items()}
    Nt = {c: torch.as_tensor(n).float() for c, n in N.items()}
    y = ref.y.float().clone().requires_grad_(True)
    B = ref.x.shape[0]
    out = T.forward_torch_cpu(PLANS[pid][0], PLANS[pid][1], LMAX_SH, ref.x.float(), y if y.shape[0] == B else y.expand(B, -1),
                              Wt, Nt)
    out.backward(ref.gout.float())
    return y.grad, {c: Wt[c].grad for c in Wt}


def on_device(ref, dtype):
    dt = TORCH_DTYPE[dtype]
    return ref.x.to(dt).to(DEV), ref.y.to(dt).to(DEV), ref.gout.to(dt).to(DEV)


def errors(pid, got, ref):
    """[(block, error)] of everything ``got`` (bwd_cases.Got) holds: out per out irreps block, grad_in1 per in1 irreps block,
    grad_in2 per degree, grad_W per path block"""
    errs = C.block_errors(got.out, ref.out, out_blocks(pid))
    if got.gx is not None:
        errs += C.block_errors(got.gx, ref.gx, C.in1_blocks(PLANS[pid][0]))
    if got.gy is not None:
        assert tuple(got.gy.shape) == tuple(ref.gy.shape), (got.gy.shape, ref.gy.shape)
        errs += C.block_errors(got.gy, ref.gy, C.in2_blocks(LMAX_SH))
    for c, gw in got.gw.items():
        if gw is not None:
            errs += C.block_errors(gw, ref.gw[c], weight_blocks(pid, c), axis=0)
    return errs


def forward(mod, x, y, kernel):
    """the module's forward on the given kernel (1 generic, 2 MFMA), no autograd"""
    mod.kernel = kernel
    try:
        with torch.no_grad():
            return mod(x, y)
    finally:
        mod.kernel = 0


# ---- direct calls through the C ABI ----
def aligned4_offset(dtype):
    """columns to skip so that a view starts on a 4-byte, not on a 16-byte boundary"""
    return 2 if dtype == "bf16" else 1


def inside(rows, width, extra, offset, dtype, fill=0.0, guard_rows=0):
    """-> (buffer, view): a [rows, width] view at column ``offset`` (and row ``guard_rows``) of a ``fill``-filled buffer whose
    rows are ``extra`` elements longer"""
    assert 0 <= offset <= extra
    buf = torch.full((rows + 2 * guard_rows, width + extra), fill, dtype=TORCH_DTYPE[dtype], device=DEV)
    return buf, buf[guard_rows:guard_rows + rows, offset:offset + width]


def untouched_outside(buf, view_rows, width, offset, guard_rows):
    """every element of ``buf`` outside the view still holds SENTINEL"""
    rest = buf.clone()
    rest[guard_rows:guard_rows + view_rows, offset:offset + width] = SENTINEL
    return bool((rest == SENTINEL).all())


def _handle(mod):
    return mod._get_plan().handle(torch.device(DEV))


def forward_call(mod, x, ld1, y, ld2, out, ldo, B, dtype, kernel):
    """e3_l1tp_forward on the module's plan and packed weights; x / y / out: tensors or views whose data_ptr is handed on with
    the given leading dimensions -> status (the stream is synchronised)"""
    from scalable_e3_gnn_amd import _lib
    dt = TORCH_DTYPE[dtype]
    with torch.cuda.device(DEV):
        packed = mod._packed_weights(dt, torch.device(DEV))
        st = _lib.load().e3_l1tp_forward(_handle(mod), x.data_ptr(), ld1, y.data_ptr(), ld2, packed.data_ptr(), out.data_ptr(), ldo,
                                         B, _lib.dtype_code(dt), kernel, torch.cuda.current_stream(DEV).cuda_stream)
        torch.cuda.synchronize()
    return st


def backward_call(mod, x, ld1, y, ld2, gout, ldg, gin1, ldgi, gin2, gws, B, dtype):
    """e3_l1tp_backward on the module's plan, weights and norms; gws: {class: tensor | None} -> status (synchronised)"""
    from scalable_e3_gnn_amd import _lib
    lib = _lib.load()
    dt = TORCH_DTYPE[dtype]
    with torch.cuda.device(DEV):
        h = _handle(mod)
        work = torch.empty(max(int(lib.e3_l1tp_backward_workspace_bytes(h, B, _lib.dtype_code(dt))), 16), dtype=torch.uint8,
                           device=DEV)
        ws = [w.detach().contiguous() if w is not None else None for w in mod._weights()]
        ns = [n.detach().contiguous() if n is not None else None for n in mod._norms()]
        st = lib.e3_l1tp_backward(h, x.data_ptr(), ld1, y.data_ptr(), ld2, _lib.ptr4(ws), _lib.ptr4(ns), gout.data_ptr(), ldg,
                                  gin1.data_ptr() if gin1 is not None else None, ldgi,
                                  gin2.data_ptr() if gin2 is not None else None,
                                  _lib.ptr4([gws.get(c) for c in O.CLASSES]), work.data_ptr(), B, _lib.dtype_code(dt),
                                  torch.cuda.current_stream(DEV).cuda_stream)
        torch.cuda.synchronize()
    return st


def weight_grad_buffers(mod, fill=SENTINEL):
    return {c: torch.full_like(w, fill) for c, w in zip(O.CLASSES, mod._weights()) if w is not None}

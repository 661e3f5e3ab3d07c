"""Every instantiation of the 16-row MFMA product kernel (csrc/e3_tp_mfma_r16.hip) that a SEGNN can reach, one product per
launch, against the fp64 oracle (oracle/tp_oracle.py + oracle/segnn_oracle.gate_blocks) on the storage-rounded inputs and
parameters of the module under test.

The error is taken PER OUTPUT BLOCK -- every contiguous block of the out irreps; after a gate silu(scalars), gated 1o and
gated 2e -- as max |got - want| over the block / max |want| over the block, both over all rows.  Bounds: fp32 storage
1e-5 (the bound of tests/test_tp_l2.py for this kernel and oracle), bf16 storage 1e-2 (the one-product bound of
tests/test_bf16_gpu.py).  The exact fp32 FMA kernel runs beside every fp32 case and its figure is printed in the same
norm.  The worst block of every case is printed; the table by (H, l_max, storage, gate) is printed when the module ends.

Table entries (``r16_kernels()``; a plan resolves by (lmax_sh, 32-channel tile counts per output degree, chunk degrees)):
hidden 32 resolves to the first eleven entries, one per product and l_max ("message TP #1", "message TP #2", "update TP
#1", "update TP #2", "embedding", "readout"; at l_max = 1 update #2 and the embedding share (1, 1,1,0 | 0,1)).  Hidden 16:
update #1 has its own entries ((2, 2,1,1 | 0,1,2,0,1,2) and (1, 1,1,0 | 0,1,0,1)), update #2, embedding and readout pad to
one 32-channel tile and resolve to the hidden-32 entries with one dead K half per chunk; message product #2 at l_max = 1
(16x0e+16x1o -> 16x0e+16x0e+16x1o: one scalar tile, one 1o tile, chunks 0,1) resolves to the l_max = 1 "update TP #2 /
embedding" entry and runs its GATED form with a 16-of-32-channel tile.  Hidden 64: the eight "hidden 64" entries, node-level
products only.  Every other message product at hidden 16 / 64 has no entry: their chunk sequences are not in the table."""
import ctypes

import numpy as np
import pytest
import torch

import models  # noqa: F401
import r16_cases as R
from r16_cases import DEV, DTYPES, GATED, HIDDEN, LMAX, PRODUCTS
from scale_reference import expected_scale

pytestmark = pytest.mark.gpu

BOUND = {"fp32": 1e-5, "bf16": 1e-2}

# what fused_supported(gate=False) / fused_supported(gate=True) must return: (plain, gated) per (product, H, l_max)
_T, _F = True, False
SUPPORT = {
    ("embed", 16, 1): (_T, _F), ("embed", 16, 2): (_T, _F), ("embed", 32, 1): (_T, _F),
    ("embed", 32, 2): (_T, _F), ("embed", 64, 1): (_T, _F), ("embed", 64, 2): (_T, _F),
    ("msg1", 16, 1): (_F, _F), ("msg1", 16, 2): (_F, _F), ("msg1", 32, 1): (_T, _T),
    ("msg1", 32, 2): (_T, _T), ("msg1", 64, 1): (_F, _F), ("msg1", 64, 2): (_F, _F),
    ("msg2", 16, 1): (_T, _T), ("msg2", 16, 2): (_F, _F), ("msg2", 32, 1): (_T, _T),
    ("msg2", 32, 2): (_T, _T), ("msg2", 64, 1): (_F, _F), ("msg2", 64, 2): (_F, _F),
    ("upd1", 16, 1): (_T, _T), ("upd1", 16, 2): (_T, _T), ("upd1", 32, 1): (_T, _T),
    ("upd1", 32, 2): (_T, _T), ("upd1", 64, 1): (_T, _T), ("upd1", 64, 2): (_T, _T),
    ("upd2", 16, 1): (_T, _F), ("upd2", 16, 2): (_T, _F), ("upd2", 32, 1): (_T, _F),
    ("upd2", 32, 2): (_T, _F), ("upd2", 64, 1): (_T, _F), ("upd2", 64, 2): (_T, _F),
    ("readout", 16, 1): (_T, _F), ("readout", 16, 2): (_T, _F), ("readout", 32, 1): (_T, _F),
    ("readout", 32, 2): (_T, _F), ("readout", 64, 1): (_T, _F), ("readout", 64, 2): (_T, _F),
}
ALL = [(p, H, l) for p in PRODUCTS for H in HIDDEN for l in LMAX]
assert sorted(SUPPORT) == sorted(ALL) and len(ALL) == 36
# (product, H, l_max, gate) of every launch the table supports: gated where the model gates, ungated for every product
LAUNCHES = [(p, H, l, g) for (p, H, l) in ALL for g in (False, True) if SUPPORT[(p, H, l)][1 if g else 0]]
MODEL_LAUNCHES = [(p, H, l, p in GATED) for (p, H, l) in ALL if SUPPORT[(p, H, l)][0]]
assert all(SUPPORT[(p, H, l)][1] == (p in GATED) for (p, H, l) in ALL if SUPPORT[(p, H, l)][0])


def _id(p, H, l, storage=None, gate=None, B=None):
    s = f"{p}-H{H}-l{l}"
    if storage is not None:
        s += f"-{storage}"
    if gate is not None:
        s += "-gated" if gate else "-plain"
    if B is not None:
        s += f"-B{B}"
    return s


_FIGURES = {}   # (H, l_max, storage, gate) -> [worst MFMA figure, worst exact-fp32 figure | None, case id]


def _note(H, l, storage, gate, err, exact, cid):
    fig = _FIGURES.setdefault((H, l, storage, gate), [-1.0, None, ""])
    if err > fig[0]:
        fig[0], fig[2] = err, cid
    if exact is not None and (fig[1] is None or exact > fig[1]):
        fig[1] = exact


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _FIGURES:
        print("\nworst per-block error by (H, l_max, storage, gate): MFMA kernel | exact fp32 kernel | case")
        for k in sorted(_FIGURES, key=str):
            e, x, cid = _FIGURES[k]
            print(f"  H={k[0]:2d} l_max={k[1]} {k[2]} {'gated' if k[3] else 'plain'}: {e:.2e} | "
                  f"{'%.2e' % x if x is not None else '   -    '} | {cid}")


def _last_kernel():
    from scalable_e3_gnn_amd import _lib
    return _lib.load().e3_tp_last_fused_kernel()


def _launch(mod, segments, in2, gate, **kw):
    """forward_fused on the 16-row kernel: anything else (another kernel, a fall-back, None) fails the test"""
    with torch.no_grad():
        r = mod.forward_fused(segments, in2, gate=gate, **kw)
    assert r is not None
    assert _last_kernel() == R.KERNEL, _last_kernel()
    return r


def _check_blocks(mod, H, l, storage, gate, got, want, cid, exact=None):
    blocks = R.out_blocks(mod, H, gate)
    errs = R.block_errors(got.float(), want, blocks)
    name, err = R.worst(errs)
    ex = None
    line = f"\n{cid}: worst block {name} {err:.2e}"
    if exact is not None:
        xerrs = R.block_errors(exact, want, blocks)
        ex = R.worst(xerrs)[1]
        line += f" | exact fp32 kernel: worst block {R.worst(xerrs)[0]} {ex:.2e}"
    print(line)
    _note(H, l, storage, gate, err, ex, cid)
    bad = [(n, e) for n, e in errs if not e <= BOUND[storage]]
    assert not bad, (cid, bad, errs)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,H,l", ALL, ids=[_id(*c) for c in ALL])
def test_support_matrix(p, H, l):
    """The library's answer for all 36 (product, H, l_max), both storage types (the table does not depend on storage)."""
    for storage in DTYPES:
        mod = R.product(p, H, l, storage)
        assert (bool(mod.fused_supported(False)), bool(mod.fused_supported(True))) == SUPPORT[(p, H, l)], (p, H, l, storage)


def test_unsupported_products_are_refused_not_rerouted():
    """A product without a table entry gets an error from the C entry: there is no other kernel behind forward_fused."""
    for (p, H, l) in ALL:
        if SUPPORT[(p, H, l)][0]:
            continue
        inp = R.Inputs(p, H, l, "fp32", 17, seed=3)
        with pytest.raises(RuntimeError), torch.no_grad():
            R.product(p, H, l, "fp32").forward_fused(inp.segments(), inp.y(), gate=True)


# ---- 1. tile edges, every supported instantiation ----
EDGE_B = (1, 15, 16, 17, 65, 137)   # 65: one workgroup of four tiles + one row; 137: two workgroups + a ragged tile
EDGE = [(p, H, l, s, g, B) for (p, H, l, g) in LAUNCHES for s in DTYPES for B in EDGE_B]


@pytest.mark.parametrize("p,H,l,storage,gate,B", EDGE, ids=[_id(*c) for c in EDGE])
def test_tile_edges_vs_oracle(p, H, l, storage, gate, B):
    mod = R.product(p, H, l, storage)
    cid = _id(p, H, l, storage, gate, B)
    inp = R.Inputs(p, H, l, storage, B, seed=7 * B + H + l)
    if p == "msg1" and B >= 15:
        for i in inp.idx[:2]:
            v = i.cpu().numpy()
            assert 0 in v and R.NTABLE - 1 in v and len(np.unique(v)) < B
        assert bool((inp.idx[0][1:] >= inp.idx[0][:-1]).all())
    got = _launch(mod, inp.segments(), inp.y(), gate)          # fp32: computes its own in_scale
    want = R.oracle(mod, H, gate, *inp.dense())
    assert got.dtype == DTYPES[storage] and tuple(got.shape) == want.shape
    assert bool(torch.isfinite(got).all())
    exact = R.exact_fp32(mod, H, gate, inp.cat(), inp.y()) if storage == "fp32" else None
    _check_blocks(mod, H, l, storage, gate, got, want, cid, exact)


# ---- 2. the wave's tile loop ----
# r16_launch: grid = min(ceil(ntiles / 4 waves), 256 * waves_per_simd) workgroups of 4 waves, so a wave runs a second tile as
# soon as B > 16 * 4 * 256 * waves_per_simd rows.  waves_per_simd is 1, 2 or 3 (r16_waves_per_simd): B = 16 * 4 * 768 + 69 is
# above the threshold of all three -- 3077 tiles over at most 3072 waves -- and its last tile has 5 rows.
LOOP_B = 16 * 4 * 768 + 69
LOOP = [(p, H, l, s, g) for (p, H, l, g) in MODEL_LAUNCHES for s in DTYPES]


def _windows(B):
    w = [(0, 16), (B - 37, B)] + [(c - 32, c + 32) for c in range(16384, B, 16384) if c + 32 <= B]
    return sorted(w)


@pytest.mark.parametrize("p,H,l,storage,gate", LOOP, ids=[_id(*c) for c in LOOP])
def test_tile_loop_sampled_rows_and_row_independence(p, H, l, storage, gate):
    """Sampled rows of a launch in which every wave runs more than one tile against the oracle, and -- bitwise -- against
    the same rows run as a small batch of their own (same row indices, in2 rows and in_scale): a row then sits in the same
    lane of the same tile position, so a difference is stale staging, a stale prefetched row index or an accumulator that
    was not reset between two tiles of a wave."""
    from scalable_e3_gnn_amd import ops
    B = LOOP_B
    assert B > 16 * 4 * 256 * 3 and B % 16 == 5
    mod = R.product(p, H, l, storage)
    inp = R.Inputs(p, H, l, storage, B, seed=11 + H + l, device_rng=True)
    sc = ops.pow2_scale(inp.tensors) if storage == "fp32" else None
    got = _launch(mod, inp.segments(), inp.y(), gate, in_scale=sc)
    assert got.shape[0] == B
    wins = _windows(B)
    assert len(wins) == 5 and all(lo % 16 == 0 for lo, _ in wins)
    rows = np.concatenate([np.arange(lo, hi) for lo, hi in wins])
    want = np.concatenate([R.oracle(mod, H, gate, *inp.dense(lo, hi)) for lo, hi in wins])
    sample = got[torch.as_tensor(rows, device=DEV)]
    assert bool(torch.isfinite(sample).all())
    _check_blocks(mod, H, l, storage, gate, sample, want, _id(p, H, l, storage, gate, B))
    for lo, hi in wins:
        small = _launch(mod, inp.segments(lo, hi), inp.y(lo, hi), gate, in_scale=sc)
        assert torch.equal(small, got[lo:hi]), (lo, hi, float((small.float() - got[lo:hi].float()).abs().max()))


# ---- 3. staging and store branches ----
NARROW = [(p, H, 2, s) for p in ("msg1", "upd1") for H in (32, 64) for s in DTYPES if SUPPORT[(p, H, 2)][1]]


@pytest.mark.parametrize("p,H,l,storage", NARROW, ids=[_id(*c) for c in NARROW])
def test_narrow_staging_of_whole_hidden_segments(p, H, l, storage):
    """Every segment as a misaligned column slice of a wider tensor: the lane-per-element staging branch (``!wide``) only
    moves data, so the result equals the aligned call bit for bit."""
    from scalable_e3_gnn_amd import ops
    mod = R.product(p, H, l, storage)
    inp = R.Inputs(p, H, l, storage, 17, seed=5 + H)
    sc = ops.pow2_scale(inp.tensors) if storage == "fp32" else None
    ref = _launch(mod, inp.segments(), inp.y(), True, in_scale=sc)
    views = {id(t): R.misaligned_copy(t) for t in inp.tensors}     # message #1 passes the same table twice
    mis = [views[id(t)] for t in inp.tensors]
    for v, t in zip(mis, inp.tensors):
        w = t.shape[1] if t.dim() == 2 else 1
        assert v.stride(0) == w + 2 and v.stride(1) == 1 and v.data_ptr() % 16 != 0
        assert (v.stride(0) * v.element_size()) % 16 != 0 and torch.equal(v.reshape(t.shape), t)
    got = _launch(mod, inp.segments(tensors=mis), inp.y(), True, in_scale=sc)
    assert torch.equal(got, ref)
    want = R.oracle(mod, H, True, *inp.dense())
    _check_blocks(mod, H, l, storage, True, got, want, _id(p, H, l, storage, True, 17) + "-narrow")


RESID = [("upd2", H, 2, s, B) for H in (64, 16) for s in DTYPES for B in (1, 17)]


@pytest.mark.parametrize("p,H,l,storage,B", RESID, ids=[_id(c[0], c[1], c[2], c[3], None, c[4]) for c in RESID])
def test_misaligned_residual_takes_the_generic_kernels_scalar_store(p, H, l, storage, B):
    """Hidden 64 / 16 have no pair kernel: update #2 adds the residual in the generic kernel, and a residual that is a
    misaligned column slice sends every tile through its element-wise store loop."""
    mod = R.product(p, H, l, storage)
    inp = R.Inputs(p, H, l, storage, B, seed=40 + B + H)
    g = torch.Generator().manual_seed(41 + B)
    res = (torch.randn(B, mod.out_dim, generator=g) * 5).to(DTYPES[storage]).to(DEV)
    mis = R.misaligned_copy(res)
    assert mis.stride(0) == mod.out_dim + 2 and mis.data_ptr() % 16 != 0 and torch.equal(mis, res)
    kw = {"out_scale": 10} if storage == "fp32" else {}
    got = _launch(mod, inp.segments(), inp.y(), False, residual=mis, **kw)
    ref = _launch(mod, inp.segments(), inp.y(), False, residual=res.clone(), **kw)
    if storage == "fp32":
        (got, sc), (ref, _) = got, ref
        s, inv, _ = expected_scale([got.cpu().numpy()], 10)
        assert (float(sc[0]), float(sc[1])) == (s, inv)
    assert torch.equal(got, ref)
    x, y = inp.dense()
    want = R.oracle(mod, H, False, x, y) + res.float().double().cpu().numpy()
    _check_blocks(mod, H, l, storage, False, got, want, _id(p, H, l, storage, False, B) + "-residual")


# ---- 4. epilogue extras at hidden 16 / 64 ----
EXTRAS = [(p, H, l, s) for p in ("upd2", "upd1", "embed") for H in (16, 64) for l in LMAX for s in DTYPES]


@pytest.mark.parametrize("p,H,l,storage", EXTRAS, ids=[_id(*c) for c in EXTRAS])
def test_epilogue_residual_and_scale(p, H, l, storage):
    """``out = product + residual`` and the operand scale of ``out`` in the product's epilogue, with the maximum planted
    in one element of the last, ragged tile (update #2: in the residual; the others: the row's inputs are 64 times larger)."""
    from scalable_e3_gnn_amd import ops
    B = 137
    r_max = B - 3                                   # tile 8 holds rows 128..136
    gate = p in GATED
    mod = R.product(p, H, l, storage)
    inp = R.Inputs(p, H, l, storage, B, seed=60 + H + l)
    if p != "upd2":
        for t in inp.tensors:
            t[r_max] *= 64
    sc_in = ops.pow2_scale(inp.tensors) if storage == "fp32" else None
    plain = _launch(mod, inp.segments(), inp.y(), gate, in_scale=sc_in)
    res = None
    if p == "upd2":
        g = torch.Generator().manual_seed(61)
        res = (torch.randn(tuple(plain.shape), generator=g) * 50).to(DTYPES[storage]).to(DEV)
        res[r_max, 7] = 7e3
    want = plain.float() + res.float() if res is not None else plain.float()
    amax = want.abs().max()
    assert int(want.abs().argmax()) // want.shape[1] == r_max     # the maximum is where it was planted
    got, sc = _launch(mod, inp.segments(), inp.y(), gate, in_scale=sc_in, residual=res, out_scale=10)
    if storage == "fp32":
        assert torch.equal(got, want)                               # the same fp32 add, in the epilogue
        ref = ops.pow2_scale([want], target_log2=10)
        assert float(sc[0]) == float(ref[0]) and float(sc[1]) == float(ref[1])
        assert float(sc[2].view(torch.int32).view(torch.float32)) == float(amax)
    elif res is not None:
        assert float((got.float() - want).abs().max()) <= 2.0 ** -7 * float(amax)   # one rounding of the fp32 sum
    else:
        assert torch.equal(got, plain)                              # the scale does not change what is stored
    if storage == "bf16":
        # the maximum is taken in fp32 before the store rounds it: within one bf16 rounding (2^-8) of max |stored|
        m = float(sc[2].view(torch.int32).view(torch.float32))
        assert abs(m - float(got.float().abs().max())) <= 2.0 ** -8 * m
        s, inv, _ = expected_scale([np.float32(m)], 10)
        assert (float(sc[0]), float(sc[1])) == (s, inv)


# ---- 5. nothing written outside the rows ----
CANARY = [(p, H, l, s) for (p, H) in (("upd1", 16), ("readout", 16), ("upd1", 64)) for l in (2, 1) for s in DTYPES]


@pytest.mark.parametrize("p,H,l,storage", CANARY, ids=[_id(*c) for c in CANARY])
def test_output_rows_with_padding_keep_the_canary(p, H, l, storage):
    """C ABI with an output of leading dimension width + 3 filled with a canary: the rows equal the contiguous call and
    every element between them is untouched (hidden 16 update #1: the 16-of-32-channel gated tile, where the compile-time
    width W and the channel count mask the store)."""
    from scalable_e3_gnn_amd import _lib, ops
    from scalable_e3_gnn_amd.tensor_product import TPSegment
    B = 17
    gate = p in GATED
    dt = DTYPES[storage]
    mod = R.product(p, H, l, storage)
    inp = R.Inputs(p, H, l, storage, B, seed=80 + H + l)
    sc = ops.pow2_scale(inp.tensors) if storage == "fp32" else None
    ref = _launch(mod, inp.segments(), inp.y(), gate, in_scale=sc)
    width = ref.shape[1]
    plan, ws, ns = R.plan_of(mod)
    assert width == (plan.gated_width() if gate else plan.out_dim)
    lib = _lib.load()
    packed = plan.packed(ws, ns, dt, ref.device)
    ld = width + 3
    buf = torch.full((B, ld), 7.0, device=DEV, dtype=dt)
    segs = (TPSegment * len(inp.tensors))()
    for i, t in enumerate(inp.tensors):
        segs[i].base, segs[i].ld, segs[i].ncols = t.data_ptr(), t.stride(0), t.shape[1]
    Y = inp.y()
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.e3_tp_forward_fused(plan.handle(ref.device), ctypes.byref(segs), len(inp.tensors), Y.data_ptr(),
                                       Y.stride(0), packed.data_ptr(), buf.data_ptr(), ld, B, _lib.dtype_code(dt),
                                       1 if gate else 0, sc.data_ptr() if sc is not None else None, stream),
               "e3_tp_forward_fused")
    torch.cuda.synchronize()
    assert _last_kernel() == R.KERNEL
    assert torch.equal(buf[:, :width], ref)
    assert bool((buf[:, width:] == 7.0).all())
    want = R.oracle(mod, H, gate, *inp.dense())
    _check_blocks(mod, H, l, storage, gate, buf[:, :width], want, _id(p, H, l, storage, gate, B) + "-padded")


# ---- 6. fused scatter ----
SCATTER_CASES = ("B1", "B17", "B211")


def test_scatter_arrays_have_the_cases():
    """host-side: the hand-made dst arrays hold what the run logic of the scatter epilogue branches on"""
    for case, B in zip(SCATTER_CASES, (1, 17, 211)):
        dst, deg = R.scatter_dst(case)
        assert len(dst) == B and dst.dtype == np.int32 and bool((np.diff(dst) >= 0).all())
        assert dst.min() >= 0 and dst.max() < R.SCATTER_NODES
    dst, deg = R.scatter_dst("B17")
    assert dst[15] == dst[16] and deg[39] == 0                           # a run across the tile edge, B just above 16
    dst, deg = R.scatter_dst("B211")
    start = np.concatenate([[0], np.cumsum(deg)[:-1]])
    end = start + deg
    assert deg[0] == 0 and deg[39] == 0                                  # isolated nodes at both ends
    assert any(deg[n] == 0 and deg[n + 1] == 0 for n in range(1, 38))    # two isolated nodes in a row
    assert any(deg[n] == 16 and start[n] % 16 == 0 for n in range(40))   # a run of exactly one tile, on a tile edge
    assert any(deg[n] > 0 and end[n] % 16 == 0 and start[n] % 16 != 0 and deg[n + 1] == 0 for n in range(39))
    assert any(deg[n] == 90 and start[n] // 64 != (end[n] - 1) // 64 for n in range(40))   # spans workgroups (64 rows)
    assert int((deg == 1).sum()) >= 3
    assert any(start[n] // 16 != (end[n] - 1) // 16 and deg[n] < 16 for n in range(40))    # a short run across a tile edge


SCATTER = [(l, case) for l in LMAX for case in SCATTER_CASES]


@pytest.mark.parametrize("l,case", SCATTER, ids=[f"msg2-H32-l{l}-fp32-gated-{case}" for l, case in SCATTER])
def test_fused_scatter_hand_made_runs(l, case):
    H = 32
    mod = R.product("msg2", H, l, "fp32")
    dst, deg = R.scatter_dst(case)
    B = len(dst)
    inp = R.Inputs("msg2", H, l, "fp32", B, seed=90 + B + l)
    with torch.no_grad():
        got = mod.forward_fused(inp.segments(), inp.y(), gate=True, scatter=(torch.as_tensor(dst).to(DEV), R.SCATTER_NODES))
    assert got is not None, "fused scatter kernel missing for message product #2 at hidden 32"
    assert _last_kernel() == R.KERNEL
    rows = R.oracle(mod, H, True, *inp.dense())
    want = np.zeros((R.SCATTER_NODES, rows.shape[1]))
    np.add.at(want, dst.astype(np.int64), rows)
    assert tuple(got.shape) == want.shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    assert float(got[torch.as_tensor(deg == 0).to(DEV)].abs().max()) == 0.0          # isolated nodes: exactly zero
    _check_blocks(mod, H, l, "fp32", True, got, want, f"msg2-H32-l{l}-scatter-{case}")


def test_no_scatter_kernel_returns_none():
    """bf16 storage and products without a fused-scatter instantiation: ``forward_fused(scatter=)`` returns None."""
    dst, _ = R.scatter_dst("B17")
    cases = [("msg2", 32, l, "bf16") for l in LMAX]
    cases += [(p, H, l, "fp32") for (p, H, l) in ALL if SUPPORT[(p, H, l)][1] and not (p == "msg2" and H == 32)]
    for p, H, l, storage in cases:
        inp = R.Inputs(p, H, l, storage, len(dst), seed=99)
        idx = torch.as_tensor(dst).to(DEV)
        with torch.no_grad():
            r = R.product(p, H, l, storage).forward_fused(inp.segments(), inp.y(), gate=True, scatter=(idx, R.SCATTER_NODES))
        assert r is None, (p, H, l, storage)

"""The edge / node stage kernels (csrc/e3_edge_ops.hip, csrc/e3_edge_bwd.hip, csrc/e3_edge_geometry_bwd.hip) against fp64 references at the shapes their code
branches on, PER BLOCK: max |got - want| / max |want| over the columns of one degree l (Y, A), of the scalars / the gates of a
block / a gated block (gate), of one structure (g_strain).  Graphs, references and bounds are in tests/edge_cases.py (checked on
the host by tests/test_edge_cases_host.py); DESIGN.md §4.5c has the table of which case stands for which branch.

Bounds (edge_cases.BOUND): 1e-6 for Y, d, A in every periodicity mode and under a strain, 1e-6 for the gates, the fp32 sums and
g_h, 2e-5 for g_pos and g_strain, 4.3e-6 for Y and A of positions moved by whole periods (twice what the fp32 expressions
themselves miss there, tests/test_edge_cases_host.py); bf16 sums elementwise |got - want| <= 2^-8 |want| + 1e-6 sum |m_e|.  Copies (gather, the
backward of the sum, g_extra) and structural zeros are compared exactly.  Lines that start with "EDGE " carry the figures."""
import ctypes

import numpy as np
import pytest
import torch

import edge_cases as E
import msg_cases as C
from scalable_e3_gnn_amd import _lib, ops
from scalable_e3_gnn_amd.radius_graph import radius_graph
from scalable_e3_gnn_amd.segnn import SEGNN

pytestmark = pytest.mark.gpu
DEV = C.DEV
INVALID = 1                                      # E3_ERR_INVALID_ARG
STRAINS = ("none", "S1", "S3")
GEOM = [(l, m, s) for l in (1, 2) for m in E.MODES for s in STRAINS]      # the 18 instantiations of each geometry kernel


def _ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(dtype).to(DEV)


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _widened(t, left=3, right=5, fill=float("nan")):
    """-> (a column slice equal to ``t`` of a wider tensor filled with ``fill``: row stride > width, the wider tensor)"""
    wide = torch.full((t.shape[0], left + t.shape[1] + right), fill, dtype=t.dtype, device=DEV)
    wide[:, left:left + t.shape[1]] = t.to(DEV)
    view = wide[:, left:left + t.shape[1]]
    assert view.stride(0) > view.shape[1] or view.shape[0] <= 1
    return view, wide


def _pad_untouched(wide, left, width, fill):
    pad = torch.cat([wide[:, :left], wide[:, left + width:]], 1)
    return bool(torch.isnan(pad).all()) if fill != fill else bool((pad == fill).all())


def _strain(kind):
    """-> (eps numpy [S,3,3] | None, structure numpy [80] | None)"""
    if kind == "none":
        return None, None
    return (E.strain_of(1), None) if kind == "S1" else (E.strain_of(3), E.structure_s3())


def _report(tag, names, errs, bounds):
    print(f"EDGE {tag}: " + " | ".join(f"{n} " + " ".join(f"{e:.2e}" for e in es) for n, es in zip(names, errs)))
    for n, es, b in zip(names, errs, bounds):
        for k, e in enumerate(es):
            assert e < b, (tag, n, k, e, b)


# ---- geometry, forward -----------------------------------------------------------------------------------------------
def _check_forward(tag, got, want, lmax, rowptr, key=None):
    """``key``: None, "strained" or "unwrapped" (edge_cases.BOUND; d keeps its own bound on unwrapped positions)"""
    (Y, d, A), (Yw, dw, Aw) = got, want
    names, errs, bounds = [], [], []
    if Y is not None:
        assert Y.dtype == torch.float32 and tuple(Y.shape) == Yw.shape and tuple(d.shape) == dw.shape
        names += ["Y", "d"]
        errs += [E.block_errors(Y, Yw, E.sh_blocks(lmax)), E.block_errors(d, dw)]
        bounds += [E.BOUND[key or "Y"], E.BOUND["strained" if key == "strained" else "d"]]
        assert bool((Y[:, 0] == 1).all()), tag
        same = torch.as_tensor(dw == 0).to(DEV)
        if bool(same.any()):                                               # coincident nodes: d = 0, no harmonic above l = 0
            assert float(d[same].abs().max()) == 0.0 and float(Y[same][:, 1:].abs().max()) == 0.0, tag
    names.append("A")
    errs.append(E.block_errors(A, Aw, E.sh_blocks(lmax)))
    bounds.append(E.BOUND[key or "A"])
    assert bool((A[:, 0] == 1).all()), tag
    empty = torch.as_tensor(np.diff(rowptr) == 0).to(DEV)
    if bool(empty.any()):
        assert float(A[empty][:, 1:].abs().max()) == 0.0, tag             # empty rows: exactly [1, 0, ...]
    _report(tag, names, errs, bounds)


def _forward_case(name, mode, lmax, kind, pos=None, want_edge=True):
    rowptr, src, dst = E.edges(name)
    g = E.graph(name, mode)
    eps, sid = _strain(kind)
    stored = E.positions_of(name) if pos is None else pos
    kw = {}
    if eps is not None:
        kw.update(strain=_dev(eps), structure=None if sid is None else _dev(sid, torch.int64))
    if pos is not None:
        kw["pos"] = _dev(pos)
    got = ops.edge_geometry(g, lmax=lmax, want_edge=want_edge, **kw)
    if not want_edge:
        assert got[0] is None and got[1] is None
    want = E.geometry(lmax, mode, stored, rowptr, src, dst, eps, sid)
    _check_forward(f"forward {name} lmax{lmax} {mode} {kind}" + ("" if want_edge else " node attribute only") +
                   ("" if pos is None else " unwrapped"), got, want, lmax, rowptr,
                   "unwrapped" if pos is not None else ("strained" if eps is not None else None))


@pytest.mark.parametrize("lmax,mode,kind", GEOM, ids=_ids(GEOM))
def test_geometry_forward(lmax, mode, kind):
    _forward_case("A", mode, lmax, kind)
    if kind == "none":
        _forward_case("B", mode, lmax, kind)


@pytest.mark.parametrize("mode", E.MODES)
def test_geometry_forward_node_attribute_only(mode):
    for lmax in (1, 2):
        _forward_case("A", mode, lmax, "none", want_edge=False)
    _forward_case("A", mode, 2, "S3", want_edge=False)


@pytest.mark.parametrize("mode", ["box", "cell"])
def test_geometry_forward_unwrapped_positions(mode):
    for lmax in (1, 2):
        _forward_case("A", mode, lmax, "none", pos=E.lattice_shifted(mode))
    _forward_case("A", mode, 2, "S1", pos=E.lattice_shifted(mode))


@pytest.mark.parametrize("lmax", [1, 2])
def test_geometry_forward_more_rows_than_one_grid_pass(lmax):
    assert E.N_W > E.ROWS_PER_PASS
    _forward_case("W", "open", lmax, "none")
    _forward_case("W", "open", lmax, "S1")


# ---- geometry, backward ----------------------------------------------------------------------------------------------
def _backward_direct(g, lmax, eps_t, sid_t, gY, gd, gA):
    """the library entry as ops._EdgeGeometryFn.backward calls it, with NULL for the upstream gradients that are None"""
    lib = _lib.load()
    N = g.pos4.shape[0]
    p = lambda t: t.data_ptr() if t is not None else None
    gpos = torch.full((N, 3), float("nan"), device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    head = (g.pos4.data_ptr(), g.rowptr.data_ptr(), g.src.data_ptr(), N, lmax)
    if eps_t is not None:
        gstrain = torch.full_like(eps_t, float("nan"))
        ws = torch.empty(max(1, lib.e3_edge_geometry_backward_strained_workspace_bytes(N)), dtype=torch.uint8, device=DEV)
        name = "e3_edge_geometry_backward_strained" + ("_cell" if g.cell is not None else "")
        _lib.check(getattr(lib, name)(*head, g.cell_arg if g.cell is not None else g.box_arg, eps_t.data_ptr(), p(sid_t),
                                      eps_t.shape[0], p(gY), p(gd), p(gA), gpos.data_ptr(), gstrain.data_ptr(), ws.data_ptr(),
                                      ws.numel(), stream), name)
        return gpos, gstrain
    if g.cell is not None:
        _lib.check(lib.e3_edge_geometry_backward_cell(*head, g.cell_arg, p(gY), p(gd), p(gA), gpos.data_ptr(), stream), "cell")
    elif g.box is not None:
        _lib.check(lib.e3_edge_geometry_backward_pbc(*head, g.box_arg, p(gY), p(gd), p(gA), gpos.data_ptr(), stream), "pbc")
    else:
        _lib.check(lib.e3_edge_geometry_backward(*head, p(gY), p(gd), p(gA), gpos.data_ptr(), stream), "open")
    return gpos, None


def _check_backward(tag, name, gpos, gstrain, want_pos, want_strain):
    assert bool(torch.isfinite(gpos).all()), tag
    free = torch.as_tensor(E.untouched_rows(name)).to(DEV)
    if bool(free.any()):
        assert float(gpos[free].abs().max()) == 0.0, tag                  # no edge in or out: exactly no force
    names, errs, bounds = ["g_pos"], [E.block_errors(gpos, want_pos)], [E.BOUND["g_pos"]]
    if want_strain is not None:
        assert bool(torch.isfinite(gstrain).all()), tag
        names.append("g_strain")
        errs.append(E.structure_errors(gstrain, want_strain))
        bounds.append(E.BOUND["g_strain"])
    _report(tag, names, errs, bounds)


def _backward_case(name, mode, lmax, kind, paths=True):
    rowptr, src, dst = E.edges(name)
    n, ne, ny = len(rowptr) - 1, len(src), (lmax + 1) ** 2
    g, pos = E.graph(name, mode), E.positions_of(name)
    eps, sid = _strain(kind)
    if sid is not None and n != C.N:
        sid = None
    gY, gd, gA = _randn((ne, ny), 21).to(DEV), _randn((ne,), 22).to(DEV), _randn((n, ny), 23).to(DEV)
    tag = f"backward {name} lmax{lmax} {mode} {kind}"
    # all three upstream gradients at once, through ops
    pos_t = _dev(pos).requires_grad_()
    eps_t = None if eps is None else _dev(eps).requires_grad_()
    sid_t = None if sid is None else _dev(sid, torch.int32)
    outs = ops.edge_geometry(g, lmax=lmax, pos=pos_t, strain=eps_t, structure=sid_t)
    grads = torch.autograd.grad(outs, [pos_t] + ([eps_t] if eps_t is not None else []), [gY, gd, gA])
    want = E.geometry_grads(lmax, mode, pos, rowptr, src, dst, gY, gd, gA, eps, sid)
    _check_backward(tag + " all", name, grads[0], grads[1] if eps_t is not None else None, *want)
    if eps_t is not None and eps_t.shape[0] == 1:                          # S = 1: a fixed order of every sum
        again = torch.autograd.grad(ops.edge_geometry(g, lmax=lmax, pos=pos_t, strain=eps_t), [eps_t], [gY, gd, gA])
        assert torch.equal(again[0], grads[1]), tag
    if not paths:
        return
    # each path alone, NULL for the others, through the library entry
    eps_d = None if eps is None else _dev(eps)
    for which, trio in (("gY", (gY, None, None)), ("gd", (None, gd, None)), ("gA", (None, None, gA))):
        gpos, gstrain = _backward_direct(g, lmax, eps_d, sid_t, *trio)
        want = E.geometry_grads(lmax, mode, pos, rowptr, src, dst, *trio, eps, sid)
        _check_backward(f"{tag} {which} only", name, gpos, gstrain, *want)


@pytest.mark.parametrize("lmax,mode,kind", GEOM, ids=_ids(GEOM))
def test_geometry_backward(lmax, mode, kind):
    _backward_case("A", mode, lmax, kind)
    _backward_case("B", mode, lmax, kind, paths=False)                     # B has rows that no edge touches


@pytest.mark.parametrize("name", ["Wcut", "W"])
def test_geometry_backward_strained_partials(name):
    """S = 1 on 4400 rows (1100 partials: one 16 x 64 trip and both tail trips of strain_partial_sum_kernel) and on 16403 rows
    (4096 partials, rows beyond one grid pass)"""
    assert E.wave_grid(len(E.edges(name)[0]) - 1) == {"Wcut": 1100, "W": 4096}[name]
    for lmax in (1, 2):
        _backward_case(name, "open", lmax, "S1", paths=False)
    _backward_case(name, "open", 2, "none", paths=False)


# ---- gather_concat ---------------------------------------------------------------------------------------------------
GATHER = [(D, nx) for D in (1, 20, 64, 65, 130) for nx in (0, 1, 3, 64)]


def _gather_case(name, D, nx):
    rowptr, src, dst = E.edges(name)
    n, ne = len(rowptr) - 1, len(src)
    g = E.graph(name)
    tag = f"gather {name} D{D} extra{nx}"
    h, _ = _widened(_randn((n, D), 31))
    extra = _randn((ne, nx), 32).to(DEV) if nx else None
    assert h.stride(0) > D
    out = ops.gather_concat(h, g, extra)
    want = E.gather(h, src, dst, extra)
    assert tuple(out.shape) == (ne, 2 * D + nx) and np.array_equal(out.double().cpu().numpy(), want), tag
    # backward: only the h[dst] half of gm, only the h[src] half, both
    gm_full = _randn((ne, 2 * D + nx), 33)
    touched = np.zeros(n, bool)
    touched[src], touched[dst] = True, True
    for half in ("dst", "src", "both"):
        gm = gm_full.clone()
        if half == "dst":
            gm[:, D:2 * D] = 0
        elif half == "src":
            gm[:, :D] = 0
        gm = gm.to(DEV)
        h_t = h.detach().requires_grad_()
        x_t = extra.detach().requires_grad_() if nx else None
        grads = torch.autograd.grad(ops.gather_concat(h_t, g, x_t), [h_t] + ([x_t] if nx else []), gm)
        wh, wx = E.gather_grads(gm, D, src, dst, n)
        _report(f"{tag} backward {half}", ["g_h"], [E.block_errors(grads[0], wh)], [E.BOUND["g_h"]])
        assert float(grads[0][torch.as_tensor(~touched).to(DEV)].abs().sum()) == 0.0, tag   # rows no edge touches
        if nx:
            assert np.array_equal(grads[1].double().cpu().numpy().reshape(ne, nx), wx), tag


@pytest.mark.parametrize("D,nx", GATHER, ids=_ids(GATHER))
def test_gather_concat(D, nx):
    for name in ("A", "B"):
        _gather_case(name, D, nx)


def test_gather_concat_more_rows_than_one_grid_pass():
    _gather_case("W", 8, 1)


@pytest.mark.parametrize("D,nx", [(20, 3), (65, 0)])
def test_gather_concat_backward_row_stride_of_g_h(D, nx):
    """ld_gh = D + 3 and a strided gm, the library entry called directly: the pad columns keep their sentinel"""
    rowptr, src, dst = E.edges("A")
    n, ne = len(rowptr) - 1, len(src)
    g = E.graph("A")
    gm, _ = _widened(_randn((ne, 2 * D + nx), 34))
    gh_wide = torch.full((n, D + 3), -7.25, device=DEV)
    gx = torch.full((ne, max(nx, 1)), float("nan"), device=DEV)
    _lib.check(_lib.load().e3_gather_concat_backward(gm.data_ptr(), gm.stride(0), D, g.rowptr.data_ptr(), g.src.data_ptr(), n, nx,
                                                     gh_wide.data_ptr(), D + 3, gx.data_ptr() if nx else None,
                                                     torch.cuda.current_stream().cuda_stream), "e3_gather_concat_backward")
    wh, wx = E.gather_grads(gm, D, src, dst, n)
    assert bool((gh_wide[:, D:] == -7.25).all())
    _report(f"gather ld_gh D{D}", ["g_h"], [E.block_errors(gh_wide[:, :D], wh)], [E.BOUND["g_h"]])
    if nx:
        assert np.array_equal(gx.double().cpu().numpy(), wx)


# ---- gates -----------------------------------------------------------------------------------------------------------
EIGHT = ((0, 3), (1, 2), (2, 0), (2, 1), (1, 0), (0, 1), (1, 5), (2, 4))
GATE_ROWS = (1, 255, 257)


def _gate_inputs(B, ns, blocks, seed, extreme=False):
    wi, wo = E.gate_width(ns, blocks)
    x = _randn((B, wi), seed).clamp(-4, 4)
    if extreme:                                                            # saturated scalars and gates
        ng = wi - wo
        vals = torch.tensor([30.0, -30.0, 100.0, -100.0])
        for c in range(ns + ng):
            x[c % B, c] = vals[c % 4]
    return x, _randn((B, wo), seed + 1)


def _gate_case(B, ns, blocks, plain=None, extreme=False):
    """forward without and with a gradient through ops, the backward through autograd and through the library entry with every
    row stride above its width.  ``plain`` = nv: the case also runs ops.gate / e3_gate."""
    blocks = tuple(blocks)
    wi, wo = E.gate_width(ns, blocks)
    tag = f"gate B{B} ns{ns} {blocks}" + (" extreme" if extreme else "")
    x_cpu, go_cpu = _gate_inputs(B, ns, blocks, 41 + B, extreme)
    x, _ = _widened(x_cpu)
    go, _ = _widened(go_cpu, 2, 1)
    want = E.gate_blocks(x_cpu.double().numpy(), ns, blocks)
    want_g = E.gate_blocks_grad(x_cpu, go_cpu, ns, blocks)
    ob, ib = E.gate_out_blocks(ns, blocks), E.gate_in_blocks(ns, blocks)
    outs = {"gate_blocks": ops.gate_blocks(x, ns, blocks)}
    x_t = x.detach().requires_grad_()
    y_t = ops.gate_blocks(x_t, ns, blocks)
    outs["gate_blocks with grad"] = y_t.detach()
    if plain is not None:
        assert blocks == ((1, plain),)
        outs["gate"] = ops.gate(x, ns, plain)
        x_p = x.detach().requires_grad_()
        y_p = ops.gate(x_p, ns, plain)                                     # runs _GateBlocksFn
        assert y_p.grad_fn is not None and torch.equal(y_p.detach(), outs["gate_blocks with grad"]), tag
        (g_p,) = torch.autograd.grad(y_p, x_p, go)
    for k, got in outs.items():
        assert tuple(got.shape) == (B, wo) and bool(torch.isfinite(got).all()), (tag, k)
        _report(f"{tag} {k}", ["out"], [E.block_errors(got, want, ob)], [E.BOUND["gate"]])
    (g_auto,) = torch.autograd.grad(y_t, x_t, go)
    # the library entry with strided in, g_out and g_in
    gi_wide = torch.full((B, wi + 4), -7.25, device=DEV)
    ls = (ctypes.c_int32 * len(blocks))(*[l for l, _ in blocks])
    ms = (ctypes.c_int32 * len(blocks))(*[m for _, m in blocks])
    _lib.check(_lib.load().e3_gate_blocks_backward(x.data_ptr(), x.stride(0), go.data_ptr(), go.stride(0), gi_wide.data_ptr(),
                                                   wi + 4, B, ns, len(blocks), ls, ms,
                                                   torch.cuda.current_stream().cuda_stream), "e3_gate_blocks_backward")
    assert bool((gi_wide[:, wi:] == -7.25).all()), tag
    grads = {"autograd": g_auto, "strided": gi_wide[:, :wi]}
    if plain is not None:
        grads["ops.gate"] = g_p
    for k, got in grads.items():
        assert tuple(got.shape) == (B, wi) and bool(torch.isfinite(got).all()), (tag, k)
        _report(f"{tag} backward {k}", ["g_in"], [E.block_errors(got, want_g, ib)], [E.BOUND["gate"]])


@pytest.mark.parametrize("B", GATE_ROWS)
@pytest.mark.parametrize("ns,nv", [(8, 8), (0, 5), (7, 0), (3, 2)])
def test_gate(ns, nv, B):
    _gate_case(B, ns, ((1, nv),), plain=nv)


def _gate_blocks_cases():
    return [(4, ((1, 2), (2, 2))), (0, EIGHT), (5, EIGHT), E.layer_gate_shape(32, 2), E.layer_gate_shape(16, 1)]


@pytest.mark.parametrize("B", GATE_ROWS)
@pytest.mark.parametrize("case", range(5))
def test_gate_blocks(case, B):
    ns, blocks = _gate_blocks_cases()[case]
    _gate_case(B, ns, blocks)


def test_gate_blocks_grid_wrap():
    """4099 rows of the (32, 2) layer's gate: forward and backward have more than 2^20 elements"""
    ns, blocks = E.layer_gate_shape(32, 2)
    wi, wo = E.gate_width(ns, blocks)
    assert 4099 * wo > 2 ** 20 and 4099 * wi > 2 ** 20
    _gate_case(4099, ns, blocks)


def test_gate_saturated_inputs():
    _gate_case(257, 5, EIGHT, extreme=True)
    _gate_case(255, 8, ((1, 8),), plain=8, extreme=True)


# ---- segment sum -----------------------------------------------------------------------------------------------------
def _segment_case(name, D):
    rowptr, src, dst = E.edges(name)
    n, ne = len(rowptr) - 1, len(src)
    g = E.graph(name)
    tag = f"segment_sum {name} D{D}"
    empty = torch.as_tensor(np.diff(rowptr) == 0).to(DEV)
    msg, _ = _widened(_randn((ne, D), 51))
    agg = ops.segment_sum(msg, g)
    assert tuple(agg.shape) == (n, D) and float(agg[empty].abs().max()) == 0.0, tag
    assert torch.equal(agg, ops.segment_sum(msg, g)), tag
    _report(tag, ["sum"], [E.block_errors(agg, E.segment_sum(msg, dst, n))], [E.BOUND["sum"]])
    # bf16 storage, elementwise against the fp64 sum of the bf16 values
    mb, _ = _widened(_randn((ne, D), 52).to(torch.bfloat16), 2, 4)
    ab = ops.segment_sum(mb, g)
    assert ab.dtype == torch.bfloat16 and tuple(ab.shape) == (n, D) and torch.equal(ab, ops.segment_sum(mb, g)), tag
    want, slack = E.segment_sum(mb, dst, n), E.segment_abs_sum(mb, dst, n)
    err, bound = np.abs(E.f64(ab) - want), E.BF16_REL * np.abs(want) + E.BF16_ABS * slack
    print(f"EDGE {tag} bf16: worst error / elementwise bound {(err[bound > 0] / bound[bound > 0]).max():.2f}")
    assert bool((err <= bound).all()) and float(ab[empty].float().abs().max()) == 0.0, tag
    # backward: a copy of g_agg[dst], every edge row written
    ga, _ = _widened(_randn((n, D), 53))
    m_t = msg.detach().requires_grad_()
    (gm,) = torch.autograd.grad(ops.segment_sum(m_t, g), m_t, ga)
    assert np.array_equal(E.f64(gm), E.f64(ga)[dst]), tag
    gm_wide = torch.full((ne, D + 2), float("nan"), device=DEV)
    _lib.check(_lib.load().e3_segment_sum_backward(ga.data_ptr(), ga.stride(0), g.rowptr.data_ptr(), n, D, gm_wide.data_ptr(),
                                                   D + 2, torch.cuda.current_stream().cuda_stream), "e3_segment_sum_backward")
    assert np.array_equal(E.f64(gm_wide[:, :D]), E.f64(ga)[dst]) and bool(torch.isnan(gm_wide[:, D:]).all()), tag


@pytest.mark.parametrize("D", [1, 63, 64, 65, 288])
def test_segment_sum(D):
    for name in ("A", "B"):
        _segment_case(name, D)


def test_segment_sum_more_rows_than_one_grid_pass():
    _segment_case("W", 8)


# ---- a graph without edges -------------------------------------------------------------------------------------------
def _empty_graph():
    pos = torch.rand(50, 3, generator=torch.Generator().manual_seed(1))
    g = radius_graph(pos.to(DEV), 1e-4, [0, 0, 0], [1, 1, 1])
    assert g.num_edges == 0
    return g


@pytest.mark.parametrize("grad", [False, True])
def test_empty_graph_ops(grad):
    g = _empty_graph()
    e0 = torch.zeros(50, 9, device=DEV)
    e0[:, 0] = 1
    for lmax in (1, 2):
        ny = (lmax + 1) ** 2
        pos = g.pos4[:, :3].clone().requires_grad_(grad)
        Y, d, A = ops.edge_geometry(g, lmax=lmax, pos=pos)
        assert tuple(Y.shape) == (0, ny) and tuple(d.shape) == (0,) and torch.equal(A, e0[:, :ny])
        if grad:
            (gp,) = torch.autograd.grad([Y.sum() + d.sum() + (A * A).sum()], [pos])
            assert tuple(gp.shape) == (50, 3) and float(gp.abs().max()) == 0.0
        eps = _dev(E.strain_of(1)).requires_grad_(grad)
        Ys, ds, As = ops.edge_geometry(g, lmax=lmax, strain=eps)
        assert tuple(Ys.shape) == (0, ny) and tuple(ds.shape) == (0,) and torch.equal(As, e0[:, :ny])
        if grad:
            (ge,) = torch.autograd.grad([Ys.sum() + ds.sum() + (As * As).sum()], [eps])
            assert tuple(ge.shape) == (1, 3, 3) and float(ge.abs().max()) == 0.0
        assert ops.edge_geometry(g, lmax=lmax, want_edge=False)[0] is None
    for D, nx in ((20, 0), (65, 1)):
        h = torch.randn(50, D, device=DEV, requires_grad=grad)
        extra = torch.zeros(0, nx, device=DEV, requires_grad=grad) if nx else None
        m = ops.gather_concat(h, g, extra)
        assert tuple(m.shape) == (0, 2 * D + nx)
        if grad:
            assert m.requires_grad
            (gh,) = torch.autograd.grad(m.sum(), h)
            assert tuple(gh.shape) == (50, D) and float(gh.abs().max()) == 0.0
        msg = torch.zeros(0, D, device=DEV, requires_grad=grad)
        agg = ops.segment_sum(msg, g)
        assert tuple(agg.shape) == (50, D) and agg.dtype == torch.float32 and float(agg.detach().abs().max()) == 0.0
        if grad:
            (gmsg,) = torch.autograd.grad(agg.sum(), msg)
            assert tuple(gmsg.shape) == (0, D)
        ab = ops.segment_sum(torch.zeros(0, D, device=DEV, dtype=torch.bfloat16), g)
        assert tuple(ab.shape) == (50, D) and ab.dtype == torch.bfloat16 and float(ab.float().abs().max()) == 0.0


@pytest.mark.parametrize("grad", [False, True])
@pytest.mark.parametrize("lmax", [1, 2])
def test_empty_graph_model_on_the_unfused_chain(lmax, grad):
    g = _empty_graph()
    torch.manual_seed(7)
    model = SEGNN("1x0e+1x1o", 16, "1x1o", 1, lmax=lmax).to(DEV)
    for layer in model.layers:
        layer.fused = False
    x = torch.randn(50, 4, device=DEV)
    if grad:
        out = model(x, g)
        grads = torch.autograd.grad(out.sum(), [p for p in model.parameters() if p.requires_grad], allow_unused=True)
        assert all(bool(torch.isfinite(t).all()) for t in grads if t is not None)
    else:
        with torch.no_grad():
            out = model(x, g)
    assert tuple(out.shape) == (50, 3) and bool(torch.isfinite(out).all())


# ---- refusals: decided on the host, nothing is launched and nothing written ---------------------------------------------
def test_refusals():
    lib = _lib.load()
    rowptr, src, _ = E.edges("A")
    n, ne = len(rowptr) - 1, len(src)
    g = E.graph("A")
    stream = torch.cuda.current_stream().cuda_stream
    SENT = -7.25
    out = torch.full((ne, 400), SENT, device=DEV)
    inp = torch.randn(max(ne, n), 400, device=DEV)
    rp, sr, o, i = g.rowptr.data_ptr(), g.src.data_ptr(), out.data_ptr(), inp.data_ptr()
    one = (ctypes.c_int32 * 1)
    nine = (ctypes.c_int32 * 9)
    ws_bytes = lib.e3_edge_geometry_backward_strained_workspace_bytes(n)
    assert ws_bytes == E.wave_grid(n) * 9 * 4
    ws = torch.full((ws_bytes,), 7, dtype=torch.uint8, device=DEV)
    eps = torch.zeros(1, 3, 3, device=DEV)
    gpos, gstrain = torch.full((n, 3), SENT, device=DEV), torch.full((1, 3, 3), SENT, device=DEV)

    def strained_bwd(lmax, S_, nbytes, cell=False):
        name = "e3_edge_geometry_backward_strained" + ("_cell" if cell else "")
        box = E.graph("A", "cell").cell_arg if cell else None
        return getattr(lib, name)(g.pos4.data_ptr(), rp, sr, n, lmax, box, eps.data_ptr(), None, S_, i, None, None,
                                  gpos.data_ptr(), gstrain.data_ptr(), ws.data_ptr(), nbytes, stream)

    cases = {
        "gather n_extra 65": lib.e3_gather_concat(i, 400, 8, rp, sr, n, i, 65, o, 400, stream),
        "gather ld_out": lib.e3_gather_concat(i, 400, 8, rp, sr, n, i, 3, o, 18, stream),
        "gather D 0": lib.e3_gather_concat(i, 400, 0, rp, sr, n, i, 3, o, 400, stream),
        "gather backward n_extra 65": lib.e3_gather_concat_backward(i, 400, 8, rp, sr, n, 65, o, 400, o, stream),
        "gather backward D 0": lib.e3_gather_concat_backward(i, 400, 0, rp, sr, n, 1, o, 400, o, stream),
        "gate ld_in": lib.e3_gate(i, 8 + 4 * 8 - 1, o, 400, ne, 8, 8, stream),
        "gate_blocks 9 blocks": lib.e3_gate_blocks(i, 400, o, 400, ne, 4, 9, nine(*[1] * 9), nine(*[1] * 9), stream),
        "gate_blocks l 3": lib.e3_gate_blocks(i, 400, o, 400, ne, 4, 1, one(3), one(2), stream),
        "gate_blocks mul < 0": lib.e3_gate_blocks(i, 400, o, 400, ne, 4, 1, one(1), one(-1), stream),
        "gate_blocks backward 9 blocks": lib.e3_gate_blocks_backward(i, 400, i, 400, o, 400, ne, 4, 9, nine(*[1] * 9),
                                                                     nine(*[1] * 9), stream),
        "gate_blocks backward l 3": lib.e3_gate_blocks_backward(i, 400, i, 400, o, 400, ne, 4, 1, one(3), one(2), stream),
        "segment_sum ld_msg": lib.e3_segment_sum(i, 7, rp, n, 8, o, 400, stream),
        "segment_sum_bf16 ld_msg": lib.e3_segment_sum_bf16(i, 7, rp, n, 8, o, 400, stream),
        "segment_sum backward ld": lib.e3_segment_sum_backward(i, 7, rp, n, 8, o, 400, stream),
        "strained backward lmax 3": strained_bwd(3, 1, ws_bytes),
        "strained backward S 0": strained_bwd(2, 0, ws_bytes),
        "strained backward workspace": strained_bwd(2, 1, ws_bytes - 1),
        "strained cell backward lmax 3": strained_bwd(3, 1, ws_bytes, True),
        "strained cell backward S 0": strained_bwd(2, 0, ws_bytes, True),
        "strained cell backward workspace": strained_bwd(2, 1, ws_bytes - 1, True),
    }
    torch.cuda.synchronize()
    for what, status in cases.items():
        assert status == INVALID, (what, status)
    for t in (out, gpos, gstrain):
        assert bool((t == SENT).all())
    assert bool((ws == 7).all())


def test_gate_blocks_entries_share_their_refusals():
    """e3_gate_blocks, e3_gate_blocks_backward and e3_gate_blocks_backward2 validate one block descriptor the same way: each
    invalid descriptor, and each leading dimension one below its minimum, is E3_ERR_INVALID_ARG from all three with nothing
    written; B = 0 and a valid call are E3_OK.  Blocks [(l=1, mul=2), (l=2, mul=1)], ns = 3: 3 gates, output width W = 14,
    input width W + 3 = 17."""
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    B, ns, W, WI = 2, 3, 14, 17
    SENT = -7.25
    x, go, ct = torch.randn(B, WI, device=DEV), torch.randn(B, W, device=DEV), torch.randn(B, WI, device=DEV)
    out, gin = torch.full((B, W), SENT, device=DEV), torch.full((B, WI), SENT, device=DEV)
    cgo, cin = torch.full((B, W), SENT, device=DEV), torch.full((B, WI), SENT, device=DEV)
    arr = lambda v: (ctypes.c_int32 * len(v))(*v)
    good = (ns, 2, arr([1, 2]), arr([2, 1]))

    def forward(desc, b=B, ld_in=WI, ld_out=W):
        return lib.e3_gate_blocks(x.data_ptr(), ld_in, out.data_ptr(), ld_out, b, *desc, stream)

    def backward(desc, b=B, ld_in=WI, ld_gout=W, ld_gin=WI):
        return lib.e3_gate_blocks_backward(x.data_ptr(), ld_in, go.data_ptr(), ld_gout, gin.data_ptr(), ld_gin, b, *desc, stream)

    def backward2(desc, b=B, ld_in=WI, ld_gout=W, ld_c=WI, ld_cgout=W, ld_cin=WI):
        return lib.e3_gate_blocks_backward2(x.data_ptr(), ld_in, go.data_ptr(), ld_gout, ct.data_ptr(), ld_c, cgo.data_ptr(),
                                            ld_cgout, cin.data_ptr(), ld_cin, b, *desc, stream)

    bad = {"nblocks 9": (ns, 9, arr([1] * 9), arr([1] * 9)), "l 3": (ns, 1, arr([3]), arr([2])),
           "mul -1": (ns, 1, arr([1]), arr([-1])), "ns -1": (-1, 2, arr([1, 2]), arr([2, 1])),
           "ls NULL": (ns, 1, None, arr([2]))}
    refused = {}
    for what, desc in bad.items():
        for entry in (forward, backward, backward2):
            refused[f"{entry.__name__} {what}"] = entry(desc)
    for entry, lds in ((forward, {"ld_in": WI, "ld_out": W}), (backward, {"ld_in": WI, "ld_gout": W, "ld_gin": WI}),
                       (backward2, {"ld_in": WI, "ld_gout": W, "ld_c": WI, "ld_cgout": W, "ld_cin": WI})):
        for name, least in lds.items():
            refused[f"{entry.__name__} {name} {least - 1}"] = entry(good, **{name: least - 1})
    torch.cuda.synchronize()
    for what, status in refused.items():
        assert status == INVALID, (what, status)
    for t in (out, gin, cgo, cin):
        assert bool((t == SENT).all())
    for entry in (forward, backward, backward2):
        assert entry(good, b=0) == 0, entry.__name__
    torch.cuda.synchronize()
    for t in (out, gin, cgo, cin):
        assert bool((t == SENT).all())
    for entry in (forward, backward, backward2):
        assert entry(good) == 0, entry.__name__
    torch.cuda.synchronize()
    for t in (out, gin, cgo, cin):
        assert bool(torch.isfinite(t).all()) and not bool((t == SENT).any())

"""The strained second-derivative kernels of the edge geometry (e3_edge_geometry_jvp_strained / e3_edge_geometry_hvp_strained,
open / box / cell, l_max 1 / 2, S = 1 / 3) through ``ops.edge_geometry(strain=)`` under ``create_graph`` and through the raw
entries, against fp64 torch autograd of the same geometry written in torch with the lattice shift a constant -- the strained
counterpart of tests/test_hessian_ops_gpu.py, on that file's cloud and ``graph()`` (N = 149, r = 0.15: rows of 99 edges, 17
empty rows, one coincident pair, every face crossed in box and cell mode).

With phi = <sY, Y> + <sd, d> + <sA, A> of the strained geometry (r' = r + eps_s r, s the structure of the dst row),
g_pos = dphi/dpos and G = dphi/deps, every case forms L = <v, g_pos> + <Xi, G> (both cotangents, v alone, Xi alone) and compares
  h_pos = dL/dpos,  h_strain = dL/deps,  the tangents dY = dL/dsY, dd = dL/dsd, dA = dL/dsA.
eps is zero or a fixed NON-symmetric matrix of magnitude 0.05 with fp32-exact entries (S = 3: three different ones), Xi is
non-symmetric too: a transposed M = I + eps or Xi, or r in place of r' in any formula, changes every output far beyond the
bound.  S = 3 uses random structure ids, with five rows (rows with edges among them) given the ids -1 and 3: they are computed
unstrained and add nothing to h_strain -- the torch reference masks them in the same way.

Norm: max |got - want| / max |want| per tensor.  Bound: max(2e-5, 20 x yardstick), the yardstick being the SAME torch
expression evaluated in fp32 on the CPU against fp64, computed by every case itself for every tensor -- 2e-5 is the project's
bound for derivatives of fp32 kernels and 20 about the margin it keeps (tests/test_hessian_ops_gpu.py,
tests/test_force_loss_gpu.py).

Measured on one MI355X (the worse of autograd and entry / yardstick, over the 24 cases of a mode): h_pos open 2.1e-7 .. 4.7e-7 /
1.4e-7 .. 5.0e-7, box 5.9e-7 .. 1.2e-6 / 5.5e-7 .. 1.2e-6, cell 6.4e-7 .. 2.3e-6 / 6.0e-7 .. 2.2e-6; h_strain open 8.7e-8 .. 3.4e-7 /
1.7e-7 .. 6.0e-7, box 2.9e-7 .. 1.0e-6 / 2.6e-7 .. 1.0e-6, cell 2.8e-7 .. 1.4e-6 / 3.2e-7 .. 1.6e-6; the tangents 7e-8 .. 2.8e-6 /
8e-8 .. 2.8e-6: at most 6 % of the bound (the table in DESIGN.md 4.6, "Strain second derivatives").  Without the feature every
comparison fails: the second derivative through a strained geometry raises NotImplementedError and the four entries do not exist."""
import functools

import numpy as np
import pytest
import torch

import models  # noqa: F401
import triclinic_reference as TR
from oracle.segnn_oracle import sh_component_torch
from scalable_e3_gnn_amd import _lib, ops
from test_hessian_ops_gpu import BOX, DEV, MODES, N, N_ISOLATED, cloud, graph

pytestmark = pytest.mark.gpu
EPS = np.array([[0.046875, -0.03125, 0.015625], [0.0234375, -0.05078125, 0.0390625], [-0.0078125, 0.02734375, 0.03515625]])
COTS = ("both", "v", "xi")
OUT_OF_RANGE = {3: -1, 40: -1, 77: 3, 101: 3, 120: -1}      # row -> structure id outside [0, 3)
NAMES = ("h_pos", "h_strain", "dY", "dd", "dA")


def _strain(S, strained):
    """eps [S,3,3] fp64 with fp32-exact entries: zero, or EPS and (S = 3) two more non-symmetric matrices made from it"""
    if not strained:
        return np.zeros((S, 3, 3))
    return np.stack([EPS, -0.5 * EPS.T, np.roll(EPS, 1, axis=0)][:S])


@functools.lru_cache(maxsize=None)
def _structure(S):
    """structure id of every row [N] int64 (None for S = 1: every row is structure 0)"""
    if S == 1:
        return None
    sid = np.random.default_rng(17).integers(0, S, N)
    for row, s in OUT_OF_RANGE.items():
        sid[row] = s
    sid.setflags(write=False)
    return sid


def _seeds(lmax, E, S):
    gen = torch.Generator().manual_seed(190 + lmax)
    ny = (lmax + 1) ** 2
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).float().double()     # fp32-exact values
    return {"Y": r(E, ny), "d": r(E), "A": r(N, ny)}, r(N, 3), r(3, 3, 3)[:S]


def _torch_second(mode, lmax, S, strained, cot, dtype):
    """(h_pos, h_strain, dY, dd, dA) by autograd of the strained geometry written in torch (CPU, ``dtype``), fp64 numpy"""
    pos, rowptr, src, dst, shift = cloud(mode)
    seeds, v, xi = _seeds(lmax, len(src), S)
    sid = _structure(S)
    src_t, dst_t = torch.as_tensor(src), torch.as_tensor(dst)
    p = torch.as_tensor(pos).to(dtype).requires_grad_(True)
    eps = torch.as_tensor(_strain(S, strained)).to(dtype).requires_grad_(True)
    s_row = torch.zeros(N, dtype=torch.long) if sid is None else torch.as_tensor(sid.copy())
    valid = ((s_row >= 0) & (s_row < S)).to(dtype)                              # a row outside [0, S) is unstrained
    eps_edge = (eps[s_row.clamp(0, S - 1)] * valid[:, None, None])[dst_t]
    rel0 = p[src_t] - p[dst_t] + torch.as_tensor(shift).to(dtype)
    rel = rel0 + torch.einsum("eab,eb->ea", eps_edge, rel0)
    nz = torch.as_tensor(np.nonzero(np.linalg.norm(rel.detach().double().numpy(), axis=1) > 0)[0])
    Ynz, dnz = sh_component_torch(lmax, rel[nz])          # an edge with d = 0 has Y = [1, 0, ...], d = 0: constants
    ny = (lmax + 1) ** 2
    Y = torch.zeros(len(src), ny, dtype=dtype).index_copy(0, nz, Ynz)
    d = torch.zeros(len(src), dtype=dtype).index_copy(0, nz, dnz)
    deg = torch.as_tensor(np.diff(rowptr)).clamp_min(1).to(dtype)
    A = torch.zeros(N, ny, dtype=dtype).index_add(0, dst_t, Y) / deg[:, None]
    A = torch.cat([torch.ones(N, 1, dtype=dtype), A[:, 1:]], 1)
    s = {k: t.to(dtype).requires_grad_(True) for k, t in seeds.items()}
    phi = (s["Y"] * Y).sum() + (s["d"] * d).sum() + (s["A"] * A).sum()
    gpos, geps = torch.autograd.grad(phi, [p, eps], create_graph=True)
    L = ((gpos * v.to(dtype)).sum() if cot != "xi" else 0) + ((geps * xi.to(dtype)).sum() if cot != "v" else 0)
    out = torch.autograd.grad(L, [p, eps, s["Y"], s["d"], s["A"]])
    return tuple(t.double().numpy() for t in out)


def _rel(got, want):
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else got
    return float(np.abs(got - want).max() / np.abs(want).max())


@functools.lru_cache(maxsize=None)
def reference(mode, lmax, S, strained, cot):
    """(fp64 tensors, fp32 yardstick per tensor = max |fp32 - fp64| / max |fp64|) of one case, once"""
    want = _torch_second(mode, lmax, S, strained, cot, torch.float64)
    for w in want:
        w.setflags(write=False)
    f32 = _torch_second(mode, lmax, S, strained, cot, torch.float32)
    return want, tuple(_rel(a, b) for a, b in zip(f32, want))


def _device_inputs(mode, lmax, S, strained):
    pos, rowptr, src, dst, shift = cloud(mode)
    g = graph(mode, pos, rowptr, src)
    seeds, v, xi = _seeds(lmax, len(src), S)
    dev = lambda t: t.float().to(DEV)
    sid = _structure(S)
    sid_d = torch.as_tensor(sid.copy()).int().to(DEV) if sid is not None else None
    eps = torch.as_tensor(_strain(S, strained)).float().to(DEV)
    return g, {k: dev(t) for k, t in seeds.items()}, dev(v), dev(xi), sid_d, eps


@pytest.mark.parametrize("cot", COTS)
@pytest.mark.parametrize("strained", [False, True], ids=["eps0", "eps"])
@pytest.mark.parametrize("S", [1, 3], ids=["S1", "S3"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("lmax", [1, 2])
def test_strained_second_derivatives_vs_fp64_autograd(lmax, mode, S, strained, cot):
    pos, rowptr, src, dst, shift = cloud(mode)
    want, yard = reference(mode, lmax, S, strained, cot)
    g, seeds, v, xi, sid, eps = _device_inputs(mode, lmax, S, strained)
    vc, xc = (v if cot != "xi" else None), (xi if cot != "v" else None)
    # through autograd: the seeds are leaves, so the tangents come back as their gradients
    p = g.pos4[:, :3].clone().requires_grad_(True)
    e = eps.clone().requires_grad_(True)
    s = {k: t.clone().requires_grad_(True) for k, t in seeds.items()}
    outs = ops.edge_geometry(g, lmax=lmax, pos=p, strain=e, structure=sid)
    gpos, geps = torch.autograd.grad(outs, [p, e], [s["Y"], s["d"], s["A"]], create_graph=True)
    first = [t for t, c in ((gpos, vc), (geps, xc)) if c is not None]
    auto = torch.autograd.grad(first, [p, e, s["Y"], s["d"], s["A"]], [c for c in (vc, xc) if c is not None])
    # the entries themselves, with NULL for the absent cotangent
    hp, hs = ops._edge_geometry_hvp_strained_raw(g.pos4, eps, g, lmax, sid, seeds["Y"], seeds["d"], seeds["A"], vc, xc)
    raw = (hp, hs) + ops._edge_geometry_jvp_raw(g.pos4, g, lmax, vc, strain=eps, structure=sid, xi=xc)
    print(f"\nl_max={lmax} {mode} S={S} eps={'0.05' if strained else '0'} cotangent={cot}: E = {len(src)}")
    ok = True
    for k, name in enumerate(NAMES):
        errs = (_rel(auto[k], want[k]), _rel(raw[k], want[k]))
        bound = max(2e-5, 20 * yard[k])
        print(f"  {name:8s} max |.| = {np.abs(want[k]).max():.3e}; autograd {errs[0]:.2e}, entry {errs[1]:.2e}; fp32 yardstick "
              f"{yard[k]:.2e}, bound {bound:.1e}")
        assert np.abs(want[k]).max() > 0 and torch.isfinite(auto[k]).all() and torch.isfinite(raw[k]).all(), name
        ok = ok and max(errs) < bound
    assert ok
    # rows without edges and the coincident pair receive exactly nothing, in h_pos and in the tangents
    empty = np.diff(rowptr) == 0
    p64 = pos.astype(np.float64)
    zero_edge = np.linalg.norm(p64[src] - p64[dst] + shift, axis=1) == 0
    untouched = empty.copy()
    untouched[dst[zero_edge]] = True                                            # the two points of the pair
    untouched, zero_edge = torch.as_tensor(untouched).to(DEV), torch.as_tensor(zero_edge).to(DEV)
    assert int(untouched.sum()) == N_ISOLATED + 2 and int(zero_edge.sum()) == 2
    for t in (auto, raw):
        assert not t[0][untouched].any() and not t[4][untouched].any()
        assert not t[2][zero_edge].any() and not t[3][zero_edge].any() and not t[2][:, 0].any() and not t[4][:, 0].any()


@pytest.mark.parametrize("mode", MODES)
def test_out_of_range_structures_add_nothing(mode):
    """every id outside [0, S): h_strain is exactly zero and h_pos is the unstrained kernel's (the same fp32 formula, eps and
    Xi being zero for such a row; the two differ by the order of the atomics: the project's 2e-5)"""
    g, seeds, v, xi, _, eps = _device_inputs(mode, 2, 3, True)
    sid = torch.full((N,), 7, dtype=torch.int32, device=DEV)
    sid[::2] = -2
    hp, hs = ops._edge_geometry_hvp_strained_raw(g.pos4, eps, g, 2, sid, seeds["Y"], seeds["d"], seeds["A"], v, xi)
    plain = ops._edge_geometry_hvp_raw(g.pos4, g, 2, seeds["Y"], seeds["d"], seeds["A"], v)
    assert not hs.any() and float(plain.abs().max()) > 0
    assert _rel(hp, plain.double().cpu().numpy()) < 2e-5
    # ... and some rows in range: their share only -- the rows of the five out-of-range ids of the main test carry edges
    deg = np.diff(cloud(mode)[1])
    assert sum(deg[row] > 0 for row in OUT_OF_RANGE) >= 2


@pytest.mark.parametrize("mode", MODES)
def test_one_structure_h_strain_is_bit_reproducible(mode):
    g, seeds, v, xi, sid, eps = _device_inputs(mode, 2, 1, True)
    runs = [ops._edge_geometry_hvp_strained_raw(g.pos4, eps, g, 2, None, seeds["Y"], seeds["d"], seeds["A"], v, xi)[1]
            for _ in range(2)]
    assert float(runs[0].abs().max()) > 0 and torch.equal(runs[0], runs[1])
    # h_pos = NULL: the same h_strain, bit for bit (the same sums in the same order)
    only = ops._edge_geometry_hvp_strained_raw(g.pos4, eps, g, 2, None, seeds["Y"], seeds["d"], seeds["A"], v, xi, want_pos=False)
    assert only[0] is None and torch.equal(only[1], runs[0])


def test_pos_hessian_false_and_first_order_bits():
    """``pos_hessian=False`` with a strain leaves g_pos and g_strain without a graph when the three gradients are constants.
    With ``create_graph=False`` the first-order call is the one it was: on a graph of disjoint pairs (every entry of g_pos is the
    sum of two addends, which commutes; g_strain of one structure is summed in a fixed order) the gradients under autograd are
    bit-equal to those of the raw backward without grad mode."""
    g, seeds, v, xi, sid, eps = _device_inputs("cell", 2, 1, True)
    p = g.pos4[:, :3].clone().requires_grad_(True)
    e = eps.clone().requires_grad_(True)
    outs = ops.edge_geometry(g, lmax=2, pos=p, strain=e, pos_hessian=False)
    gpos, geps = torch.autograd.grad(outs, [p, e], [seeds[k] for k in "YdA"], create_graph=True)
    assert not gpos.requires_grad and not geps.requires_grad
    pos = cloud("cell")[0]
    pairs = N // 2
    rowptr = np.minimum(np.arange(N + 1), 2 * pairs)
    src = np.arange(2 * pairs) ^ 1                                               # 2k <-> 2k + 1
    gp = graph("cell", pos, rowptr, src)
    sd = {k: t[:2 * pairs].contiguous() if k != "A" else t for k, t in seeds.items()}
    p = gp.pos4[:, :3].clone().requires_grad_(True)
    e = eps.clone().requires_grad_(True)
    outs = ops.edge_geometry(gp, lmax=2, pos=p, strain=e)
    gpos, geps = torch.autograd.grad(outs, [p, e], [sd[k] for k in "YdA"])
    with torch.no_grad():
        gpos0, geps0 = ops._edge_geometry_backward_raw(gp.pos4, eps, gp, 2, None, sd["Y"], sd["d"], sd["A"])
    assert float(gpos.abs().max()) > 0 and float(geps.abs().max()) > 0
    assert torch.equal(gpos, gpos0) and torch.equal(geps, geps0)


def _entry_args(mode, structures=1, **over):
    """the arguments of one entry call on ``structures`` structures, ``over`` replacing some; NaN-filled outputs"""
    S = structures
    g, seeds, v, xi, sid, eps = _device_inputs(mode, 2, S, True)
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    outs = {"hp": nan(N, 3), "hs": nan(S, 9), "dY": nan(g.num_edges, 9), "dd": nan(g.num_edges), "dA": nan(N, 9)}
    ws = torch.empty(_lib.load().e3_edge_geometry_backward_strained_workspace_bytes(N), dtype=torch.uint8, device=DEV)
    a = dict(pos4=g.pos4.data_ptr(), rowptr=g.rowptr.data_ptr(), src=g.src.data_ptr(), N=N, lmax=2, strain=eps.data_ptr(),
             sid=sid.data_ptr() if sid is not None else None, S=S, gY=seeds["Y"].data_ptr(), gd=seeds["d"].data_ptr(),
             gA=seeds["A"].data_ptr(), v=v.data_ptr(), xi=xi.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel(),
             **{k: t.data_ptr() for k, t in outs.items()})
    a.update(over)
    return a, outs, (g, seeds, v, xi, sid, eps, ws)


def _call(kind, name, a, pbc):
    head = (a["pos4"], a["rowptr"], a["src"], a["N"], a["lmax"], pbc, a["strain"], a["sid"], a["S"])
    if kind == "jvp":
        return getattr(_lib.load(), name)(*head, a["v"], a["xi"], a["dY"], a["dd"], a["dA"], None)
    return getattr(_lib.load(), name)(*head, a["gY"], a["gd"], a["gA"], a["v"], a["xi"], a["hp"], a["hs"], a["ws"],
                                      a["ws_bytes"], None)


def test_status_codes():
    INVALID = 1
    box, cell = _lib.Float3(*BOX), _lib.Float9(*[float(t) for t in TR.T.reshape(9)])
    common = ({"lmax": 0}, {"lmax": 3}, {"N": -1}, {"strain": None}, {"S": 0}, {"v": None, "xi": None})
    hvp_only = ({"hp": None, "hs": None}, {"ws": None}, {"ws_bytes": 8})
    for kind, more in (("jvp", ()), ("hvp", hvp_only)):
        for suffix, mode, pbc in (("", "open", None), ("", "box", box), ("_cell", "cell", cell)):
            name = f"e3_edge_geometry_{kind}_strained{suffix}"
            for over in common + more:
                a, outs, keep = _entry_args(mode, **over)
                assert _call(kind, name, a, pbc) == INVALID, (name, over)
                torch.cuda.synchronize()
                assert all(torch.isnan(t).all() for t in outs.values()), (name, over)      # refused before anything was written
            a, outs, keep = _entry_args(mode, N=0)
            assert _call(kind, name, a, pbc) == _lib.E3_OK
            # S > 1 needs no workspace; one cotangent and one output alone are accepted
            a, outs, keep = _entry_args(mode, structures=3, ws=None, ws_bytes=0, v=None, hp=None)
            assert _call(kind, name, a, pbc) == _lib.E3_OK
            torch.cuda.synchronize()
            assert torch.isnan(outs["hp"]).all() and torch.isfinite(outs["hs" if kind == "hvp" else "dY"]).all()
        for bad in ((1.0, -1.0, 1.0), (1.0, float("nan"), 1.0), (float("inf"), 1.0, 1.0)):
            a, outs, keep = _entry_args("box")
            assert _call(kind, f"e3_edge_geometry_{kind}_strained", a, _lib.Float3(*bad)) == INVALID, bad
        a, outs, keep = _entry_args("cell")
        singular = (1.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 0.0, 1.0)
        assert _call(kind, f"e3_edge_geometry_{kind}_strained_cell", a, _lib.Float9(*singular)) == INVALID
        torch.cuda.synchronize()
        assert all(torch.isnan(t).all() for t in outs.values())


@pytest.mark.parametrize("mode", MODES)
def test_no_edges_is_a_zero_fill(mode):
    pos, rowptr, src, _, _ = cloud(mode)
    g = graph(mode, pos, np.zeros(N + 1, np.int64), np.zeros(0, np.int64))
    v, xi = torch.randn(N, 3, device=DEV), torch.randn(1, 3, 3, device=DEV)
    eps = torch.as_tensor(_strain(1, True)).float().to(DEV)
    gA = torch.randn(N, 9, device=DEV)
    hp, hs = ops._edge_geometry_hvp_strained_raw(g.pos4, eps, g, 2, None, None, None, gA, v, xi)
    assert hp.shape == (N, 3) and hs.shape == (1, 3, 3) and not hp.any() and not hs.any()
    # the entry itself on a graph of empty rows: zero-fill only, with and without a src array
    one = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = ops._strain_workspace(N, DEV)
    name, pbc = g.entry("e3_edge_geometry_hvp_strained", strained=True)
    for src_ptr in (None, one.data_ptr()):
        out, outs = torch.full((N, 3), float("nan"), device=DEV), torch.full((1, 9), float("nan"), device=DEV)
        _lib.call(name, g.pos4.data_ptr(), g.rowptr.data_ptr(), src_ptr, N, 2, *pbc, eps.data_ptr(), None, 1, None, None,
                  gA.data_ptr(), v.data_ptr(), xi.data_ptr(), out.data_ptr(), outs.data_ptr(), ws.data_ptr(), ws.numel(), None)
        assert not out.any() and not outs.any()
    # through autograd
    p = g.pos4[:, :3].clone().requires_grad_(True)
    e = eps.clone().requires_grad_(True)
    A = ops.edge_geometry(g, lmax=2, pos=p, strain=e)[2]
    gpos, geps = torch.autograd.grad(A, [p, e], torch.randn_like(A), create_graph=True)
    hh, he = torch.autograd.grad([gpos, geps], [p, e], [v, xi])
    assert not hh.any() and not he.any()

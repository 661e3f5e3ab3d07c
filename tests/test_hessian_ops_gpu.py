"""The Hessian kernel of the edge geometry (e3_edge_geometry_hvp, open / box / cell, l_max 1 / 2) through ``ops.edge_geometry``:
h_pos = d<v, g_pos(pos; gY, gd, gA)>/dpos against fp64 torch autograd of the same geometry written in torch, as
tests/test_second_order_ops_gpu.py does for the tangent.

One hand-made cloud of N = 149 (no multiple of the four waves of a block) per periodicity, r = 0.15: a tight cluster of 100
points of diameter < r around the origin -- rows of 99 edges, so the lane loop of a row passes twice, and in the periodic modes
the cluster straddles every face of the box / cell -- a chain of 30 loosely connected points, 17 isolated points (empty rows)
and one exactly coincident pair (d = 0: no contribution).  Apart from that pair no two points are closer than 0.05 r, so the
1 / d^2 terms stay of the order of the rest.  The edge set is every pair within r by the fp64 minimum image; the lattice shift of
every edge is a constant of the reference.

Norm: max |got - want| / max |want|.  Bound: max(2e-5, 20 x yardstick), the yardstick being the SAME torch expression
evaluated in fp32 on the CPU against fp64, computed by every case itself -- 2e-5 is the project's bound for derivatives of fp32
kernels and 20 about the margin it keeps (tests/test_force_loss_gpu.py); it covers the order of the atomics.

Measured on one MI355X (error / yardstick over l_max and the absent gradient): open 2.0e-7 .. 4.5e-7 / 2.0e-7 .. 3.5e-7, box
8.3e-7 .. 1.9e-6 / 8.3e-7 .. 1.7e-6, cell 1.0e-6 .. 1.8e-6 / 1.0e-6 .. 2.0e-6 ("Hessian-vector products").
Without the kernel the comparison fails: the positions are no input of the geometry's backward, so the second derivative in
them is not even defined."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import models  # noqa: F401
import pbc_reference as P
import triclinic_reference as TR
from oracle.segnn_oracle import sh_component_torch
from scalable_e3_gnn_amd import _lib, ops
from scalable_e3_gnn_amd.radius_graph import RadiusGraph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, R = 149, 0.15
N_CLUSTER, N_LOOSE, N_ISOLATED = 100, 30, 17       # + the coincident pair
MIN_SEP = 0.05 * R
BOX = (1.0, 1.0, 1.0)
MODES = ("open", "box", "cell")
ABSENT = (None, "Y", "d", "A")


def _image(rel, mode):
    """fp64 minimum image of [..., 3] displacements"""
    flat = np.asarray(rel, np.float64).reshape(-1, 3)
    out = flat if mode == "open" else P.min_image64(flat, BOX) if mode == "box" else TR.min_image64_cell(flat, TR.T)
    return out.reshape(np.shape(rel))


@functools.lru_cache(maxsize=None)
def cloud(mode):
    """-> pos [N,3] fp32 (shuffled), rowptr, src, dst, shift [E,3] fp64 (image - raw: whole periods)"""
    rng = np.random.default_rng(70 + MODES.index(mode))
    M = TR.T if mode == "cell" else np.eye(3)
    pts = []

    def far_enough(p, least):
        return not pts or np.linalg.norm(_image(np.asarray(pts) - p, mode), axis=1).min() >= least

    while len(pts) < N_CLUSTER:                         # a ball of radius 0.48 r around the origin
        p = rng.standard_normal(3)
        p *= 0.48 * R * rng.random() ** (1 / 3) / np.linalg.norm(p)
        if far_enough(p, 1.5 * MIN_SEP):
            pts.append(p)
    last = np.array([0.5, 0.5, 0.5]) @ M
    pts.append(last)
    while len(pts) < N_CLUSTER + N_LOOSE:               # a chain: each point 0.4 r .. 0.9 r from the one before
        step = rng.standard_normal(3)
        p = last + step * rng.uniform(0.4, 0.9) * R / np.linalg.norm(step)
        if far_enough(p, 1.5 * MIN_SEP) and np.abs(p @ np.linalg.inv(M) - 0.5).max() < 0.22:
            pts.append(p)
            last = p
    while len(pts) < N_CLUSTER + N_LOOSE + N_ISOLATED + 1:   # isolated: 1.3 r from everything, in every image
        p = rng.uniform(-0.5, 0.5, 3) @ M
        if far_enough(p, 1.3 * R):
            pts.append(p)
    pts.append(pts[-1].copy())                          # the coincident pair: the last isolated point twice
    pos = np.asarray(pts)
    if mode != "open":                                  # wrapped into the box / cell: the cluster straddles every face
        f = pos @ np.linalg.inv(M)
        pos = (f - np.floor(f)) @ M
    pos = pos[rng.permutation(N)].astype(np.float32)
    raw = pos.astype(np.float64)[None, :, :] - pos.astype(np.float64)[:, None, :]      # [dst, src]
    img = _image(raw, mode)
    adj = (np.linalg.norm(img, axis=-1) < R) & ~np.eye(N, dtype=bool)
    dst, src = np.nonzero(adj)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=N))]).astype(np.int64)
    return pos, rowptr, src.astype(np.int64), dst.astype(np.int64), (img - raw)[dst, src]


def graph(mode, pos, rowptr, src):
    pos4 = torch.zeros(len(pos), 4)
    pos4[:, :3] = torch.as_tensor(pos)
    return RadiusGraph(perm=torch.arange(len(pos), dtype=torch.int32, device=DEV), pos4=pos4.to(DEV),
                       rowptr=torch.as_tensor(rowptr).int().to(DEV), src=torch.as_tensor(src).int().to(DEV).contiguous(),
                       num_edges=int(len(src)), grid=(1, 1, 1), box=BOX if mode == "box" else None,
                       cell=tuple(float(t) for t in TR.T.reshape(9)) if mode == "cell" else None)


def test_the_cloud_is_what_the_docstring_says():
    for mode in MODES:
        pos, rowptr, src, dst, shift = cloud(mode)
        deg = np.diff(rowptr)
        d = np.linalg.norm(pos.astype(np.float64)[src] - pos.astype(np.float64)[dst] + shift, axis=1)
        assert len(pos) == N == 149 and N % 4 != 0
        assert int((deg >= 99).sum()) == N_CLUSTER and int((deg == 0).sum()) == N_ISOLATED
        assert int((d == 0).sum()) == 2 and d[d > 0].min() >= MIN_SEP, (mode, d[d > 0].min())
        loose = (deg > 0) & (deg < 99)
        assert int(loose.sum()) == N_LOOSE + 2 and deg[loose].max() < 30       # the chain and the coincident pair
        if mode != "open":    # some edge crosses every face: a nonzero lattice shift along every direction
            n = np.rint(shift @ np.linalg.inv(TR.T if mode == "cell" else np.eye(3)))
            assert (np.abs(n).max(0) == 1).all(), (mode, np.abs(n).max(0))


def _seeds(lmax, E):
    gen = torch.Generator().manual_seed(90 + lmax)
    ny = (lmax + 1) ** 2
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).float().double()     # fp32-exact values
    return {"Y": r(E, ny), "d": r(E), "A": r(N, ny)}, r(N, 3)


def _torch_hvp(mode, lmax, absent, dtype):
    """h_pos by autograd of the geometry written in torch (CPU, ``dtype``), fp64 numpy"""
    pos, rowptr, src, dst, shift = cloud(mode)
    seeds, v = _seeds(lmax, len(src))
    src_t, dst_t = torch.as_tensor(src), torch.as_tensor(dst)
    p = torch.as_tensor(pos).to(dtype).requires_grad_(True)
    rel = p[src_t] - p[dst_t] + torch.as_tensor(shift).to(dtype)
    nz = torch.as_tensor(np.nonzero(np.linalg.norm(rel.detach().double().numpy(), axis=1) > 0)[0])
    Ynz, dnz = sh_component_torch(lmax, rel[nz])          # an edge with d = 0 has Y = [1, 0, ...], d = 0: constants
    ny = (lmax + 1) ** 2
    Y = torch.zeros(len(src), ny, dtype=dtype).index_copy(0, nz, Ynz)
    d = torch.zeros(len(src), dtype=dtype).index_copy(0, nz, dnz)
    deg = torch.as_tensor(np.diff(rowptr)).clamp_min(1).to(dtype)
    A = torch.zeros(N, ny, dtype=dtype).index_add(0, dst_t, Y) / deg[:, None]
    A = torch.cat([torch.ones(N, 1, dtype=dtype), A[:, 1:]], 1)
    phi = sum((seeds[k].to(dtype) * t).sum() for k, t in (("Y", Y), ("d", d), ("A", A)) if k != absent)
    (gpos,) = torch.autograd.grad(phi, [p], create_graph=True)
    (h,) = torch.autograd.grad((gpos * v.to(dtype)).sum(), [p])
    return h.double().numpy()


@functools.lru_cache(maxsize=None)
def reference(mode, lmax, absent):
    """(fp64 h_pos, fp32 yardstick = max |fp32 - fp64| / max |fp64|) of one case, once"""
    want = _torch_hvp(mode, lmax, absent, torch.float64)
    want.setflags(write=False)
    return want, _rel(_torch_hvp(mode, lmax, absent, torch.float32), want)


def _rel(got, want):
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else got
    return float(np.abs(got - want).max() / np.abs(want).max())


@pytest.mark.parametrize("absent", ABSENT, ids=lambda a: "all" if a is None else "no-" + a)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("lmax", [1, 2])
def test_edge_geometry_hessian_vs_fp64_autograd(lmax, mode, absent):
    pos, rowptr, src, dst, shift = cloud(mode)
    g = graph(mode, pos, rowptr, src)
    want, yard = reference(mode, lmax, absent)
    seeds, v = _seeds(lmax, len(src))
    dev = lambda t: t.float().to(DEV)
    # through autograd: the gradient of <v, g_pos> in the positions; the three output gradients are constants here, so
    # nothing but the Hessian term reaches pos
    p = g.pos4[:, :3].clone().requires_grad_(True)
    outs = dict(zip("YdA", ops.edge_geometry(g, lmax=lmax, pos=p)))
    keys = [k for k in "YdA" if k != absent]
    (gpos,) = torch.autograd.grad([outs[k] for k in keys], [p], [dev(seeds[k]) for k in keys], create_graph=True)
    (h,) = torch.autograd.grad((gpos * dev(v)).sum(), [p])
    # the entry itself, with NULL for the absent gradient
    raw = ops._edge_geometry_hvp_raw(g.pos4, g, lmax, *(dev(seeds[k]) if k != absent else None for k in "YdA"), dev(v))
    errs = (_rel(h, want), _rel(raw, want))
    bound = max(2e-5, 20 * yard)
    print(f"\nhvp l_max={lmax} {mode} absent={absent}: E = {len(src)}, max |h| = {np.abs(want).max():.3e}; autograd "
          f"{errs[0]:.2e}, entry {errs[1]:.2e}; fp32 yardstick {yard:.2e}, bound {bound:.1e}")
    assert np.abs(want).max() > 0 and torch.isfinite(h).all() and torch.isfinite(raw).all()
    assert max(errs) < bound, (errs, yard)
    # rows without edges and the coincident pair receive exactly nothing
    untouched = np.diff(rowptr) == 0
    p64 = pos.astype(np.float64)
    untouched[dst[np.linalg.norm(p64[src] - p64[dst] + shift, axis=1) == 0]] = True      # the two points of the pair
    untouched = torch.as_tensor(untouched).to(DEV)
    assert int(untouched.sum()) == N_ISOLATED + 2 and not h[untouched].any() and not raw[untouched].any()
    # pos_hessian=False: the positions get no edge from the geometry's backward
    p2 = g.pos4[:, :3].clone().requires_grad_(True)
    outs2 = ops.edge_geometry(g, lmax=lmax, pos=p2, pos_hessian=False)
    (gpos2,) = torch.autograd.grad(outs2, [p2], [dev(seeds[k]) for k in "YdA"], create_graph=True)
    assert not gpos2.requires_grad


def _entry_args(mode, lmax=2, **over):
    pos, rowptr, src, _, _ = cloud(mode)
    g = graph(mode, pos, rowptr, src)
    seeds, v = _seeds(lmax, len(src))
    t = {k: s.float().to(DEV) for k, s in seeds.items()}
    vd, h = v.float().to(DEV), torch.full((N, 3), float("nan"), device=DEV)
    a = dict(pos4=g.pos4.data_ptr(), rowptr=g.rowptr.data_ptr(), src=g.src.data_ptr(), N=N, lmax=lmax, gY=t["Y"].data_ptr(),
             gd=t["d"].data_ptr(), gA=t["A"].data_ptr(), v=vd.data_ptr(), h=h.data_ptr())
    a.update(over)
    keep = (g, t, vd, h)
    return a, keep


def _call(name, a, pbc=()):
    return getattr(_lib.load(), name)(a["pos4"], a["rowptr"], a["src"], a["N"], a["lmax"], *pbc, a["gY"], a["gd"], a["gA"],
                                      a["v"], a["h"], None)


def test_status_codes():
    INVALID = 1
    box, cell = _lib.Float3(*BOX), _lib.Float9(*[float(t) for t in TR.T.reshape(9)])
    for name, mode, pbc in (("e3_edge_geometry_hvp", "open", ()), ("e3_edge_geometry_hvp_pbc", "box", (box,)),
                            ("e3_edge_geometry_hvp_cell", "cell", (cell,))):
        for over in ({"lmax": 0}, {"lmax": 3}, {"v": None}, {"h": None}, {"N": -1}):
            a, keep = _entry_args(mode, **over)
            assert _call(name, a, pbc) == INVALID, (name, over)
            torch.cuda.synchronize()
            assert torch.isnan(keep[3]).all(), (name, over)              # refused before anything was written
        a, keep = _entry_args(mode, N=0)
        assert _call(name, a, pbc) == _lib.E3_OK
    a, _ = _entry_args("box")
    for bad in ((1.0, -1.0, 1.0), (1.0, float("nan"), 1.0), (float("inf"), 1.0, 1.0)):
        assert _call("e3_edge_geometry_hvp_pbc", a, (_lib.Float3(*bad),)) == INVALID, bad
    a, _ = _entry_args("cell")
    singular = (1.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 0.0, 1.0)
    assert _call("e3_edge_geometry_hvp_cell", a, (_lib.Float9(*singular),)) == INVALID


@pytest.mark.parametrize("mode", MODES)
def test_no_edges_is_a_zero_fill(mode):
    pos, rowptr, src, _, _ = cloud(mode)
    g = graph(mode, pos, np.zeros(N + 1, np.int64), np.zeros(0, np.int64))
    v = torch.randn(N, 3, device=DEV)
    h = ops._edge_geometry_hvp_raw(g.pos4, g, 2, None, None, torch.randn(N, 9, device=DEV), v)
    assert h.shape == (N, 3) and not h.any()
    # the entry itself on a graph of empty rows: zero-fill only, with and without a src array
    one = torch.zeros(1, dtype=torch.int32, device=DEV)
    name, pbc = g.entry("e3_edge_geometry_hvp")
    for src_ptr in (None, one.data_ptr()):
        out = torch.full((N, 3), float("nan"), device=DEV)
        _lib.call(name, g.pos4.data_ptr(), g.rowptr.data_ptr(), src_ptr, N, 2, *pbc, None, None, None, v.data_ptr(),
                  out.data_ptr(), None)
        assert not out.any()
    # through autograd
    p = g.pos4[:, :3].clone().requires_grad_(True)
    A = ops.edge_geometry(g, lmax=2, pos=p)[2]
    (gpos,) = torch.autograd.grad(A, [p], torch.randn_like(A), create_graph=True)
    (hh,) = torch.autograd.grad((gpos * v).sum(), [p])
    assert not hh.any()

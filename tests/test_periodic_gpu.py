"""Periodic boxes on the GPU: the radius graph bit for bit against the numpy restatement (tests/pbc_reference.py), the
minimum-image edge geometry against fp64, every SEGNN execution path against the fp64 oracle on the 27-image tiled cloud,
energy and forces against an fp64 autograd restatement, and translation invariance at 100 k particles.
Tolerances: 1e-5 of the output scale for fp32 paths (as tests/test_segnn_gpu.py), 5e-2 for bf16 storage (as
tests/test_bf16_gpu.py), 2e-5 for forces (as tests/test_forces_gpu.py)."""
import warnings

import numpy as np
import pytest
import torch

import pbc_reference as P
from oracle import graph_oracle as G
from oracle import segnn_oracle as S
from scalable_e3_gnn_amd import ops
from scalable_e3_gnn_amd.radius_graph import radius_graph
from scalable_e3_gnn_amd.segnn import SEGNN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rel(a, b):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _check_graph(pos, lo, hi, r, periodic):
    g = radius_graph(torch.as_tensor(pos, dtype=torch.float32).to(DEV), r, lo, hi, periodic=periodic)
    perm, pos4, rowptr, src = P.graph_pbc(pos, lo, hi, r, periodic)
    assert np.array_equal(g.perm.cpu().numpy(), perm)
    assert np.array_equal(g.pos4.cpu().numpy(), pos4)
    assert np.array_equal(g.rowptr.cpu().numpy(), rowptr)
    assert np.array_equal(g.src.cpu().numpy(), src)
    assert g.box == tuple(float(v) for v in P.box_lengths(lo, hi, periodic))
    return g


def _uniform(n, seed, lo=0.0, hi=1.0):
    return (lo + (hi - lo) * np.random.default_rng(seed).random((n, 3))).astype(np.float32)


def _dyadic(n, seed):
    """Uniform in [0, 1) on the 2^-16 grid: whole periods, box copies and grid-step translations are exact in fp32, so
    the periodic cloud and its moved / tiled versions have identical edge sets (no cutoff tie can flip)."""
    return (np.random.default_rng(seed).integers(0, 1 << 16, size=(n, 3)) / float(1 << 16)).astype(np.float32)


def test_graph_uniform_20k():
    pos = _uniform(20000, 0)
    g = _check_graph(pos, [0, 0, 0], [1, 1, 1], 0.04, True)
    assert g.num_edges > 0


def test_graph_corner_clusters():
    pos = _uniform(6000, 1)
    c = np.array([[0, 0, 0], [1, 1, 1], [1, 0, 1], [0, 1, 0]], np.float32)
    pos = (c[np.arange(6000) % 4] + (pos - 0.5) * np.float32(0.12)).astype(np.float32)  # straddling the corners
    _check_graph(pos, [0, 0, 0], [1, 1, 1], 0.05, True)


def test_graph_lattice_ties_at_the_cutoff():
    k = 16
    r = 1.0 / k
    q = (np.arange(k) / k).astype(np.float32)
    pos = np.stack(np.meshgrid(q, q, q, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    g = _check_graph(pos, [0, 0, 0], [1, 1, 1], r, True)
    # spacing, r and r^2 are exact: every site has its 6 face neighbours (ties d = r included, across the faces too)
    assert np.all(np.diff(g.rowptr.cpu().numpy()) == 6)


def test_graph_mixed_periodicity():
    pos = _uniform(8000, 2)
    _check_graph(pos, [0, 0, 0], [1, 1, 1], 0.06, (True, True, False))
    _check_graph(pos, [0, 0, 0], [1, 1, 1], 0.06, (False, False, True))


@pytest.mark.parametrize("L_over_r", [2.5, 2.0001, 2.3])
def test_graph_few_cells(L_over_r):
    """2 < L / r < 3: n = 2 cells per axis (neighbour offsets name a cell twice); L / r just above 2: n = 1."""
    pos = _uniform(1500, 3)
    r = 1.0 / L_over_r
    g = _check_graph(pos, [0, 0, 0], [1, 1, 1], r, True)
    assert g.grid[0][0] == (1 if L_over_r < 2.0002 else 2)


def test_graph_positions_outside_the_box():
    pos = _uniform(5000, 4, 0.5, 2.5)  # box [0.5, 2.5)
    lo, hi = [0.5, 0.5, 0.5], [2.5, 2.5, 2.5]
    base = _check_graph(pos, lo, hi, 0.12, True)
    shifts = np.random.default_rng(5).integers(-3, 4, size=pos.shape).astype(np.float32) * np.float32(2.0)
    _check_graph(pos + shifts, lo, hi, 0.12, True)  # whole periods
    _check_graph((pos + np.float32(0.37) * np.float32(2.0)).astype(np.float32), lo, hi, 0.12, True)  # fractional shift
    assert base.num_edges > 0


def test_open_graph_unchanged():
    pos = torch.as_tensor(_uniform(5000, 6)).to(DEV)
    a = radius_graph(pos, 0.05, [0, 0, 0], [1, 1, 1])
    b = radius_graph(pos, 0.05, [0, 0, 0], [1, 1, 1], periodic=False)
    c = radius_graph(pos, 0.05, [0, 0, 0], [1, 1, 1], periodic=(False, False, False))
    for g in (b, c):
        assert g.box is None
        for f in ("perm", "pos4", "rowptr", "src"):
            assert torch.equal(getattr(a, f), getattr(g, f))


def test_graph_1m_at_the_bench_cutoff():
    N = 1 << 20
    r = float((3 * 24.0 / (4 * np.pi * N)) ** (1 / 3))
    pos = _uniform(N, 7)
    g = radius_graph(torch.as_tensor(pos).to(DEV), r, [0, 0, 0], [1, 1, 1], periodic=True)
    rowptr, src = g.rowptr.cpu().numpy().astype(np.int64), g.src.cpu().numpy().astype(np.int64)
    dst = np.repeat(np.arange(N), np.diff(rowptr))
    assert np.all(src != dst)
    row_start = np.zeros(len(src), bool)
    row_start[rowptr[:-1][np.diff(rowptr) > 0]] = True
    assert np.all((np.diff(src) > 0) | row_start[1:])  # ascending inside every row
    fwd = np.sort(src * N + dst)
    assert np.array_equal(fwd, np.sort(dst * N + src))  # symmetric
    sp = g.pos4.cpu().numpy()[:, :3].astype(np.float64)
    relv = P.min_image64(sp[src] - sp[dst], [1.0, 1.0, 1.0])
    d = np.linalg.norm(relv, axis=1)
    assert d.max() <= r * (1 + 1e-6)
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return
    w = sp
    pairs = cKDTree(w, boxsize=1.0).query_pairs(r, output_type="ndarray").astype(np.int64)
    pd = np.linalg.norm(P.min_image64(w[pairs[:, 0]] - w[pairs[:, 1]], [1.0] * 3), axis=1)
    pairs = pairs[np.abs(pd - r) > 1e-6]
    lo_, hi_ = np.minimum(src, dst), np.maximum(src, dst)
    ours = lo_ * N + hi_
    ours = np.unique(ours[np.abs(d - r) > 1e-6])
    theirs = np.unique(np.minimum(pairs[:, 0], pairs[:, 1]) * N + np.maximum(pairs[:, 0], pairs[:, 1]))
    assert np.array_equal(ours, theirs)


@pytest.mark.parametrize("lmax", [1, 2])
def test_edge_geometry_vs_fp64(lmax):
    pos = _dyadic(6000, 8)
    g = radius_graph(torch.as_tensor(pos).to(DEV), 0.06, [0, 0, 0], [1, 1, 1], periodic=(True, False, True))
    L = np.array(g.box)
    src, rowptr = g.src.cpu().numpy(), g.rowptr.cpu().numpy()
    dst = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    sp = g.pos4.cpu().numpy()[:, :3].astype(np.float64)
    Yw, dw = P.sh64(lmax, P.min_image64(sp[src] - sp[dst], L))
    Aw = np.zeros((len(rowptr) - 1, (lmax + 1) ** 2))
    np.add.at(Aw, dst, Yw)
    Aw /= np.maximum(np.diff(rowptr), 1)[:, None]
    Aw[:, 0] = 1.0
    # wrapped (the graph's own pos4) and unwrapped (whole periods added per particle on the periodic axes)
    shifts = np.random.default_rng(9).integers(-2, 3, size=sp.shape) * np.array([1.0, 0.0, 1.0])
    unwrapped = torch.as_tensor((sp + shifts).astype(np.float32)).to(DEV)
    for pos_arg in (None, unwrapped):
        Y, d, A = ops.edge_geometry(g, lmax=lmax, pos=pos_arg)
        assert rel(Y, Yw) < 2e-5 and rel(d, dw) < 2e-5 and rel(A, Aw) < 2e-5
    # the open-box geometry of the same graph differs on the edges across the faces
    assert (np.abs(P.min_image64(sp[src] - sp[dst], L) - (sp[src] - sp[dst])).max()) > 0.5


# ---------------------------------------------------------------------------------------------------------------------
# the 27-image oracle: a periodic cloud equals the centre copy of the cloud tiled 3 x 3 x 3 as an open cloud
# ---------------------------------------------------------------------------------------------------------------------
def _tiled_case(M, layers, seed, in_dim=4):
    rng = np.random.default_rng(seed)
    Lb = 1.0
    r = Lb / (layers + 2.2)  # L >= (layers + 2) r: the centre copy's receptive field stays inside the tiling
    pos = _dyadic(M, seed)
    x = rng.standard_normal((M, in_dim)).astype(np.float32)
    tiled, centre = P.tile27(pos.astype(np.float64), [Lb] * 3)
    tiled = tiled.astype(np.float32)
    return pos, x, r, tiled, centre


def _oracle_centre(fn, M, x, tiled, centre, r):
    perm, rowptr, src = G.graph(tiled, [-1, -1, -1], [2, 2, 2], r)
    xt = np.tile(x, (27, 1)).astype(np.float64)
    out = fn(xt[perm], tiled[perm].astype(np.float64), rowptr, src)
    back = np.empty_like(out)
    back[perm] = out
    return back[centre * M:(centre + 1) * M]


def _periodic_forward(model, pos, x, r, dtype=torch.float32, grad=False):
    g = radius_graph(torch.as_tensor(pos).to(DEV), r, [0, 0, 0], [1, 1, 1], periodic=True)
    perm = g.perm.cpu().long()
    xs = torch.as_tensor(x)[perm].to(DEV).to(dtype)
    if grad:
        xs.requires_grad_(True)
        with torch.enable_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # "the unfused differentiable chain runs": what is tested here
            out = model(xs, g)
    else:
        with torch.no_grad():
            out = model(xs, g)
    back = torch.empty_like(out)
    back[perm.to(DEV)] = out
    return back.detach().float().double().cpu().numpy()


@pytest.mark.parametrize("path", ["one_launch_l2", "msg_fused_l1", "per_tp", "grad_chain"])
def test_27_image_oracle(path):
    M, H, layers = 200, 32, 2
    lmax = 1 if path == "msg_fused_l1" else 2
    pos, x, r, tiled, centre = _tiled_case(M, layers, seed=11)
    torch.manual_seed(12)
    model = SEGNN("1x0e+1x1o", H, "1x1o", layers, lmax=lmax).to(DEV)
    if path == "per_tp":
        for l in model.layers:
            l.fuse_message = False
    got = _periodic_forward(model, pos, x, r, grad=(path == "grad_chain"))
    params = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    fwd = S.forward_l2 if lmax == 2 else S.forward
    want = _oracle_centre(lambda xx, pp, rp, sr: fwd(params, H, layers, "1x0e+1x1o", "1x1o", xx, pp, rp, sr),
                          M, x, tiled, centre, r)
    assert rel(got, want) < 1e-5, rel(got, want)


def test_27_image_oracle_bf16():
    M, H, layers = 200, 32, 2
    pos, x, r, tiled, centre = _tiled_case(M, layers, seed=13)
    torch.manual_seed(14)
    model = SEGNN("1x0e+1x1o", H, "1x1o", layers, lmax=2).bfloat16().to(DEV)
    x = torch.as_tensor(x).bfloat16().float().numpy()
    got = _periodic_forward(model, pos, x, r, dtype=torch.bfloat16)
    params = {k: v.detach().float().cpu().numpy() for k, v in model.state_dict().items()}
    want = _oracle_centre(lambda xx, pp, rp, sr: S.forward_l2(params, H, layers, "1x0e+1x1o", "1x1o", xx, pp, rp, sr),
                          M, x, tiled, centre, r)
    assert rel(got, want) < 5e-2, rel(got, want)


def test_energy_and_forces():
    M, H, layers, lmax = 200, 16, 2, 2
    pos, x, r, tiled, centre = _tiled_case(M, layers, seed=15)
    torch.manual_seed(16)
    model = SEGNN("1x0e+1x1o", H, "1x0e", layers, lmax=lmax).to(DEV)
    params = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    # reference energy: molecule 0 = the centre copy of the 27-image open cloud
    perm_t, rowptr_t, src_t = G.graph(tiled, [-1, -1, -1], [2, 2, 2], r)
    mol = np.ones(27 * M, np.int64)
    mol[centre * M:(centre + 1) * M] = 0
    xt = np.tile(x, (27, 1)).astype(np.float64)
    e27, _, _ = S.energy_forces_torch(params, H, layers, lmax, "1x0e+1x1o", xt[perm_t], tiled[perm_t].astype(np.float64),
                                      rowptr_t, src_t, mol[perm_t], 2)
    # periodic graph, unwrapped positions (whole periods added per particle) through the periodic geometry backward
    g = radius_graph(torch.as_tensor(pos).to(DEV), r, [0, 0, 0], [1, 1, 1], periodic=True)
    perm = g.perm.cpu().numpy()
    sp = g.pos4.cpu().numpy()[:, :3].astype(np.float64)
    unwrapped = sp + np.random.default_rng(17).integers(-2, 3, size=sp.shape)
    e_ref, f_ref = P.energy_forces_pbc(params, H, layers, lmax, "1x0e+1x1o", x[perm].astype(np.float64), unwrapped,
                                       g.rowptr.cpu().numpy(), g.src.cpu().numpy(), g.box)
    assert abs(e_ref - e27[0]) < 1e-9 * max(1.0, abs(e27[0])) + 1e-10, (e_ref, e27[0])
    p = torch.as_tensor(unwrapped.astype(np.float32)).to(DEV).requires_grad_(True)
    xs = torch.as_tensor(x[perm]).to(DEV)
    with torch.enable_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        geom = ops.edge_geometry(g, lmax=lmax, pos=p)
        energy = model(xs, g, geometry=geom).sum()
        (gp,) = torch.autograd.grad(energy, [p])
    forces = -gp.double().cpu().numpy()
    assert abs(float(energy) - e_ref) < 1e-5 * max(1.0, abs(e_ref))
    assert rel(forces, f_ref) < 2e-5, rel(forces, f_ref)
    assert np.abs(forces.sum(0)).max() < 1e-4 * np.abs(forces).max()


@pytest.mark.parametrize("lmax", [1, 2])
def test_translation_invariance_100k(lmax):
    N, H, layers = 100000, 32, 2
    r = float((3 * 24.0 / (4 * np.pi * N)) ** (1 / 3))
    pos = _dyadic(N, 18)
    x = np.random.default_rng(19).standard_normal((N, 4)).astype(np.float32)
    torch.manual_seed(20)
    model = SEGNN("1x0e+1x1o", H, "1x0e", layers, lmax=lmax).to(DEV)
    t = _dyadic(1, 21)[0]
    moved = (pos + t).astype(np.float32)  # exact: outside the box on the periodic axes, wrapped by the builder
    moved_w = np.where(moved >= 1, moved - 1, moved).astype(np.float32)  # the same cloud as an open user would see it

    def run(p, periodic):
        g = radius_graph(torch.as_tensor(p).to(DEV), r, [0, 0, 0], [1, 1, 1], periodic=periodic)
        perm = g.perm.cpu().long()
        with torch.no_grad():
            out = model(torch.as_tensor(x)[perm].to(DEV), g)
        back = torch.empty_like(out)
        back[perm.to(DEV)] = out
        return back.double().cpu().numpy()

    a, b = run(pos, True), run(moved, True)
    assert rel(b, a) < 1e-5, rel(b, a)
    # what the periodic box guards: the open graph of the moved cloud loses the neighbours across the old faces
    oa, ob = run(pos, False), run(moved_w, False)
    face = np.any((pos < 2 * r) | (pos > 1 - 2 * r), axis=1)
    assert np.abs(ob - oa)[face].max() > 1e-2 * np.abs(oa).max()

"""General (triclinic) periodic cells on the GPU: the radius graph bit for bit against the numpy restatement
(tests/triclinic_reference.py), the minimum-image edge geometry against fp64, every SEGNN execution path against the fp64
oracle on the 27-image tiled cloud, energy / forces / virial / stress against the fp64 autograd restatement, lattice
equivalence (T and T' = M T span the same lattice), rotation, strain, and the untouched open / orthorhombic paths.

Tolerances (those of tests/test_periodic_gpu.py and tests/test_stress_gpu.py: the oracles are the same): 1e-5 of the
output scale for fp32 forwards, 2e-5 for forces, virial and stress, 5e-2 for bf16 storage, 2e-5 for the geometry against
fp64, 2e-3 for central differences."""
import contextlib
import warnings

import numpy as np
import pytest
import torch

import triclinic_reference as R
from oracle import graph_oracle as G
from oracle import segnn_oracle as S
from scalable_e3_gnn_amd import ops
from scalable_e3_gnn_amd.batched import PeriodicEnergyModel
from scalable_e3_gnn_amd.radius_graph import radius_graph
from scalable_e3_gnn_amd.segnn import SEGNN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, TP = R.T, R.TP
VOL = 0.65625


def rel(a, b):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@contextlib.contextmanager
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # "the unfused differentiable chain runs": what is used here
        yield


def _uniform(n, seed, cell, origin=(0.0, 0.0, 0.0)):
    s = np.random.default_rng(seed).random((n, 3))
    return (s @ np.asarray(cell, np.float64) + np.asarray(origin, np.float64)).astype(np.float32)


def _dyadic(n, seed, cell=T):
    """Fractional coordinates uniform in [0, 1) on the 2^-16 grid, in a cell with dyadic entries (T, T', the unit cube):
    the positions, their differences and whole-lattice shifts are exact in fp32 (no cutoff tie can flip)."""
    s = np.random.default_rng(seed).integers(0, 1 << 16, size=(n, 3)) / float(1 << 16)
    p = s @ np.asarray(cell, np.float64)
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
    return p.astype(np.float32)


def _pairs(g):
    """Sorted codes of the directed edges in the caller's ids."""
    perm = g.perm.cpu().numpy().astype(np.int64)
    n = len(perm)
    return np.sort(perm[g.dst.cpu().numpy()] * n + perm[g.src.cpu().numpy()])


# ---------------------------------------------------------------------------------------------------------------------
# 1: the graph, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def _check_graph(pos, cell, r, origin=None):
    kw = {} if origin is None else {"origin": origin}
    g = radius_graph(torch.as_tensor(pos, dtype=torch.float32).to(DEV), r, cell=np.asarray(cell).tolist(), **kw)
    perm, pos4, rowptr, src = R.graph_cell(pos, cell, r, (0.0, 0.0, 0.0) if origin is None else origin)
    assert np.array_equal(g.perm.cpu().numpy(), perm)
    assert np.array_equal(g.pos4.cpu().numpy(), pos4)
    assert np.array_equal(g.rowptr.cpu().numpy(), rowptr)
    assert np.array_equal(g.src.cpu().numpy(), src)
    assert g.box is None and g.box_arg is None
    assert g.cell == tuple(float(np.float32(v)) for v in np.asarray(cell).reshape(9))
    assert g.origin == tuple(float(np.float32(v)) for v in ((0, 0, 0) if origin is None else origin))
    assert g.volume == float(R.derive(cell)[2])
    return g


def test_graph_uniform_20k():
    g = _check_graph(_uniform(20000, 0, T), T, 0.04)
    assert g.num_edges > 0 and g.volume == VOL


def test_graph_corner_clusters():
    u = np.random.default_rng(1).random((6000, 3))
    corners = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], np.float64)
    s = corners[np.arange(6000) % 8] + (u - 0.5) * 0.12  # straddling the eight corners of the cell
    _check_graph((s @ T).astype(np.float32), T, 0.05)


@pytest.mark.parametrize("r, n", [(0.37499, (2, 2, 1)), (0.3, (3, 2, 2)), (0.36, (2, 2, 2))])
def test_graph_few_cells(r, n):
    """r just under h_min / 2 = 0.375: one or two grid cells per direction (neighbour offsets name a cell twice)."""
    g = _check_graph(_uniform(1500, 3, T), T, r)
    assert g.grid[0] == n


def test_graph_positions_outside_the_cell():
    pos = _dyadic(5000, 4)
    base = _check_graph(pos, T, 0.09)
    k = np.random.default_rng(5).integers(-3, 4, size=pos.shape).astype(np.float64)
    moved = _check_graph((pos + k @ T).astype(np.float32), T, 0.09)  # whole lattice vectors (exact)
    assert np.array_equal(_pairs(moved), _pairs(base)) and base.num_edges > 0
    frac = np.array([0.37, -1.21, 2.6]) @ T
    _check_graph((pos + frac).astype(np.float32), T, 0.09)  # a fractional shift


def test_graph_origin():
    origin = (0.3, -0.2, 0.1)
    pos = _uniform(6000, 6, T, origin)
    _check_graph(pos, T, 0.07, origin)
    _check_graph((pos + np.array([2.0, 1.0, -1.0]) @ T).astype(np.float32), T, 0.07, origin)
    _check_graph(_uniform(4000, 7, TP), TP, 0.07, (-5.0, 3.0, 0.25))  # all points outside the cell of this origin


# ---------------------------------------------------------------------------------------------------------------------
# 2: one million points at the bench cutoff
# ---------------------------------------------------------------------------------------------------------------------
def test_graph_1m_at_the_bench_cutoff():
    N = 1 << 20
    r = float((3 * 24.0 / (4 * np.pi * N)) ** (1 / 3))
    cell = (T / VOL ** (1 / 3)).astype(np.float32)  # T scaled to unit volume
    pos = _uniform(N, 8, cell)
    g = radius_graph(torch.as_tensor(pos).to(DEV), r, cell=cell.tolist())
    assert abs(g.volume - 1.0) < 1e-6
    rowptr, src = g.rowptr.cpu().numpy().astype(np.int64), g.src.cpu().numpy().astype(np.int64)
    dst = np.repeat(np.arange(N), np.diff(rowptr))
    assert np.all(src != dst)
    row_start = np.zeros(len(src), bool)
    row_start[rowptr[:-1][np.diff(rowptr) > 0]] = True
    assert np.all((np.diff(src) > 0) | row_start[1:])  # ascending inside every row
    assert np.array_equal(np.sort(src * N + dst), np.sort(dst * N + src))  # symmetric
    sp = g.pos4.cpu().numpy()[:, :3].astype(np.float64)
    c64 = cell.astype(np.float64)
    d = np.linalg.norm(R.min_image64_cell(sp[src] - sp[dst], c64), axis=1)
    assert d.max() <= r * (1 + 1e-6)
    assert 20 < len(src) / N < 28  # k about 24
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return
    # the 27-image tiling, cut down to the images that can reach the cell: copy o of a point matters only when it lies
    # within r of the cell, i.e. q_a <= r for o_a = +1 and q_a >= h_a - r for o_a = -1 (q = s h, the distance to the faces)
    _, hgt, _ = R.derive(cell)
    q = (sp @ np.linalg.inv(c64)) * hgt.astype(np.float64)
    tol = 1e-4
    ext, owner = [sp], [np.arange(N)]
    for o in [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) != (0, 0, 0)]:
        m = np.ones(N, bool)
        for a in range(3):
            if o[a] == 1:
                m &= q[:, a] <= r + tol
            elif o[a] == -1:
                m &= q[:, a] >= hgt[a] - r - tol
        ext.append(sp[m] + np.asarray(o, np.float64) @ c64)
        owner.append(np.nonzero(m)[0])
    ext, owner = np.concatenate(ext), np.concatenate(owner)
    pairs = cKDTree(ext).query_pairs(r + 2e-6, output_type="ndarray").astype(np.int64)
    pairs = pairs[pairs[:, 0] < N]  # i < j: at least one end in the centre copy
    pd = np.linalg.norm(ext[pairs[:, 0]] - ext[pairs[:, 1]], axis=1)
    a, b = owner[pairs[:, 0]], owner[pairs[:, 1]]
    code = np.minimum(a, b) * N + np.maximum(a, b)
    ties = np.unique(np.concatenate([code[np.abs(pd - r) <= 1e-6],
                                     (np.minimum(src, dst) * N + np.maximum(src, dst))[np.abs(d - r) <= 1e-6]]))
    theirs = np.unique(code[pd <= r])
    ours = np.unique(np.minimum(src, dst) * N + np.maximum(src, dst))
    assert len(ties) <= 1e-3 * len(theirs), (len(ties), len(theirs))
    assert np.array_equal(np.setdiff1d(ours, ties), np.setdiff1d(theirs, ties))


# ---------------------------------------------------------------------------------------------------------------------
# 3: a cubic cell is the orthorhombic box
# ---------------------------------------------------------------------------------------------------------------------
def _forward(model, g, x, dtype=torch.float32, grad=False):
    perm = g.perm.cpu().long()
    xs = torch.as_tensor(x)[perm].to(DEV).to(dtype)
    if grad:
        xs.requires_grad_(True)
        with torch.enable_grad(), _quiet():
            out = model(xs, g)
    else:
        with torch.no_grad():
            out = model(xs, g)
    back = torch.empty_like(out)
    back[perm.to(DEV)] = out
    return back.detach().float().double().cpu().numpy()


@pytest.mark.parametrize("lmax", [1, 2])
def test_cubic_cell_equals_the_periodic_box(lmax):
    N, H, layers, r = 20000, 32, 2, 0.05
    pos = _dyadic(N, 9, np.eye(3))
    x = np.random.default_rng(10).standard_normal((N, 4)).astype(np.float32)
    pd = torch.as_tensor(pos).to(DEV)
    gc = radius_graph(pd, r, cell=np.eye(3).tolist())
    gp = radius_graph(pd, r, [0, 0, 0], [1, 1, 1], periodic=True)
    assert gc.box is None and gp.cell is None and gc.volume == 1.0
    assert np.array_equal(_pairs(gc), _pairs(gp)) and gc.num_edges > 0
    torch.manual_seed(11)
    model = SEGNN("1x0e+1x1o", H, "1x0e", layers, lmax=lmax).to(DEV)
    a, b = _forward(model, gc, x), _forward(model, gp, x)
    assert rel(a, b) < 1e-5, rel(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# 4: geometry against fp64
# ---------------------------------------------------------------------------------------------------------------------
def _geometry_ref(g, lmax, cell):
    import pbc_reference as P
    src, rowptr = g.src.cpu().numpy(), g.rowptr.cpu().numpy()
    dst = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    sp = g.pos4.cpu().numpy()[:, :3].astype(np.float64)
    Yw, dw = P.sh64(lmax, R.min_image64_cell(sp[src] - sp[dst], cell))
    Aw = np.zeros((len(rowptr) - 1, (lmax + 1) ** 2))
    np.add.at(Aw, dst, Yw)
    Aw /= np.maximum(np.diff(rowptr), 1)[:, None]
    Aw[:, 0] = 1.0
    return Yw, dw, Aw, sp, src, dst


@pytest.mark.parametrize("lmax", [1, 2])
def test_edge_geometry_vs_fp64(lmax):
    g = radius_graph(torch.as_tensor(_dyadic(6000, 12)).to(DEV), 0.07, cell=T.tolist())
    Yw, dw, Aw, sp, src, dst = _geometry_ref(g, lmax, T)
    k = np.random.default_rng(13).integers(-2, 3, size=sp.shape).astype(np.float64)
    unwrapped = torch.as_tensor((sp + k @ T).astype(np.float32)).to(DEV)  # whole lattice vectors per particle (exact)
    for pos_arg in (None, unwrapped):
        Y, d, A = ops.edge_geometry(g, lmax=lmax, pos=pos_arg)
        assert rel(Y, Yw) < 2e-5 and rel(d, dw) < 2e-5 and rel(A, Aw) < 2e-5, (rel(Y, Yw), rel(d, dw), rel(A, Aw))
    # the open-box geometry of the same graph differs on the edges across the faces
    assert np.abs(R.min_image64_cell(sp[src] - sp[dst], T) - (sp[src] - sp[dst])).max() > 0.5


# ---------------------------------------------------------------------------------------------------------------------
# 5: the 27-image oracle on T
# ---------------------------------------------------------------------------------------------------------------------
def _tiled_case(M, layers, seed, cell=T, in_dim=4):
    rng = np.random.default_rng(seed)
    hmin = float(R.derive(cell)[1].min())
    r = hmin / (layers + 2.2)  # h_min >= (layers + 2) r: the centre copy's receptive field stays inside the tiling
    pos = _dyadic(M, seed, cell)
    x = rng.standard_normal((M, in_dim)).astype(np.float32)
    tiled, centre = R.tile27(pos.astype(np.float64), cell)
    tiled = tiled.astype(np.float32)
    return pos, x, r, tiled, centre


def _tiled_graph(tiled, r):
    lo, hi = tiled.min(0) - 0.5, tiled.max(0) + 0.5
    return G.graph(tiled, lo.tolist(), hi.tolist(), r)


def _oracle_centre(fn, M, x, tiled, centre, r):
    perm, rowptr, src = _tiled_graph(tiled, r)
    xt = np.tile(x, (27, 1)).astype(np.float64)
    out = fn(xt[perm], tiled[perm].astype(np.float64), rowptr, src)
    back = np.empty_like(out)
    back[perm] = out
    return back[centre * M:(centre + 1) * M]


@pytest.mark.parametrize("path", ["one_launch_l2", "msg_fused_l1", "per_tp", "grad_chain"])
def test_27_image_oracle(path):
    M, H, layers = 200, 32, 2
    lmax = 1 if path == "msg_fused_l1" else 2
    pos, x, r, tiled, centre = _tiled_case(M, layers, seed=14)
    torch.manual_seed(15)
    model = SEGNN("1x0e+1x1o", H, "1x1o", layers, lmax=lmax).to(DEV)
    if path == "per_tp":
        for l in model.layers:
            l.fuse_message = False
    g = radius_graph(torch.as_tensor(pos).to(DEV), r, cell=T.tolist())
    got = _forward(model, g, x, grad=(path == "grad_chain"))
    params = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    fwd = S.forward_l2 if lmax == 2 else S.forward
    want = _oracle_centre(lambda xx, pp, rp, sr: fwd(params, H, layers, "1x0e+1x1o", "1x1o", xx, pp, rp, sr),
                          M, x, tiled, centre, r)
    assert rel(got, want) < 1e-5, rel(got, want)


def test_27_image_oracle_bf16():
    M, H, layers = 200, 32, 2
    pos, x, r, tiled, centre = _tiled_case(M, layers, seed=16)
    torch.manual_seed(17)
    model = SEGNN("1x0e+1x1o", H, "1x1o", layers, lmax=2).bfloat16().to(DEV)
    x = torch.as_tensor(x).bfloat16().float().numpy()
    g = radius_graph(torch.as_tensor(pos).to(DEV), r, cell=T.tolist())
    got = _forward(model, g, x, dtype=torch.bfloat16)
    params = {k: v.detach().float().cpu().numpy() for k, v in model.state_dict().items()}
    want = _oracle_centre(lambda xx, pp, rp, sr: S.forward_l2(params, H, layers, "1x0e+1x1o", "1x1o", xx, pp, rp, sr),
                          M, x, tiled, centre, r)
    assert rel(got, want) < 5e-2, rel(got, want)


# ---------------------------------------------------------------------------------------------------------------------
# 6: energy and forces
# ---------------------------------------------------------------------------------------------------------------------
def test_energy_and_forces():
    M, H, layers, lmax = 200, 16, 2, 2
    pos, x, r, tiled, centre = _tiled_case(M, layers, seed=18)
    torch.manual_seed(19)
    model = SEGNN("1x0e+1x1o", H, "1x0e", layers, lmax=lmax).to(DEV)
    params = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    # reference energy: molecule 0 = the centre copy of the 27-image open cloud
    perm_t, rowptr_t, src_t = _tiled_graph(tiled, r)
    mol = np.ones(27 * M, np.int64)
    mol[centre * M:(centre + 1) * M] = 0
    xt = np.tile(x, (27, 1)).astype(np.float64)
    e27, _, _ = S.energy_forces_torch(params, H, layers, lmax, "1x0e+1x1o", xt[perm_t], tiled[perm_t].astype(np.float64),
                                      rowptr_t, src_t, mol[perm_t], 2)
    # the cell graph, unwrapped positions (whole lattice vectors added per particle) through the cell geometry backward
    g = radius_graph(torch.as_tensor(pos).to(DEV), r, cell=T.tolist())
    perm = g.perm.cpu().numpy()
    sp = g.pos4.cpu().numpy()[:, :3].astype(np.float64)
    unwrapped = sp + np.random.default_rng(20).integers(-2, 3, size=sp.shape).astype(np.float64) @ T
    e_ref, f_ref, _ = R.energy_forces_strain_cell(params, H, layers, lmax, "1x0e+1x1o", x[perm].astype(np.float64),
                                                  unwrapped, g.rowptr.cpu().numpy(), g.src.cpu().numpy(), T)
    assert abs(e_ref - e27[0]) < 1e-9 * max(1.0, abs(e27[0])) + 1e-10, (e_ref, e27[0])
    p = torch.as_tensor(unwrapped.astype(np.float32)).to(DEV).requires_grad_(True)
    xs = torch.as_tensor(x[perm]).to(DEV)
    with torch.enable_grad(), _quiet():
        geom = ops.edge_geometry(g, lmax=lmax, pos=p)
        energy = model(xs, g, geometry=geom).sum()
        (gp,) = torch.autograd.grad(energy, [p])
    forces = -gp.double().cpu().numpy()
    assert abs(float(energy) - e_ref) < 1e-5 * max(1.0, abs(e_ref))
    assert rel(forces, f_ref) < 2e-5, rel(forces, f_ref)
    assert np.abs(forces.sum(0)).max() < 1e-4 * np.abs(forces).max()


# ---------------------------------------------------------------------------------------------------------------------
# 7-9: PeriodicEnergyModel(cell=): the oracle, lattice equivalence, rotation, strain and stress
# ---------------------------------------------------------------------------------------------------------------------
def _model_case(lmax, seed, M=200, H=16, layers=2, scalar_only=False):
    rng = np.random.default_rng(seed)
    pos = _dyadic(M, seed)
    unwrapped = (pos + rng.integers(-2, 3, size=pos.shape).astype(np.float64) @ T).astype(np.float32)  # exact
    x = rng.standard_normal((M, 4)).astype(np.float32)
    if scalar_only:
        x[:, 1:] = 0.0  # a rotation of every edge vector leaves the energy unchanged: W is symmetric
    torch.manual_seed(seed + 1)
    model = PeriodicEnergyModel("1x0e+1x1o", H, layers, lmax=lmax).to(DEV).eval()
    return model, x, unwrapped, 0.2


def _oracle(model, x, pos, r, lmax, H=16, layers=2):
    """e, forces (caller order), dE/deps of the fp64 restatement on the graph of T."""
    g = radius_graph(torch.as_tensor(pos).to(DEV), r, cell=T.tolist())
    perm = g.perm.cpu().numpy()
    params = {k[len("net."):]: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    e, f, dE = R.energy_forces_strain_cell(params, H, layers, lmax, "1x0e+1x1o", x[perm].astype(np.float64),
                                           pos[perm].astype(np.float64), g.rowptr.cpu().numpy(), g.src.cpu().numpy(), T)
    f_want = np.empty_like(f)
    f_want[perm] = f
    return e, f_want, dE, g


@pytest.mark.parametrize("lmax", [1, 2])
def test_cell_model_vs_oracle(lmax):
    model, x, pos, r = _model_case(lmax, 21)
    xd, pd = torch.as_tensor(x).to(DEV), torch.as_tensor(pos).to(DEV)
    with _quiet():
        e, f, W, sigma = model(xd, pd, r, cell=T.tolist(), forces=True, virial=True, stress=True)
        e_only = model(xd, pd, r, cell=torch.as_tensor(T))
    assert e.dim() == 0 and f.shape == (200, 3) and W.shape == (3, 3) and sigma.shape == (3, 3)
    e_ref, f_ref, dE, _ = _oracle(model, x, pos, r, lmax)
    assert abs(float(e) - e_ref) < 1e-5 * max(1.0, abs(e_ref)), (float(e), e_ref)
    assert abs(float(e_only) - e_ref) < 1e-5 * max(1.0, abs(e_ref))
    assert rel(f, f_ref) < 2e-5, rel(f, f_ref)
    assert rel(W, -dE) < 2e-5, rel(W, -dE)
    assert rel(sigma, dE / VOL) < 2e-5, rel(sigma, dE / VOL)
    # sigma = -W / V with V = |det T| = 0.65625
    assert np.allclose(sigma.double().cpu().numpy(), -W.double().cpu().numpy() / VOL, rtol=1e-6,
                       atol=1e-7 * float(sigma.abs().max()))
    # the requested subset, in the documented order
    with _quiet():
        out = model(xd, pd, r, cell=T.tolist(), stress=True)
        out2 = model(xd, pd, r, cell=T.tolist(), forces=True, stress=True)
    assert len(out) == 2 and rel(out[1], dE / VOL) < 2e-5
    assert len(out2) == 3 and rel(out2[1], f_ref) < 2e-5 and rel(out2[2], dE / VOL) < 2e-5


@pytest.mark.parametrize("lmax", [1, 2])
def test_lattice_equivalence(lmax):
    """The same points under T and under T' = M T (the same lattice, other basis vectors and heights)."""
    model, x, pos, r = _model_case(lmax, 23)
    xd, pd = torch.as_tensor(x).to(DEV), torch.as_tensor(pos).to(DEV)
    e_ref, f_ref, dE, g_t = _oracle(model, x, pos, r, lmax)
    g_tp = radius_graph(pd, r, cell=TP.tolist())
    assert np.array_equal(_pairs(g_t), _pairs(g_tp)) and g_t.num_edges > 0
    assert g_tp.volume == VOL and g_tp.grid != g_t.grid
    for cell in (T, TP):
        with _quiet():
            e, f, sigma = model(xd, pd, r, cell=cell.tolist(), forces=True, stress=True)
        assert abs(float(e) - e_ref) < 1e-5 * max(1.0, abs(e_ref)), (float(e), e_ref)
        assert rel(f, f_ref) < 2e-5, rel(f, f_ref)
        assert rel(sigma, dE / VOL) < 2e-5, rel(sigma, dE / VOL)


def test_rotation():
    """The rotated cell, positions and 1o input on the GPU against the rotated oracle of T.  The oracle takes the
    back-rotation (fp64) of exactly the fp32 numbers the GPU sees, so the rounding of the rotated inputs is not in the
    comparison; the points sit on a jittered lattice, wrapped, so that no pair is close enough to amplify the fp32
    rounding of a coordinate difference."""
    lmax, M, H, layers, r = 2, 200, 16, 2, 0.2
    rng = np.random.default_rng(25)
    sites = np.array([[i, j, k] for i in range(6) for j in range(6) for k in range(6)], np.float64)[rng.permutation(216)[:M]]
    pos = ((sites + 0.25 + 0.5 * rng.random((M, 3))) / 6.0) @ T
    x = rng.standard_normal((M, 4)).astype(np.float32)
    torch.manual_seed(26)
    model = PeriodicEnergyModel("1x0e+1x1o", H, layers, lmax=lmax).to(DEV).eval()
    Q = R.rotation()
    cell_q = (T @ Q.T).astype(np.float32)  # every lattice vector rotated
    pos_q = (pos @ Q.T).astype(np.float32)
    x_q = x.copy()
    x_q[:, 1:] = (x[:, 1:].astype(np.float64) @ Q.T).astype(np.float32)  # the 1o input turns with the frame
    with _quiet():
        e, f, sigma = model(torch.as_tensor(x_q).to(DEV), torch.as_tensor(pos_q).to(DEV), r, cell=cell_q.tolist(),
                            forces=True, stress=True)
    # the oracle in the frame of T
    cell_b, pos_b = cell_q.astype(np.float64) @ Q, pos_q.astype(np.float64) @ Q
    x_b = x_q.astype(np.float64)
    x_b[:, 1:] = x_b[:, 1:] @ Q
    g = radius_graph(torch.as_tensor(pos_q).to(DEV), r, cell=cell_q.tolist())
    perm = g.perm.cpu().numpy()
    params = {k[len("net."):]: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    e_ref, f_ref, dE = R.energy_forces_strain_cell(params, H, layers, lmax, "1x0e+1x1o", x_b[perm], pos_b[perm],
                                                   g.rowptr.cpu().numpy(), g.src.cpu().numpy(), cell_b)
    f_want = np.empty_like(f_ref)
    f_want[perm] = f_ref
    vol = abs(np.linalg.det(cell_b))
    assert abs(float(e) - e_ref) < 1e-5 * max(1.0, abs(e_ref)), (float(e), e_ref)
    assert rel(f, f_want @ Q.T) < 2e-5, rel(f, f_want @ Q.T)
    assert rel(sigma, Q @ (dE / vol) @ Q.T) < 2e-5, rel(sigma, Q @ (dE / vol) @ Q.T)
    # and the invariants against the unrotated GPU run: the same energy, forces R f, stress R sigma R^T
    with _quiet():
        e0, f0, s0 = model(torch.as_tensor(x).to(DEV), torch.as_tensor(pos.astype(np.float32)).to(DEV), r,
                           cell=T.tolist(), forces=True, stress=True)
    assert abs(float(e) - float(e0)) < 1e-5 * max(1.0, abs(float(e0)))
    assert rel(f, f0.double().cpu().numpy() @ Q.T) < 1e-4 and rel(sigma, Q @ s0.double().cpu().numpy() @ Q.T) < 1e-4


def _graph(N, r, seed):
    return radius_graph(torch.as_tensor(_dyadic(N, seed)).to(DEV), r, cell=T.tolist())


def _geometry64(g, lmax, eps, sid, cell=T):
    """fp64 torch (on the device) Y, d, A of r + eps[s] r, r = the cell's minimum image of x_src - x_dst; differentiable
    w.r.t. the returned leaves pos64 [N,3] and eps64 [S,3,3]."""
    p64 = g.pos4[:, :3].double().detach().clone().requires_grad_(True)
    e64 = eps.double().detach().clone().requires_grad_(True)
    src, dst = g.src.long(), g.dst.long()
    r = p64[src] - p64[dst]
    c = torch.as_tensor(np.asarray(cell, np.float64), device=DEV)
    r = r - torch.round(r.detach() @ torch.linalg.inv(c)) @ c
    r = r + torch.einsum("eab,eb->ea", e64[sid.long()[dst]], r)
    d = r.norm(dim=1)
    u = r / d[:, None]
    parts = [torch.ones_like(d)[:, None], 3 ** 0.5 * u]
    if lmax == 2:
        x, y, z = u[:, 0], u[:, 1], u[:, 2]
        s3 = 3 ** 0.5
        parts.append(5 ** 0.5 * torch.stack([s3 * x * y, s3 * y * z, (2 * z * z - x * x - y * y) / 2, s3 * z * x,
                                             s3 / 2 * (x * x - y * y)], 1))
    Y = torch.cat(parts, 1)
    N = g.rowptr.numel() - 1
    deg = (g.rowptr[1:] - g.rowptr[:-1]).double().clamp_min(1)
    A = torch.cat([torch.ones(N, 1, device=DEV, dtype=torch.float64),
                   torch.zeros(N, Y.shape[1] - 1, device=DEV, dtype=torch.float64).index_add(0, dst, Y[:, 1:]) / deg[:, None]], 1)
    return Y, d, A, p64, e64


@pytest.mark.parametrize("lmax", [1, 2])
def test_zero_strain_is_bit_equal_to_the_unstrained_geometry(lmax):
    g = _graph(4000, 0.09, 27)
    N = g.rowptr.numel() - 1
    want = ops.edge_geometry(g, lmax=lmax)
    sid = torch.randint(0, 3, (N,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    for strain, structure in ((torch.zeros(3, 3, device=DEV), None), (torch.zeros(3, 3, 3, device=DEV), sid)):
        got = ops.edge_geometry(g, lmax=lmax, strain=strain, structure=structure)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    # unwrapped positions (whole lattice vectors added) through the strained entry too
    k = torch.randint(-2, 3, (N, 3), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)).float()
    p = g.pos4[:, :3] + k @ torch.as_tensor(T, dtype=torch.float32, device=DEV)
    got = ops.edge_geometry(g, lmax=lmax, pos=p, strain=torch.zeros(3, 3, device=DEV))
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("lmax", [1, 2])
@pytest.mark.parametrize("S", [1, 5])
def test_strained_geometry_and_backward_vs_fp64_autograd(lmax, S):
    g = _graph(5000, 0.09, 28)
    N = g.rowptr.numel() - 1
    gen = torch.Generator(device=DEV).manual_seed(7)
    eps = (1e-2 * torch.randn(S, 3, 3, device=DEV, generator=gen)).requires_grad_(True)  # off-diagonal terms included
    sid = torch.randint(0, S, (N,), device=DEV, generator=gen) if S > 1 else None
    pos = g.pos4[:, :3].clone().requires_grad_(True)
    Y, d, A = ops.edge_geometry(g, lmax=lmax, pos=pos, strain=eps, structure=sid)
    sid0 = sid if sid is not None else torch.zeros(N, dtype=torch.int64, device=DEV)
    Y64, d64, A64, p64, e64 = _geometry64(g, lmax, eps, sid0)
    assert rel(Y, Y64) < 2e-5 and rel(d, d64) < 2e-5 and rel(A, A64) < 2e-5, (rel(Y, Y64), rel(d, d64), rel(A, A64))
    Y0, _, _ = ops.edge_geometry(g, lmax=lmax)
    assert rel(Y.detach(), Y0) > 1e-3  # the strain does move the geometry
    # without a gradient the forward-only strained entry gives the same numbers
    Yn, dn, An = ops.edge_geometry(g, lmax=lmax, strain=eps.detach(), structure=sid)
    assert torch.equal(Yn, Y.detach()) and torch.equal(dn, d.detach()) and torch.equal(An, A.detach())
    wY, wd, wA = (torch.randn(t.shape, device=DEV, generator=gen) for t in (Y, d, A))
    gp, ge = torch.autograd.grad((Y * wY).sum() + (d * wd).sum() + (A * wA).sum(), [pos, eps])
    gp64, ge64 = torch.autograd.grad((Y64 * wY.double()).sum() + (d64 * wd.double()).sum() + (A64 * wA.double()).sum(),
                                     [p64, e64])
    assert rel(ge, ge64) < 2e-5, rel(ge, ge64)
    assert rel(gp, gp64) < 2e-5, rel(gp, gp64)


@pytest.mark.parametrize("lmax", [1, 2])
def test_zero_strain_backward_matches_plain_and_is_reproducible(lmax):
    g = _graph(20000, 0.05, 29)
    gen = torch.Generator(device=DEV).manual_seed(9)
    pos = g.pos4[:, :3].clone().requires_grad_(True)
    Y, d, A = ops.edge_geometry(g, lmax=lmax, pos=pos)
    wY, wd, wA = (torch.randn(t.shape, device=DEV, generator=gen) for t in (Y, d, A))
    (gp_plain,) = torch.autograd.grad((Y * wY).sum() + (d * wd).sum() + (A * wA).sum(), [pos])
    runs = []
    for _ in range(2):
        eps = torch.zeros(3, 3, device=DEV, requires_grad=True)
        Y, d, A = ops.edge_geometry(g, lmax=lmax, pos=pos, strain=eps)
        runs.append(torch.autograd.grad((Y * wY).sum() + (d * wd).sum() + (A * wA).sum(), [pos, eps]))
    assert rel(runs[0][0], gp_plain) < 1e-6, rel(runs[0][0], gp_plain)  # atomics: order of arrival only
    assert torch.equal(runs[0][1], runs[1][1])  # S = 1: bitwise reproducible
    assert runs[0][1].shape == (3, 3) and float(runs[0][1].abs().max()) > 0


@pytest.mark.parametrize("lmax", [1, 2])
def test_stress_vs_central_differences_of_the_gpu_energy(lmax):
    model, x, pos, r = _model_case(lmax, 30, scalar_only=True)
    xd, pd = torch.as_tensor(x).to(DEV), torch.as_tensor(pos).to(DEV)
    with _quiet():
        e, W, sigma = model(xd, pd, r, cell=T.tolist(), virial=True, stress=True)
    g = radius_graph(pd, r, cell=T.tolist())
    perm = g.perm.long()

    def energy(eps):
        # a strain that requires grad routes the layers through the differentiable chain, the path that sees geometry=
        eps = eps.clone().requires_grad_(True)
        with _quiet(), torch.enable_grad():
            geom = ops.edge_geometry(g, lmax=lmax, pos=pd[perm], strain=eps)
            return float(model.net(xd[perm], g, geometry=geom)[:, 0].sum().double())

    delta = 1e-3
    fd = np.zeros((3, 3))
    for a in range(3):
        for b in range(3):
            ep = torch.zeros(3, 3, device=DEV)
            ep[a, b] = delta
            fd[a, b] = (energy(ep) - energy(-ep)) / (2 * delta) / VOL
    s = sigma.double().cpu().numpy()
    assert np.abs(s - fd).max() < 2e-3 * np.abs(s).max(), (s, fd)
    assert abs(energy(torch.zeros(3, 3, device=DEV)) - float(e)) < 1e-5 * max(1.0, abs(float(e)))
    Wn = W.double().cpu().numpy()
    assert np.abs(Wn - Wn.T).max() <= 1e-5 * np.abs(Wn).max(), Wn
    assert np.allclose(s, -Wn / VOL, rtol=1e-6, atol=1e-7 * np.abs(s).max())


# ---------------------------------------------------------------------------------------------------------------------
# 10: the open and orthorhombic paths are untouched
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("periodic", [False, True])
def test_existing_paths_unchanged(periodic):
    """A call that names ``cell=None`` is the call that never mentions it: graphs and geometry ``torch.equal``, and the
    forward ``torch.equal`` on the path with a fixed summation order (fuse_scatter = False).

    One relaxation of the issue's item 10 ("``torch.equal`` on graphs and forwards"): the one-launch forward scatters with
    float atomics, whose order of arrival differs between two launches of the same call, so it is not bitwise
    reproducible even against itself; it is compared at 1e-6 of the output scale (the same fp32 terms of a row summed
    in another order, far below the 1e-5 of the forward tolerances).  Both calls of a pair run in this build,
    so this test shows that the new keywords do not steer an open or orthorhombic call elsewhere; that the open and
    orthorhombic kernels themselves are the parent's is the instruction-count comparison of DESIGN.md section 5."""
    N, H, layers, r = 5000, 32, 2, 0.07
    pos = torch.as_tensor(_dyadic(N, 31, np.eye(3))).to(DEV)
    box = ([0, 0, 0], [1, 1, 1])
    a = radius_graph(pos, r, *box, periodic=periodic)
    b = radius_graph(pos, r, *box, periodic=periodic, cell=None, origin=None)
    assert a.cell is None and a.origin is None and a.volume is None and a.cell_arg is None
    assert (a.box is not None) == periodic and a.box == b.box and a.grid == b.grid
    for f in ("perm", "pos4", "rowptr", "src"):
        assert torch.equal(getattr(a, f), getattr(b, f))
    for lmax in (1, 2):
        for u, v in zip(ops.edge_geometry(a, lmax=lmax), ops.edge_geometry(b, lmax=lmax)):
            assert torch.equal(u, v)
    x = torch.randn(N, 4, generator=torch.Generator().manual_seed(32)).to(DEV)[a.perm.long()]
    torch.manual_seed(33)
    model = SEGNN("1x0e+1x1o", H, "1x1o", layers, lmax=2).to(DEV)
    with torch.no_grad():
        fused = model(x, a), model(x, b)
        for l in model.layers:
            l.fuse_scatter = False
        fixed = model(x, a), model(x, b)
    assert torch.equal(fixed[0], fixed[1])
    assert rel(fused[0], fused[1]) < 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# 11: error paths
# ---------------------------------------------------------------------------------------------------------------------
def test_error_paths():
    model, x, pos, r = _model_case(1, 34, M=50, H=8)
    xd, pd = torch.as_tensor(x).to(DEV), torch.as_tensor(pos).to(DEV)
    g = radius_graph(pd, r, cell=T.tolist())
    perm = g.perm.long()
    # a cell graph cannot be sharded, like a periodic box
    for kw in (dict(halo=object()), dict(split=object())):
        with pytest.raises(NotImplementedError):
            model.net(xd[perm], g, **kw)
    # stress=True is not refused for a cell (it is for a box with an open axis)
    with _quiet():
        out = model(xd, pd, r, cell=T.tolist(), stress=True)
    assert len(out) == 2 and out[1].shape == (3, 3)
    with pytest.raises(ValueError):
        model(xd, pd, r, [0, 0, 0], [1, 1, 1], periodic=(True, True, False), stress=True)
    # a cell together with the orthorhombic arguments, bad shapes, a cutoff beyond the heights
    for kw in (dict(lo=[0, 0, 0], hi=[1, 1, 1]), dict(periodic=False), dict(periodic=(True, True, True))):
        with pytest.raises(ValueError):
            model(xd, pd, r, cell=T.tolist(), **kw)
    for bad in ([[1, 0, 0], [0, 1, 0]], [1.0] * 9, torch.eye(3, device=DEV), np.eye(4).tolist()):
        with pytest.raises(ValueError):
            radius_graph(pd, r, cell=bad)
    with pytest.raises(ValueError, match="height"):
        radius_graph(pd, 0.375, cell=T.tolist())
    with pytest.raises(ValueError):
        radius_graph(pd, r, cell=T.tolist(), origin=[0.0, 0.0])
    with pytest.raises(RuntimeError):
        radius_graph(pd.double(), r, cell=T.tolist())
    N = g.rowptr.numel() - 1
    for bad in (torch.zeros(3, device=DEV), torch.zeros(3, 2, device=DEV), torch.zeros(0, 3, 3, device=DEV)):
        with pytest.raises(ValueError):
            ops.edge_geometry(g, lmax=1, strain=bad)
    with pytest.raises(ValueError):
        ops.edge_geometry(g, lmax=1, strain=torch.zeros(2, 3, 3, device=DEV),
                          structure=torch.zeros(N + 1, dtype=torch.int32, device=DEV))

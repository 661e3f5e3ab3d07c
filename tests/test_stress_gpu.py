"""Strain, virial and stress on the GPU (include/e3gnn.h, e3_edge_geometry_strained / e3_edge_geometry_backward_strained;
ops.edge_geometry(strain=, structure=); BatchedEnergyModel(virial=True); PeriodicEnergyModel).

The strained geometry against the unstrained entries (bit for bit at eps = 0) and fp64 geometry of r + eps r, its
backward against fp64 torch autograd, the models against the fp64 restatement (tests/virial_reference.py) and the
stress against central differences of the GPU energy.  Tolerances: 2e-5 of the output scale for energies, forces,
virials and stresses (as tests/test_forces_gpu.py)."""
import contextlib
import warnings

import numpy as np
import pytest
import torch

import pbc_reference as P
import virial_reference as V
from scalable_e3_gnn_amd import ops
from scalable_e3_gnn_amd.batched import BatchedEnergyModel, PeriodicEnergyModel, batched_radius_graph
from scalable_e3_gnn_amd.radius_graph import radius_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rel(a, b):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _dyadic(n, seed):
    """Uniform in [0, 1) on the 2^-16 grid (edge vectors, whole-period shifts and translations exact in fp32)."""
    return (np.random.default_rng(seed).integers(0, 1 << 16, size=(n, 3)) / float(1 << 16)).astype(np.float32)


def _graph(N, r, periodic, seed):
    return radius_graph(torch.as_tensor(_dyadic(N, seed)).to(DEV), r, [0, 0, 0], [1, 1, 1], periodic=periodic)


@contextlib.contextmanager
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # "the unfused differentiable chain runs": what is used here
        yield


def _geometry64(g, lmax, eps, sid, pos=None):
    """fp64 torch (on the device) Y, d, A of r + eps[s] r, r = minimum image of x_src - x_dst; differentiable w.r.t. the
    returned leaves pos64 [N,3] and eps64 [S,3,3]."""
    p64 = (g.pos4[:, :3] if pos is None else pos).double().detach().clone().requires_grad_(True)
    e64 = eps.double().detach().clone().requires_grad_(True)
    src, dst = g.src.long(), g.dst.long()
    r = p64[src] - p64[dst]
    if g.box is not None:
        L = torch.tensor(g.box, dtype=torch.float64, device=DEV)
        r = r - torch.where(L > 0, L * torch.round(r.detach() / torch.where(L > 0, L, 1.0)), 0.0)
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


# ---------------------------------------------------------------------------------------------------------------------
# 1-3: the strained geometry and its backward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lmax", [1, 2])
@pytest.mark.parametrize("periodic", [False, True])
def test_zero_strain_is_bit_equal_to_the_unstrained_geometry(lmax, periodic):
    g = _graph(4000, 0.07, periodic, 1)
    N = g.rowptr.numel() - 1
    want = ops.edge_geometry(g, lmax=lmax)
    sid = torch.randint(0, 3, (N,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    for strain, structure in ((torch.zeros(3, 3, device=DEV), None), (torch.zeros(3, 3, 3, device=DEV), sid)):
        got = ops.edge_geometry(g, lmax=lmax, strain=strain, structure=structure)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    # unwrapped positions (whole periods added on the periodic axes) through the strained entry too
    shifts = torch.randint(-2, 3, (N, 3), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)).float()
    p = g.pos4[:, :3] + (shifts if periodic else 0.0)
    got = ops.edge_geometry(g, lmax=lmax, pos=p, strain=torch.zeros(3, 3, device=DEV))
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("lmax", [1, 2])
@pytest.mark.parametrize("periodic", [False, (True, False, True)])
def test_strained_geometry_vs_fp64(lmax, periodic):
    g = _graph(6000, 0.06, periodic, 4)
    N = g.rowptr.numel() - 1
    gen = torch.Generator(device=DEV).manual_seed(5)
    S = 3
    eps = 1e-2 * torch.randn(S, 3, 3, device=DEV, generator=gen)  # off-diagonal terms included
    sid = torch.randint(0, S, (N,), device=DEV, generator=gen)
    Y, d, A = ops.edge_geometry(g, lmax=lmax, strain=eps, structure=sid)
    Y64, d64, A64, _, _ = _geometry64(g, lmax, eps, sid)
    assert rel(Y, Y64) < 4e-6 and rel(d, d64) < 4e-6 and rel(A, A64) < 4e-6, (rel(Y, Y64), rel(d, d64), rel(A, A64))
    # the strain does move the geometry
    Y0, _, _ = ops.edge_geometry(g, lmax=lmax)
    assert rel(Y, Y0) > 1e-3


@pytest.mark.parametrize("lmax", [1, 2])
@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("S", [1, 5])
def test_strained_backward_vs_fp64_autograd(lmax, periodic, S):
    g = _graph(5000, 0.07, periodic, 6)
    N = g.rowptr.numel() - 1
    gen = torch.Generator(device=DEV).manual_seed(7)
    eps = (1e-2 * torch.randn(S, 3, 3, device=DEV, generator=gen)).requires_grad_(True)
    sid = torch.randint(0, S, (N,), device=DEV, generator=gen) if S > 1 else None
    pos = g.pos4[:, :3].clone().requires_grad_(True)
    Y, d, A = ops.edge_geometry(g, lmax=lmax, pos=pos, strain=eps, structure=sid)
    wY, wd, wA = (torch.randn(t.shape, device=DEV, generator=gen) for t in (Y, d, A))
    gp, ge = torch.autograd.grad((Y * wY).sum() + (d * wd).sum() + (A * wA).sum(), [pos, eps])
    sid0 = sid if sid is not None else torch.zeros(N, dtype=torch.int64, device=DEV)
    Y64, d64, A64, p64, e64 = _geometry64(g, lmax, eps, sid0)
    gp64, ge64 = torch.autograd.grad((Y64 * wY.double()).sum() + (d64 * wd.double()).sum() + (A64 * wA.double()).sum(),
                                     [p64, e64])
    assert rel(ge, ge64) < 1e-5, rel(ge, ge64)
    assert rel(gp, gp64) < 2e-5, rel(gp, gp64)


@pytest.mark.parametrize("lmax", [1, 2])
def test_zero_strain_backward_matches_plain_and_is_reproducible(lmax):
    g = _graph(20000, 0.04, True, 8)
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


# ---------------------------------------------------------------------------------------------------------------------
# 4-6: PeriodicEnergyModel
# ---------------------------------------------------------------------------------------------------------------------
def _periodic_case(lmax, periodic, seed, M=200, H=16, layers=2, scalar_only=False):
    rng = np.random.default_rng(seed)
    pos = _dyadic(M, seed)
    axes = np.array(P.axes_of(periodic), np.float64)
    unwrapped = (pos + rng.integers(-2, 3, size=pos.shape) * axes).astype(np.float32)  # whole periods, exact
    x = rng.standard_normal((M, 4)).astype(np.float32)
    if scalar_only:
        x[:, 1:] = 0.0  # a rotation of every edge vector leaves the energy unchanged: W is symmetric
    torch.manual_seed(seed + 1)
    model = PeriodicEnergyModel("1x0e+1x1o", H, layers, lmax=lmax).to(DEV).eval()
    return model, x, unwrapped, 0.2


def _oracle(model, x, pos, r, periodic, lmax, H=16, layers=2):
    g = radius_graph(torch.as_tensor(pos).to(DEV), r, [0, 0, 0], [1, 1, 1], periodic=periodic)
    perm = g.perm.cpu().numpy()
    params = {k[len("net."):]: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    L = g.box if g.box is not None else (0.0, 0.0, 0.0)
    e, f, dE = V.energy_forces_strain(params, H, layers, lmax, "1x0e+1x1o", x[perm].astype(np.float64),
                                      pos[perm].astype(np.float64), g.rowptr.cpu().numpy(), g.src.cpu().numpy(), L)
    f_want = np.empty_like(f)
    f_want[perm] = f
    return e, f_want, dE[0], L


@pytest.mark.parametrize("lmax", [1, 2])
def test_periodic_model_vs_oracle(lmax):
    model, x, pos, r = _periodic_case(lmax, True, 10)
    xd, pd = torch.as_tensor(x).to(DEV), torch.as_tensor(pos).to(DEV)
    with _quiet():
        e, f, W, sigma = model(xd, pd, r, [0, 0, 0], [1, 1, 1], forces=True, virial=True, stress=True)
        e_only = model(xd, pd, r, [0, 0, 0], [1, 1, 1])
    assert e.dim() == 0 and f.shape == (200, 3) and W.shape == (3, 3) and sigma.shape == (3, 3)
    e_ref, f_ref, dE, L = _oracle(model, x, pos, r, True, lmax)
    Vol = float(L[0]) * float(L[1]) * float(L[2])
    assert abs(float(e) - e_ref) < 1e-5 * max(1.0, abs(e_ref)), (float(e), e_ref)
    assert abs(float(e_only) - e_ref) < 1e-5 * max(1.0, abs(e_ref))
    assert rel(f, f_ref) < 2e-5, rel(f, f_ref)
    assert rel(W, -dE) < 2e-5, rel(W, -dE)
    assert rel(sigma, dE / Vol) < 2e-5, rel(sigma, dE / Vol)
    # the requested subset, in the documented order
    with _quiet():
        out = model(xd, pd, r, [0, 0, 0], [1, 1, 1], stress=True)
    assert len(out) == 2 and rel(out[1], dE / Vol) < 2e-5


def test_periodic_model_virial_with_an_open_axis():
    periodic = (True, True, False)
    model, x, pos, r = _periodic_case(2, periodic, 11)
    with _quiet():
        e, W = model(torch.as_tensor(x).to(DEV), torch.as_tensor(pos).to(DEV), r, [0, 0, 0], [1, 1, 1],
                     periodic=periodic, virial=True)
    e_ref, _, dE, _ = _oracle(model, x, pos, r, periodic, 2)
    assert abs(float(e) - e_ref) < 1e-5 * max(1.0, abs(e_ref))
    assert rel(W, -dE) < 2e-5, rel(W, -dE)


@pytest.mark.parametrize("lmax", [1, 2])
def test_stress_vs_central_differences_of_the_gpu_energy(lmax):
    model, x, pos, r = _periodic_case(lmax, True, 12, scalar_only=True)
    xd, pd = torch.as_tensor(x).to(DEV), torch.as_tensor(pos).to(DEV)
    with _quiet():
        e, W, sigma = model(xd, pd, r, [0, 0, 0], [1, 1, 1], virial=True, stress=True)
    g = radius_graph(pd, r, [0, 0, 0], [1, 1, 1], periodic=True)
    perm = g.perm.long()
    Vol = g.box[0] * g.box[1] * g.box[2]

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
            fd[a, b] = (energy(ep) - energy(-ep)) / (2 * delta) / Vol
    s = sigma.double().cpu().numpy()
    assert np.abs(s - fd).max() < 2e-3 * np.abs(s).max(), (s, fd)
    assert abs(energy(torch.zeros(3, 3, device=DEV)) - float(e)) < 1e-5 * max(1.0, abs(float(e)))
    Wn = W.double().cpu().numpy()
    assert np.abs(Wn - Wn.T).max() <= 1e-5 * np.abs(Wn).max(), Wn
    assert np.allclose(s, -Wn / Vol, rtol=1e-6, atol=1e-7 * np.abs(s).max())


def test_stress_translation_invariance_and_unchanged_forces_100k():
    N, H, layers, lmax = 100000, 32, 2, 2
    r = float((3 * 24.0 / (4 * np.pi * N)) ** (1 / 3))
    pos = _dyadic(N, 13)
    x = np.random.default_rng(14).standard_normal((N, 4)).astype(np.float32)
    torch.manual_seed(15)
    model = PeriodicEnergyModel("1x0e+1x1o", H, layers, lmax=lmax).to(DEV)
    t = _dyadic(1, 16)[0]
    moved = (pos + t).astype(np.float32)  # exact: outside the box, wrapped by the builder
    xd = torch.as_tensor(x).to(DEV)
    box = ([0, 0, 0], [1, 1, 1])
    with _quiet():
        e, f, sigma = model(xd, torch.as_tensor(pos).to(DEV), r, *box, forces=True, stress=True)
        _, sigma2 = model(xd, torch.as_tensor(moved).to(DEV), r, *box, stress=True)
        e3, f3 = model(xd, torch.as_tensor(pos).to(DEV), r, *box, forces=True)
    assert rel(sigma2, sigma) < 1e-5, rel(sigma2, sigma)
    assert rel(f, f3) < 1e-5, rel(f, f3)  # the strained backward at eps = 0: atomics' order of arrival only
    assert abs(float(e3) - float(e)) <= 1e-6 * abs(float(e))
    assert float(sigma.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# 7: BatchedEnergyModel(virial=True)
# ---------------------------------------------------------------------------------------------------------------------
def make_batch(seed, n_mol):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(3, 30, n_mol)  # QM9-shaped: 3..29 atoms
    pos = np.concatenate([rng.normal(size=(n, 3)) * 1.5 + rng.uniform(-40, 40, 3) for n in sizes]).astype(np.float32)
    batch = np.concatenate([np.full(n, i) for i, n in enumerate(sizes)])
    order = rng.permutation(len(batch))
    return pos[order], batch[order], sizes


def test_batched_model_virial():
    pos, batch, sizes = make_batch(5, 128)
    r, H, layers, lmax = 5.0, 16, 2, 2
    n_mol = len(sizes)
    torch.manual_seed(6)
    model = BatchedEnergyModel("1x0e+1x1o", H, layers, lmax=lmax).to(DEV).eval()
    x = torch.randn(len(batch), 4, generator=torch.Generator().manual_seed(7))
    xd, pd, bd = x.to(DEV), torch.from_numpy(pos).to(DEV), torch.from_numpy(batch).to(DEV)
    with _quiet():
        e, f, W = model(xd, pd, bd, r, forces=True, virial=True)
        e_v, W_v = model(xd, pd, bd, r, virial=True)
        e0, f0 = model(xd, pd, bd, r, forces=True)
    assert W.shape == (n_mol, 3, 3) and e.shape == (n_mol,)
    assert rel(e, e0) < 1e-6 and rel(f, f0) < 1e-6, (rel(e, e0), rel(f, f0))
    assert rel(e_v, e0) < 1e-6 and rel(W_v, W) < 1e-5
    # the oracle per molecule on the model's graph
    g, mol = batched_radius_graph(pd, bd, r)
    perm = g.perm.cpu().numpy()
    params = {k[len("net."):]: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    E64, _, dE = V.energy_forces_strain(params, H, layers, lmax, "1x0e+1x1o", x.double().numpy()[perm],
                                        pos.astype(np.float64)[perm], g.rowptr.cpu().numpy(), g.src.cpu().numpy(),
                                        structure=mol.cpu().numpy(), S=n_mol, per_structure=True)
    assert rel(e, E64) < 1e-5
    assert rel(W, -dE) < 2e-5, rel(W, -dE)
    # the molecules' virials sum to the one-structure virial of the batch
    with _quiet(), torch.enable_grad():
        eps = torch.zeros(3, 3, device=DEV, requires_grad=True)
        geom = ops.edge_geometry(g, lmax=lmax, pos=g.pos4[:, :3], strain=eps)
        (ge,) = torch.autograd.grad(model.net(xd[g.perm.long()], g, geometry=geom)[:, 0].sum(), [eps])
    assert rel(W.sum(0), -ge) < 1e-5, rel(W.sum(0), -ge)


# ---------------------------------------------------------------------------------------------------------------------
# 8: error paths
# ---------------------------------------------------------------------------------------------------------------------
def test_error_paths():
    model, x, pos, r = _periodic_case(1, True, 17, M=50, H=8)
    xd, pd = torch.as_tensor(x).to(DEV), torch.as_tensor(pos).to(DEV)
    for periodic in ((True, True, False), False):
        with pytest.raises(ValueError):
            model(xd, pd, r, [0, 0, 0], [1, 1, 1], periodic=periodic, stress=True)
    g = radius_graph(pd, r, [0, 0, 0], [1, 1, 1], periodic=True)
    N = g.rowptr.numel() - 1
    for bad in (torch.zeros(3, device=DEV), torch.zeros(3, 2, device=DEV), torch.zeros(2, 3, 4, device=DEV),
                torch.zeros(0, 3, 3, device=DEV)):
        with pytest.raises(ValueError):
            ops.edge_geometry(g, lmax=1, strain=bad)
    with pytest.raises(ValueError):
        ops.edge_geometry(g, lmax=1, strain=torch.zeros(2, 3, 3, device=DEV),
                          structure=torch.zeros(N + 1, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ops.edge_geometry(g, lmax=1, structure=torch.zeros(N, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError):
        ops.edge_geometry(g, lmax=1, strain=torch.zeros(3, 3))

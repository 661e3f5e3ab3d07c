"""Training on forces: dL/dtheta of a loss on energies AND forces (``forward(..., forces=True, create_graph=True)``) against
the fp64 torch restatement that is differentiated twice (tests/force_loss_reference.py).

Losses: L = 0.3 sum E + sum <c, F>  and  L = mean((F - F*)^2) + mean((E - E*)^2).  Norm: max |got - want| / max |want| per
parameter tensor, as tests/test_forces_gpu.py.  Bound per tensor: max(2e-5, 20 x yardstick), the yardstick being the error of
the SAME restatement run in fp32 on the CPU against fp64 for that tensor, computed by every case itself: 2e-5 is the
project's bound for first derivatives, and 20 is about the margin it keeps between that bound and its measured error; it
covers the summation order of the atomics and the fp16-split forward that produced the saved activations.

Measured on one MI355X (largest error of any parameter tensor / largest yardstick, over both losses): batched l_max 2 H 16
1.4e-6 / 1.0e-6, l_max 1 H 16 3.3e-6 / 8.8e-7, l_max 2 H 32 4.2e-6 / 3.8e-6; periodic box 1.8e-6 / 1.2e-6, cell 1.1e-6 / 1.4e-6,
box with a Verlet list 5.4e-7 / 1.2e-6 ("Second derivatives").  Without the feature every test here fails:
``create_graph=`` is a TypeError."""
import contextlib
import functools
import warnings

import numpy as np
import pytest
import torch

import models  # noqa: F401
import force_loss_reference as FR
import triclinic_reference as TR
from scalable_e3_gnn_amd.batched import (BatchedEnergyModel, PeriodicEnergyModel, ShardedEnergyModel,
                                         batched_radius_graph)
from scalable_e3_gnn_amd.neighbor_list import NeighborList
from scalable_e3_gnn_amd.radius_graph import radius_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IN = "1x0e+1x1o"
LAYERS = 2
LOSSES = ("linear", "matching")

CASES = {   # name -> (kind, l_max, hidden, size)
    "batched-l2-h16": ("batched", 2, 16, 12),
    "batched-l1-h16": ("batched", 1, 16, 12),
    "batched-l2-h32": ("batched", 2, 32, 6),
    "periodic-box": ("box", 2, 16, 60),
    "periodic-cell": ("cell", 2, 16, 60),
    "periodic-box-neighbors": ("neighbors", 1, 16, 60),
}
R_MOL, R_BOX, P_ENV, SKIN = 3.0, 0.3, 6, 0.05


@contextlib.contextmanager
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # "the unfused differentiable chain runs": what is used here
        yield


def make_batch(seed, n_mol, lo=3, hi=30):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(lo, hi, n_mol)                      # QM9-shaped: 3..29 atoms
    pos = np.concatenate([rng.normal(size=(n, 3)) * 1.5 + rng.uniform(-40, 40, 3) for n in sizes]).astype(np.float32)
    batch = np.concatenate([np.full(n, i) for i, n in enumerate(sizes)])
    order = rng.permutation(len(batch))
    return pos[order], batch[order]


def _params(model):
    return {k[len("net."):]: v.detach().cpu().numpy() for k, v in model.state_dict().items()}


def _grads(model):
    return {n[len("net."):]: p.grad.detach().double().cpu().numpy().copy() for n, p in model.named_parameters()}


def _losses(rng, n_atoms, n_e, E_scale, F_scale):
    c = rng.standard_normal((n_atoms, 3))
    return {"linear": FR.linear_loss(c),
            "matching": FR.matching_loss(E_scale * rng.standard_normal(n_e), F_scale * rng.standard_normal((n_atoms, 3)))}


@functools.lru_cache(maxsize=None)
def _run(name):
    """One case: the model's dL/dtheta for both losses from ONE graph, the fp64 reference and the fp32 yardstick.
    -> {loss: (got, want, yardstick)} of {parameter: array | float}, plus the outputs"""
    kind, lmax, H, size = CASES[name]
    seed = sorted(CASES).index(name)
    rng = np.random.default_rng(100 + seed)
    torch.manual_seed(200 + seed)
    ref_kw = {}
    if kind == "batched":
        pos, batch = make_batch(5 + seed, size)
        model = BatchedEnergyModel(IN, H, LAYERS, lmax=lmax).to(DEV)
        model.train(seed % 2 == 0)
        n_e = size
    else:
        T = TR.T
        frac = rng.integers(0, 1 << 16, size=(size, 3)) / float(1 << 16)
        pos = ((frac + rng.integers(-1, 2, size=frac.shape)) @ (T if kind == "cell" else np.eye(3))).astype(np.float32)
        model = PeriodicEnergyModel(IN, H, LAYERS, lmax=lmax, envelope=P_ENV).to(DEV)
        model.train(seed % 2 == 0)
        n_e = 1
        ref_kw["envelope"] = (float(np.float32(R_BOX)), P_ENV)
    x = rng.standard_normal((len(pos), 4)).astype(np.float32)
    xd, pd = torch.as_tensor(x).to(DEV), torch.as_tensor(pos).to(DEV)
    with _quiet():
        if kind == "batched":
            bd = torch.as_tensor(batch).to(DEV)
            e, f = model(xd, pd, bd, R_MOL, forces=True, create_graph=True)
            g, mol = batched_radius_graph(pd, bd, R_MOL)
            ref_kw.update(mol=mol.cpu().numpy(), n_mol=size)
        elif kind == "box":
            e, f = model(xd, pd, R_BOX, [0, 0, 0], [1, 1, 1], forces=True, create_graph=True)
            g = radius_graph(pd, R_BOX, [0, 0, 0], [1, 1, 1], periodic=True)
            ref_kw["L"] = g.box
        elif kind == "cell":
            e, f = model(xd, pd, R_BOX, cell=T.tolist(), forces=True, create_graph=True)
            g = radius_graph(pd, R_BOX, cell=T.tolist())
            ref_kw["cell"] = T
        else:
            nl = NeighborList(R_BOX, SKIN, [0, 0, 0], [1, 1, 1], periodic=True)
            e, f = model(xd, pd, R_BOX, forces=True, neighbors=nl, create_graph=True)
            g = nl.update(pd)   # nothing moved: the graph of the forward
            ref_kw["L"] = g.box
    assert e.requires_grad and f.requires_grad and f.shape == pd.shape
    perm = g.perm.long().cpu().numpy()
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    args = (_params(model), H, LAYERS, lmax, IN, x[perm].astype(np.float64), pos[perm].astype(np.float64),
            g.rowptr.cpu().numpy(), g.src.cpu().numpy())
    E64, F64, leaves64 = FR.energy_forces(*args, dtype=torch.float64, **ref_kw)
    E32, F32, leaves32 = FR.energy_forces(*args, dtype=torch.float32, **ref_kw)
    losses = _losses(rng, len(pos), n_e, float(E64.detach().abs().max()), float(F64.detach().abs().max()))
    caller = lambda F: F[torch.as_tensor(inv)]     # graph order -> the caller's atom order
    shape_e = lambda E: E if kind == "batched" else E[0]
    out = {"E": (e.detach().double().cpu().numpy(), shape_e(E64).detach().numpy()),
           "F": (f.detach().double().cpu().numpy(), caller(F64).detach().numpy()), "edges": g.num_edges}
    for ln in LOSSES:
        model.zero_grad()
        losses[ln](e, f).backward(retain_graph=True)
        got = _grads(model)
        want = FR.parameter_gradients(losses[ln](shape_e(E64), caller(F64)), leaves64, retain_graph=True)
        g32 = FR.parameter_gradients(losses[ln](shape_e(E32), caller(F32)), leaves32, retain_graph=True)
        out[ln] = (got, want, FR.worst(g32, want))
    model.zero_grad()
    return out


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("name", list(CASES))
def test_force_loss_parameter_gradients_vs_fp64(name, loss):
    res = _run(name)
    (e, E64), (f, F64) = res["E"], res["F"]
    assert np.abs(e - E64).max() < 1e-5 * max(1.0, np.abs(E64).max())
    assert np.abs(f - F64).max() < 2e-5 * np.abs(F64).max()
    got, want, yard = res[loss]
    assert set(got) == set(want)
    err = FR.worst(got, want)
    k = max(err, key=lambda n: err[n] / max(2e-5, 20 * yard[n]))
    print(f"\n{name} ({res['edges']} edges), {loss} loss: worst tensor {k}: err {err[k]:.2e}, fp32 yardstick {yard[k]:.2e}; "
          f"largest err {max(err.values()):.2e}, largest yardstick {max(yard.values()):.2e}")
    for n in want:
        assert np.abs(want[n]).max() > 0, n
        assert err[n] < max(2e-5, 20 * yard[n]), (n, err[n], yard[n])


def _dimers(n=12):
    """n well separated pairs of atoms, one molecule each (small inputs for the tests of the interface below)"""
    rng = np.random.default_rng(3)
    centre = rng.uniform(-30, 30, (n, 1, 3))
    pos = (centre + 0.6 * rng.standard_normal((n, 2, 3))).reshape(-1, 3).astype(np.float32)
    return pos, np.repeat(np.arange(n), 2), rng.standard_normal((2 * n, 4)).astype(np.float32)


def _dimer_gas(seed):
    """8 pairs of atoms 0.05 .. 0.1 apart, centred on the 2 x 2 x 2 lattice of spacing 1 / 2 of the periodic unit box (the
    pairs at k = 0 straddle a face): every atom has exactly one neighbour within 0.2.  As the gas of
    tests/test_neighbor_list_gpu.py, but 16 atoms, so that the parameter gradients have one value too (below)."""
    rng = np.random.default_rng(seed)
    c = np.array([[i, j, k] for i in range(2) for j in range(2) for k in range(2)]) / 2.0
    u = rng.standard_normal(c.shape)
    u *= rng.uniform(0.025, 0.05, (len(c), 1)) / np.linalg.norm(u, axis=1, keepdims=True)
    pos = np.concatenate([c + u, c - u])
    return pos[rng.permutation(len(pos))].astype(np.float32), rng.standard_normal((len(pos), 4)).astype(np.float32)


def test_create_graph_false_is_the_call_without_the_argument():
    """Energy, forces and the parameter gradients of an energy backward, compared with torch.equal between the call without
    the argument, a second such call, ``create_graph=False`` and (detached) ``create_graph=True``.

    The first-order backward sums with float atomics in the order of arrival, so two calls of the same code are bit-equal only
    where no such sum has more than two addends (a + b from zero is one value).  A gas of dimers at l_max = 1 is that for the
    forces (g_pos, g_h: one edge as source, one row sum).  The weight gradients of the one general product of an l_max = 1
    model, the readout, add one partial per tile of 8 rows (tp_bwd_w_kernel): 16 atoms are two tiles.  The L1TensorProduct
    weight gradients are reduced in a fixed order.  A molecular cloud at l_max = 2 follows with what holds on it: equal
    energies, and forces to the project's first-derivative bound (two summation orders of the same kernels)."""
    R, LO, HI = 0.2, [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
    pos, x = _dimer_gas(61)
    xd, pd = torch.as_tensor(x).to(DEV), torch.as_tensor(pos).to(DEV)
    g = radius_graph(pd, R, LO, HI, periodic=True)
    assert len(pos) == 16 and g.num_edges == 16 and bool(torch.all(g.rowptr[1:] - g.rowptr[:-1] == 1))
    torch.manual_seed(62)
    model = PeriodicEnergyModel(IN, 16, LAYERS, lmax=1).to(DEV).train()

    def run(**kw):
        model.zero_grad()
        with _quiet():
            e, f = model(xd, pd, R, LO, HI, forces=True, **kw)
        e.backward()
        return e.detach().clone(), f.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters()}, f.requires_grad

    e0, f0, g0, graph0 = run()
    assert float(f0.abs().max()) > 0 and all(float(v.abs().max()) > 0 for v in g0.values()) and not graph0
    for kw in ({}, {"create_graph": False}, {"create_graph": True}):
        e, f, grads, graph = run(**kw)
        assert torch.equal(e, e0) and torch.equal(f, f0), kw
        for n in g0:
            assert torch.equal(grads[n], g0[n]), (kw, n)
        assert graph == bool(kw.get("create_graph")), kw            # the forces carry a graph only on request
    # eval mode, first order: detached as before; with create_graph the graph is kept
    model.eval()
    with _quiet():
        e1, f1 = model(xd, pd, R, LO, HI, forces=True, create_graph=False)
        e2, f2 = model(xd, pd, R, LO, HI, forces=True, create_graph=True)
    assert not e1.requires_grad and not f1.requires_grad and e2.requires_grad and f2.requires_grad
    assert torch.equal(e1, e0) and torch.equal(f1, f0) and torch.equal(e2.detach(), e0) and torch.equal(f2.detach(), f0)
    # a molecular cloud, l_max = 2
    pos, batch = make_batch(5, 12)
    torch.manual_seed(1)
    model = BatchedEnergyModel(IN, 16, LAYERS, lmax=2).to(DEV).eval()
    xd, pd, bd = torch.randn(len(pos), 4, device=DEV), torch.as_tensor(pos).to(DEV), torch.as_tensor(batch).to(DEV)
    with _quiet():
        e0, f0 = model(xd, pd, bd, R_MOL, forces=True)
        ea, fa = model(xd, pd, bd, R_MOL, forces=True)
        e1, f1 = model(xd, pd, bd, R_MOL, forces=True, create_graph=False)
        e2, f2 = model(xd, pd, bd, R_MOL, forces=True, create_graph=True)
    top = float(f0.abs().max())
    diff = lambda a, b: float((a - b).abs().max()) / top
    print(f"\nmolecular cloud, forces, largest difference / largest force: two calls without the argument {diff(f0, fa):.1e}, "
          f"create_graph=False {diff(f0, f1):.1e}, create_graph=True {diff(f0, f2.detach()):.1e}")
    assert torch.equal(e0, ea) and torch.equal(e0, e1) and torch.equal(e0, e2.detach())
    assert diff(f0, f1) <= 2e-5 and diff(f0, f2.detach()) <= 2e-5


def test_refusals():
    pos, batch, x = _dimers(4)
    xd, pd, bd = (torch.as_tensor(t).to(DEV) for t in (x, pos, batch))
    bm = BatchedEnergyModel(IN, 16, 1, lmax=1).to(DEV)
    pm = PeriodicEnergyModel(IN, 16, 1, lmax=1, envelope=P_ENV).to(DEV)
    box = ([-40, -40, -40], [40, 40, 40])
    with pytest.raises(NotImplementedError, match="tangent"):
        bm(xd, pd, bd, R_MOL, forces=True, virial=True, create_graph=True)
    with pytest.raises(NotImplementedError, match="tangent"):
        pm(xd, pd, R_MOL, *box, forces=True, virial=True, create_graph=True)
    with pytest.raises(NotImplementedError, match="tangent"):
        pm(xd, pd, R_MOL, *box, forces=True, stress=True, create_graph=True)
    with pytest.raises(NotImplementedError, match="bf16"):
        bm(xd.bfloat16(), pd, bd, R_MOL, forces=True, create_graph=True)
    with pytest.raises(NotImplementedError, match="refresh"):
        ShardedEnergyModel(IN, 16, 1, lmax=1).to(DEV)(xd, pd, R_MOL, None, forces=True, create_graph=True)
    with pytest.raises(ValueError, match="forces=True"):
        bm(xd, pd, bd, R_MOL, create_graph=True)
    bm.requires_grad_(False)
    with pytest.raises(ValueError, match="requires grad"):
        bm(xd, pd, bd, R_MOL, forces=True, create_graph=True)


def test_backward_twice_on_one_graph():
    pos, batch, x = _dimers(6)
    xd, pd, bd = (torch.as_tensor(t).to(DEV) for t in (x, pos, batch))
    torch.manual_seed(2)
    model = BatchedEnergyModel(IN, 16, 1, lmax=2).to(DEV)
    with _quiet():
        e, f = model(xd, pd, bd, R_MOL, forces=True, create_graph=True)
    loss = e.sum() + f.square().sum()
    loss.backward(retain_graph=True)
    once = {n: p.grad.clone() for n, p in model.named_parameters()}
    loss.backward()                                   # accumulates, as torch does; the graph is freed now
    for n, p in model.named_parameters():
        assert float(once[n].abs().max()) > 0, n
        assert float((p.grad - 2 * once[n]).abs().max()) <= 1e-5 * float(once[n].abs().max()), n
    with pytest.raises(RuntimeError, match="second time|already been freed"):
        loss.backward()

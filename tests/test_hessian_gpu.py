"""Hessian-vector products of the energy models (``hessian_vector_product`` / ``hessian``) against fp64 torch autograd of the
restatement (tests/hessian_reference.py over tests/force_loss_reference.py), at the shapes of tests/test_force_loss_gpu.py.

Norm: max |got - want| / max |want| per vector.  Bound: max(2e-5, 20 x yardstick), the yardstick being the SAME restatement
run in fp32 on the CPU against fp64 for that vector, computed by every case itself (the project's bound for derivatives of fp32
kernels and the margin it keeps, as tests/test_force_loss_gpu.py).  Symmetry and translation invariance are held to the same
bound relative to max |H v|: with delta the error of H v, |<u, H v> - <v, H u>| <= |u|_1 max|delta_v| + |v|_1 max|delta_u|, so
the difference is divided by |u|_1 max |H .| (u and v are drawn alike); H t = 0 for a uniform translation t with |t|_max = 1,
beside random v with |v|_max ~ 3.

Measured on one MI355X (largest error of any vector / largest yardstick): batched l_max 2 6.5e-7 / 5.1e-7, l_max 1 5.5e-7 /
5.5e-7; periodic box 6.9e-7 / 6.8e-7, cell 5.5e-7 / 4.5e-7, box with a Verlet list 6.2e-7 / 6.7e-7; asymmetry 1e-9 .. 4e-9,
H t exactly 0; dense Hessian of 6 atoms 3.4e-7, its asymmetry 9.6e-8 ("Hessian-vector products").  Without the
feature every test here fails: the models have no ``hessian_vector_product``."""
import functools

import numpy as np
import pytest
import torch

import models  # noqa: F401
import hessian_reference as HR
import triclinic_reference as TR
from scalable_e3_gnn_amd.batched import (HESSIAN_MAX_ATOMS, BatchedEnergyModel, PeriodicEnergyModel, ShardedEnergyModel,
                                         batched_radius_graph)
from scalable_e3_gnn_amd.neighbor_list import NeighborList
from scalable_e3_gnn_amd.radius_graph import radius_graph
from test_force_loss_gpu import _dimer_gas, _quiet, make_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IN = "1x0e+1x1o"
LAYERS = 2
K = 3
CASES = {   # name -> (kind, l_max, hidden, size, frozen in eval())
    "batched-l2-h16": ("batched", 2, 16, 12, True),
    "batched-l1-h16": ("batched", 1, 16, 12, False),
    "periodic-box": ("box", 2, 16, 60, False),
    "periodic-cell": ("cell", 2, 16, 60, True),
    "periodic-box-neighbors": ("neighbors", 1, 16, 60, False),
}
R_MOL, R_BOX, P_ENV, SKIN = 3.0, 0.3, 6, 0.05
TRANSLATION = (0.3, -1.0, 0.7)


def _params(model):
    return {k[len("net."):]: v.detach().cpu().numpy() for k, v in model.state_dict().items()}


@functools.lru_cache(maxsize=None)
def _run(name):
    """One case -> got [K + 1, N, 3] (K random v and the translation, caller order), the fp64 reference, the fp32 restatement,
    the vectors, and whether any parameter has a .grad afterwards"""
    kind, lmax, H, size, frozen = CASES[name]
    seed = sorted(CASES).index(name)
    rng = np.random.default_rng(300 + seed)
    torch.manual_seed(400 + seed)
    ref_kw = {}
    if kind == "batched":
        pos, batch = make_batch(5 + seed, size)
        model = BatchedEnergyModel(IN, H, LAYERS, lmax=lmax).to(DEV)
    else:
        T = TR.T
        frac = rng.integers(0, 1 << 16, size=(size, 3)) / float(1 << 16)
        pos = ((frac + rng.integers(-1, 2, size=frac.shape)) @ (T if kind == "cell" else np.eye(3))).astype(np.float32)
        model = PeriodicEnergyModel(IN, H, LAYERS, lmax=lmax, envelope=P_ENV).to(DEV)
        ref_kw["envelope"] = (float(np.float32(R_BOX)), P_ENV)
    if frozen:
        model.requires_grad_(False).eval()
    else:
        model.train()
    x = rng.standard_normal((len(pos), 4)).astype(np.float32)
    v = np.concatenate([rng.standard_normal((K, len(pos), 3)), np.broadcast_to(TRANSLATION, (1, len(pos), 3))]).astype(np.float32)
    xd, pd, vd = torch.as_tensor(x).to(DEV), torch.as_tensor(pos).to(DEV), torch.as_tensor(v).to(DEV)
    with _quiet():
        if kind == "batched":
            bd = torch.as_tensor(batch).to(DEV)
            hv = model.hessian_vector_product(xd, pd, bd, R_MOL, vd)
            g, mol = batched_radius_graph(pd, bd, R_MOL)
            ref_kw.update(mol=mol.cpu().numpy(), n_mol=size)
        elif kind == "box":
            hv = model.hessian_vector_product(xd, pd, R_BOX, [0, 0, 0], [1, 1, 1], v=vd)
            g = radius_graph(pd, R_BOX, [0, 0, 0], [1, 1, 1], periodic=True)
            ref_kw["L"] = g.box
        elif kind == "cell":
            hv = model.hessian_vector_product(xd, pd, R_BOX, cell=T.tolist(), v=vd)
            g = radius_graph(pd, R_BOX, cell=T.tolist())
            ref_kw["cell"] = T
        else:
            nl = NeighborList(R_BOX, SKIN, [0, 0, 0], [1, 1, 1], periodic=True)
            hv = model.hessian_vector_product(xd, pd, R_BOX, v=vd, neighbors=nl)
            g = nl.update(pd)   # nothing moved: the graph of the call
            ref_kw["L"] = g.box
    assert hv.shape == vd.shape and not hv.requires_grad and hv.dtype == torch.float32
    has_grad = [n for n, p in model.named_parameters() if p.grad is not None]
    perm = g.perm.long().cpu().numpy()
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    args = (_params(model), H, LAYERS, lmax, IN, x[perm].astype(np.float64), pos[perm].astype(np.float64),
            g.rowptr.cpu().numpy(), g.src.cpu().numpy())
    want = HR.Reference(*args, dtype=torch.float64, **ref_kw).hvp(v[:, perm])[:, inv]
    f32 = HR.Reference(*args, dtype=torch.float32, **ref_kw).hvp(v[:, perm])[:, inv]
    return hv.double().cpu().numpy(), want, f32, v.astype(np.float64), has_grad, g.num_edges


def _bound(f32, want):
    return max(2e-5, 20 * HR.rel_max(f32, want))


@pytest.mark.parametrize("name", list(CASES))
def test_hessian_vector_products_vs_fp64(name):
    got, want, f32, v, has_grad, E = _run(name)
    assert not has_grad, has_grad
    for k in range(K):
        err, yard = HR.rel_max(got[k], want[k]), HR.rel_max(f32[k], want[k])
        print(f"\n{name} ({E} edges), v{k}: max |H v| = {np.abs(want[k]).max():.3e}, err {err:.2e}, fp32 yardstick {yard:.2e}")
        assert np.abs(want[k]).max() > 0
        assert err < _bound(f32[k], want[k]), (k, err, yard)


@pytest.mark.parametrize("name", list(CASES))
def test_symmetry_and_translation(name):
    got, want, f32, v, _, _ = _run(name)
    bound = max(_bound(f32[k], want[k]) for k in range(K))
    top = np.abs(got[:K]).max()
    (u, Hu), (w, Hw) = (v[0], got[0]), (v[1], got[1])
    asym = abs(float((u * Hw).sum()) - float((w * Hu).sum())) / (np.abs(u).sum() * top)
    trans = np.abs(got[K]).max() / top
    print(f"\n{name}: |<u, Hv> - <v, Hu>| / (|u|_1 max|Hv|) = {asym:.2e}, max |H t| / max |H v| = {trans:.2e}, bound {bound:.1e}")
    assert asym < bound and trans < bound, (asym, trans, bound)


def _molecule():
    rng = np.random.default_rng(9)
    pos = (rng.normal(size=(6, 3)) * 0.8).astype(np.float32)
    return pos, np.zeros(6, np.int64), rng.standard_normal((6, 4)).astype(np.float32)


def test_dense_hessian_of_one_molecule():
    pos, batch, x = _molecule()
    xd, pd, bd = (torch.as_tensor(t).to(DEV) for t in (x, pos, batch))
    torch.manual_seed(7)
    model = BatchedEnergyModel(IN, 16, LAYERS, lmax=2).to(DEV).requires_grad_(False).eval()
    with _quiet():
        Hd = model.hessian(xd, pd, bd, R_MOL)
        unit = torch.eye(18, device=DEV).view(18, 6, 3)
        cols = model.hessian_vector_product(xd, pd, bd, R_MOL, unit)           # cols[(j, b), i, a] = H[i, a, j, b]
        one = model.hessian_vector_product(xd, pd, bd, R_MOL, unit[4])         # v [N,3] -> [N,3]
        g, mol = batched_radius_graph(pd, bd, R_MOL)
    assert Hd.shape == (6, 3, 6, 3) and cols.shape == (18, 6, 3) and one.shape == (6, 3) and not Hd.requires_grad
    perm = g.perm.long().cpu().numpy()
    inv = np.empty_like(perm)
    inv[perm] = np.arange(6)
    args = (_params(model), 16, LAYERS, 2, IN, x[perm].astype(np.float64), pos[perm].astype(np.float64),
            g.rowptr.cpu().numpy(), g.src.cpu().numpy())
    eye = np.eye(18).reshape(18, 6, 3)
    want = HR.Reference(*args, dtype=torch.float64).hvp(eye[:, perm])[:, inv]
    f32 = HR.Reference(*args, dtype=torch.float32).hvp(eye[:, perm])[:, inv]
    bound = _bound(f32, want)
    H = Hd.double().cpu().numpy().reshape(18, 18)
    W = want.reshape(18, 18).T                                               # W[(i, a), (j, b)]
    top = np.abs(W).max()
    errs = {"vs fp64": np.abs(H - W).max() / top, "asymmetry": np.abs(H - H.T).max() / top,
            "vs stacked H v": np.abs(H - cols.double().cpu().numpy().reshape(18, 18).T).max() / top,
            "v [N,3]": np.abs(one.double().cpu().numpy().reshape(18) - W[:, 4]).max() / top}
    print(f"\n6 atoms ({g.num_edges} edges), max |H| = {top:.3e}: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items())
          + f"; bound {bound:.1e}")
    assert g.num_edges >= 20 and top > 0
    assert max(errs.values()) < bound, (errs, bound)
    assert all(p.grad is None for p in model.parameters())


def test_refusals_and_shapes():
    pos, batch, x = _molecule()
    xd, pd, bd = (torch.as_tensor(t).to(DEV) for t in (x, pos, batch))
    bm = BatchedEnergyModel(IN, 16, 1, lmax=1).to(DEV)
    pm = PeriodicEnergyModel(IN, 16, 1, lmax=1, envelope=P_ENV).to(DEV)
    v = torch.randn(6, 3, device=DEV)
    with pytest.raises(NotImplementedError, match="bf16"):
        bm.hessian_vector_product(xd.bfloat16(), pd, bd, R_MOL, v)
    with pytest.raises(NotImplementedError, match="bf16"):
        pm.hessian_vector_product(xd.bfloat16(), pd, R_MOL, [-9, -9, -9], [9, 9, 9], v=v)
    for bad in (torch.randn(5, 3, device=DEV), torch.randn(6, 2, device=DEV), torch.randn(2, 2, 6, 3, device=DEV)):
        with pytest.raises(ValueError, match="v must be"):
            bm.hessian_vector_product(xd, pd, bd, R_MOL, bad)
    with pytest.raises(ValueError, match="needs v="):
        pm.hessian_vector_product(xd, pd, R_MOL, [-9, -9, -9], [9, 9, 9])
    n = HESSIAN_MAX_ATOMS + 1
    with pytest.raises(ValueError, match="HESSIAN_MAX_ATOMS"):
        bm.hessian(torch.zeros(n, 4, device=DEV), torch.zeros(n, 3, device=DEV), torch.zeros(n, dtype=torch.long, device=DEV), R_MOL)
    assert HESSIAN_MAX_ATOMS == 256 and not hasattr(ShardedEnergyModel, "hessian_vector_product")
    with _quiet():
        assert bm.hessian_vector_product(xd, pd, bd, R_MOL, torch.zeros(0, 6, 3, device=DEV)).shape == (0, 6, 3)


def test_forward_after_the_call_is_unchanged():
    """The dimer gas of tests/test_force_loss_gpu.py (l_max = 1, one neighbour per atom): no float sum has more than two
    addends, so two plain calls are bit-equal -- and stay so around a Hessian-vector product, which also leaves every .grad
    alone and the parameter gradients of a following energy backward unchanged."""
    R, LO, HI = 0.2, [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
    pos, x = _dimer_gas(61)
    xd, pd = torch.as_tensor(x).to(DEV), torch.as_tensor(pos).to(DEV)
    torch.manual_seed(62)
    model = PeriodicEnergyModel(IN, 16, LAYERS, lmax=1).to(DEV).train()

    def run():
        model.zero_grad()
        with _quiet():
            e, f = model(xd, pd, R, LO, HI, forces=True)
        e.backward()
        return e.detach().clone(), f.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters()}

    e0, f0, g0 = run()
    model.zero_grad()
    with _quiet():
        hv = model.hessian_vector_product(xd, pd, R, LO, HI, v=torch.randn(2, 16, 3, device=DEV))
    assert float(hv.abs().max()) > 0 and all(p.grad is None for p in model.parameters())
    e1, f1, g1 = run()
    assert torch.equal(e0, e1) and torch.equal(f0, f1) and float(f0.abs().max()) > 0
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n

"""``PeriodicEnergyModel.strain_hessian_vector_product`` / ``elastic_tensor`` against fp64 torch autograd of the strained
restatement (tests/strain_hessian_reference.py over tests/force_loss_reference.py), at the periodic shapes of
tests/test_hessian_gpu.py: 60 particles, r = 0.3, envelope 6, H = 16, 2 layers; box and cell at l_max 2, box with a Verlet list
at l_max 1.

Norm: max |got - want| / max |want| per tensor (per vector for the K = 3 products).  Bound: max(2e-5, 20 x yardstick), the
yardstick being the SAME restatement run in fp32 on the CPU against fp64 for that tensor, computed by every case itself (the
project's bound for derivatives of fp32 kernels and the margin it keeps, tests/test_hessian_gpu.py).  The symmetries are held to
the same bound: B[ab,cd] against B[cd,ab] relative to max |B|; and with delta the error of a product,
|<v, Lambda Xi> - <Lambda^T v, Xi>| <= |v|_1 max |delta(Lambda Xi)| + |Xi|_1 max |delta(Lambda^T v)|, so the difference is divided
by |v|_1 max |Lambda Xi| + |Xi|_1 max |Lambda^T v|.  A uniform translation with Xi = 0 has t = v_src - v_dst = 0 on every edge:
both outputs are exactly zero.

Measured on one MI355X (error / fp32 yardstick, ranges over the K = 3 vectors and the three cotangent choices): box h_pos
1.7e-7 .. 1.2e-6 / 2.9e-7 .. 7.4e-7, h_strain 2.1e-7 .. 8.0e-7 / 2.7e-7 .. 1.2e-6; cell h_pos 2.4e-7 .. 1.1e-6 / 2.9e-7 .. 6.2e-7,
h_strain 1.3e-7 .. 1.1e-6 / 4.2e-7 .. 1.3e-6; box with a Verlet list h_pos 4.9e-7 .. 1.3e-6 / 3.0e-7 .. 1.3e-6, h_strain
2.3e-7 .. 3.0e-6 / 3.9e-7 .. 3.3e-6; born 2.3e-7 .. 1.9e-6 / 3.6e-7 .. 1.0e-6, coupling 5.1e-7 .. 6.9e-7 / 3.5e-7 .. 4.6e-7;
strain_v=None against hessian_vector_product 6e-8 .. 2.3e-7; asymmetry of B 7.6e-8 .. 1.1e-7, of Lambda 8e-10 .. 6.5e-9; the
translation exactly 0 ("Strain second derivatives").  Without the feature every test here fails: the model has no
``strain_hessian_vector_product`` and no ``elastic_tensor``."""
import functools

import numpy as np
import pytest
import torch

import models  # noqa: F401
import strain_hessian_reference as SR
import triclinic_reference as TR
from scalable_e3_gnn_amd.batched import PeriodicEnergyModel, voigt
from scalable_e3_gnn_amd.neighbor_list import NeighborList
from scalable_e3_gnn_amd.radius_graph import radius_graph
from test_force_loss_gpu import _quiet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IN = "1x0e+1x1o"
LAYERS, H, SIZE, K = 2, 16, 60, 3
CASES = {   # name -> (kind, l_max, frozen in eval())
    "box": ("box", 2, False),
    "cell": ("cell", 2, True),
    "box-neighbors": ("neighbors", 1, False),
}
R_BOX, P_ENV, SKIN = 0.3, 6, 0.05
TRANSLATION = (0.3, -1.0, 0.7)
LO, HI = [0, 0, 0], [1, 1, 1]


def _params(model):
    return {k[len("net."):]: v.detach().cpu().numpy() for k, v in model.state_dict().items()}


@functools.lru_cache(maxsize=None)
def _run(name):
    """One case: every call of the model, the fp64 reference and the fp32 restatement of each, once"""
    kind, lmax, frozen = CASES[name]
    seed = sorted(CASES).index(name)
    rng = np.random.default_rng(500 + seed)
    torch.manual_seed(600 + seed)
    T = TR.T
    frac = rng.integers(0, 1 << 16, size=(SIZE, 3)) / float(1 << 16)
    pos = ((frac + rng.integers(-1, 2, size=frac.shape)) @ (T if kind == "cell" else np.eye(3))).astype(np.float32)
    model = PeriodicEnergyModel(IN, H, LAYERS, lmax=lmax, envelope=P_ENV).to(DEV)
    if frozen:
        model.requires_grad_(False).eval()
    else:
        model.train()
    x = rng.standard_normal((SIZE, 4)).astype(np.float32)
    v = rng.standard_normal((K, SIZE, 3)).astype(np.float32)
    xi = rng.standard_normal((K, 3, 3)).astype(np.float32)                      # non-symmetric
    shift = np.broadcast_to(np.asarray(TRANSLATION, np.float32), (SIZE, 3)).copy()
    xd, pd, vd, xid = (torch.as_tensor(t).to(DEV) for t in (x, pos, v, xi))
    ref_kw = {"envelope": (float(np.float32(R_BOX)), P_ENV)}
    if kind == "box":
        graph_kw = dict(lo=LO, hi=HI)
        g = radius_graph(pd, R_BOX, LO, HI, periodic=True)
    elif kind == "cell":
        graph_kw = dict(cell=T.tolist())
        g = radius_graph(pd, R_BOX, cell=T.tolist())
    else:
        graph_kw = dict(neighbors=NeighborList(R_BOX, SKIN, LO, HI, periodic=True))
        g = graph_kw["neighbors"].update(pd)                                     # nothing moves: the graph of every call
    if kind == "cell":
        ref_kw["cell"], V = T, abs(float(np.linalg.det(T)))
    else:
        ref_kw["L"], V = g.box, 1.0
    got = {}
    with _quiet():
        got["both"] = model.strain_hessian_vector_product(xd, pd, R_BOX, v=vd, strain_v=xid, **graph_kw)
        got["v"] = model.strain_hessian_vector_product(xd, pd, R_BOX, v=vd, **graph_kw)
        got["xi"] = model.strain_hessian_vector_product(xd, pd, R_BOX, strain_v=xid, **graph_kw)
        got["one"] = model.strain_hessian_vector_product(xd, pd, R_BOX, v=vd[0], strain_v=xid[0], **graph_kw)
        got["shift"] = model.strain_hessian_vector_product(xd, pd, R_BOX, v=torch.as_tensor(shift).to(DEV), **graph_kw)
        got["elastic"] = model.elastic_tensor(xd, pd, R_BOX, **graph_kw)
        got["hvp"] = (model.hessian_vector_product(xd, pd, R_BOX, v=vd, **graph_kw),)
    for pair in got.values():
        assert all(not t.requires_grad and t.dtype == torch.float32 for t in pair)
    has_grad = [n for n, p in model.named_parameters() if p.grad is not None]
    got = {k: tuple(t.double().cpu().numpy() for t in pair) for k, pair in got.items()}
    perm = g.perm.long().cpu().numpy()
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    args = (_params(model), H, LAYERS, lmax, IN, x[perm].astype(np.float64), pos[perm].astype(np.float64),
            g.rowptr.cpu().numpy(), g.src.cpu().numpy())
    want, f32 = {}, {}
    for out, dtype in ((want, torch.float64), (f32, torch.float32)):
        ref = SR.Reference(*args, dtype=dtype, **ref_kw)
        v64, xi64 = v[:, perm].astype(np.float64), xi.astype(np.float64)
        for key, kw in (("both", dict(v=v64, xi=xi64)), ("v", dict(v=v64)), ("xi", dict(xi=xi64))):
            hp, hs = ref.hvp(**kw)
            out[key] = (hp[:, inv], hs)
        born, coupling = ref.elastic(V)
        out["elastic"] = (born, coupling[inv])
    return got, want, f32, (v.astype(np.float64), xi.astype(np.float64)), has_grad, g.num_edges, model.training


def _bound(f32, want):
    return max(2e-5, 20 * SR.rel_max(f32, want))


@pytest.mark.parametrize("name", list(CASES))
def test_strain_hessian_vector_products_vs_fp64(name):
    got, want, f32, _, has_grad, E, _ = _run(name)
    assert not has_grad, has_grad
    assert got["both"][0].shape == (K, SIZE, 3) and got["both"][1].shape == (K, 3, 3)
    assert got["one"][0].shape == (SIZE, 3) and got["one"][1].shape == (3, 3)
    worst = 0.0
    for key in ("both", "v", "xi"):
        for t, label in enumerate(("h_pos", "h_strain")):
            for k in range(K):
                g_, w_, f_ = got[key][t][k], want[key][t][k], f32[key][t][k]
                err, yard, bound = SR.rel_max(g_, w_), SR.rel_max(f_, w_), _bound(f_, w_)
                print(f"\n{name} ({E} edges), cotangents {key}, {label} {k}: max |.| = {np.abs(w_).max():.3e}, err {err:.2e}, "
                      f"fp32 yardstick {yard:.2e}, bound {bound:.1e}")
                assert np.abs(w_).max() > 0
                worst = max(worst, err / bound)
    # v [N,3] with strain_v [3,3]: the first pair of the K = 3 call, to the same bound
    for t in range(2):
        assert SR.rel_max(got["one"][t], want["both"][t][0]) < _bound(f32["both"][t][0], want["both"][t][0])
    assert worst < 1.0, worst


@pytest.mark.parametrize("name", list(CASES))
def test_strain_v_none_is_the_hessian_vector_product(name):
    got, want, f32, _, _, _, _ = _run(name)
    for k in range(K):
        err, bound = SR.rel_max(got["v"][0][k], got["hvp"][0][k]), _bound(f32["v"][0][k], want["v"][0][k])
        print(f"\n{name}, v{k}: h_pos of strain_hessian_vector_product(strain_v=None) vs hessian_vector_product {err:.2e}, "
              f"bound {bound:.1e}")
        assert err < bound, (k, err, bound)


@pytest.mark.parametrize("name", list(CASES))
def test_elastic_tensor_vs_fp64(name):
    got, want, f32, _, _, E, _ = _run(name)
    born, coupling = got["elastic"]
    assert born.shape == (3, 3, 3, 3) and coupling.shape == (SIZE, 3, 3, 3)
    ok = True
    for t, label in enumerate(("born", "coupling")):
        err, yard = SR.rel_max(got["elastic"][t], want["elastic"][t]), SR.rel_max(f32["elastic"][t], want["elastic"][t])
        bound = _bound(f32["elastic"][t], want["elastic"][t])
        print(f"\n{name} ({E} edges), {label}: max |.| = {np.abs(want['elastic'][t]).max():.3e}, err {err:.2e}, fp32 yardstick "
              f"{yard:.2e}, bound {bound:.1e}")
        ok = ok and np.abs(want["elastic"][t]).max() > 0 and err < bound
    assert ok
    # the Voigt contraction: the helper against the same contraction of the reference
    basis = np.zeros((6, 3, 3))
    for i, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))):
        basis[i, a, b] += 0.5
        basis[i, b, a] += 0.5
    c_want = np.einsum("iab,abcd,jcd->ij", basis, want["elastic"][0], basis)
    c_got = voigt(torch.as_tensor(born)).numpy()
    assert c_got.shape == (6, 6) and SR.rel_max(c_got, c_want) < _bound(f32["elastic"][0], want["elastic"][0])


@pytest.mark.parametrize("name", list(CASES))
def test_symmetry_and_translation(name):
    got, want, f32, (v, xi), _, _, _ = _run(name)
    born = got["elastic"][0]
    sym_b = np.abs(born - born.transpose(2, 3, 0, 1)).max() / np.abs(born).max()
    bound_b = _bound(f32["elastic"][0], want["elastic"][0])
    lam_xi, lamt_v = got["xi"][0][0], got["v"][1][0]                            # Lambda Xi_0 [N,3], Lambda^T v_0 [3,3]
    a, b = float((v[0] * lam_xi).sum()), float((lamt_v * xi[0]).sum())
    sym_l = abs(a - b) / (np.abs(v[0]).sum() * np.abs(lam_xi).max() + np.abs(xi[0]).sum() * np.abs(lamt_v).max())
    bound_l = max(_bound(f32["xi"][0][0], want["xi"][0][0]), _bound(f32["v"][1][0], want["v"][1][0]))
    print(f"\n{name}: |B[ab,cd] - B[cd,ab]| / max |B| = {sym_b:.2e} (bound {bound_b:.1e}); |<v, L Xi> - <L^T v, Xi>| / (|v|_1 max "
          f"|L Xi| + |Xi|_1 max |L^T v|) = {sym_l:.2e} (bound {bound_l:.1e})")
    assert sym_b < bound_b and sym_l < bound_l, (sym_b, sym_l)
    assert not got["shift"][0].any() and not got["shift"][1].any()              # a uniform translation: exactly zero


@pytest.mark.parametrize("name", list(CASES))
def test_no_leftovers(name):
    _, _, _, _, has_grad, _, training = _run(name)
    assert not has_grad and training == (not CASES[name][2])                     # "cell" ran frozen, in eval()


def test_refusals():
    rng = np.random.default_rng(9)
    pos = torch.as_tensor(rng.random((SIZE, 3)).astype(np.float32)).to(DEV)
    x = torch.as_tensor(rng.standard_normal((SIZE, 4)).astype(np.float32)).to(DEV)
    pm = PeriodicEnergyModel(IN, H, 1, lmax=1, envelope=P_ENV).to(DEV)
    v, xi = torch.randn(2, SIZE, 3, device=DEV), torch.randn(3, 3, 3, device=DEV)
    with pytest.raises(NotImplementedError, match="bf16"):
        pm.strain_hessian_vector_product(x.bfloat16(), pos, R_BOX, LO, HI, v=v[0])
    with pytest.raises(NotImplementedError, match="bf16"):
        pm.elastic_tensor(x.bfloat16(), pos, R_BOX, LO, HI)
    with pytest.raises(ValueError, match="needs v="):
        pm.strain_hessian_vector_product(x, pos, R_BOX, LO, HI)
    with pytest.raises(ValueError, match="same number K"):
        pm.strain_hessian_vector_product(x, pos, R_BOX, LO, HI, v=v, strain_v=xi)
    with pytest.raises(ValueError, match="same number K"):
        pm.strain_hessian_vector_product(x, pos, R_BOX, LO, HI, v=v[0], strain_v=xi[:1])
    with pytest.raises(ValueError, match="strain_v must be"):
        pm.strain_hessian_vector_product(x, pos, R_BOX, LO, HI, strain_v=torch.randn(3, device=DEV))
    with pytest.raises(ValueError, match="all three axes"):
        pm.elastic_tensor(x, pos, R_BOX, LO, HI, periodic=(True, True, False))
    with pytest.raises(ValueError, match="\\[3,3,3,3\\]"):
        voigt(torch.zeros(3, 3))

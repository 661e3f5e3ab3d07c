"""The yardstick of the strain-Hessian tests checked on its own (no GPU): ``strain_hessian_reference.Reference.hvp`` -- autograd
through the first derivatives (dE/dpos, dE/deps) of the strained restatement -- against central differences of those first
derivatives, in eps and in pos, and the symmetries of the joint Hessian.  So the reference cannot be wrong along with the
kernels it judges.

40 nodes, H = 16, 2 layers, fp64, the periodic cases of tests/test_hessian_reference_host.py: the periodic unit box at r = 0.3
with the envelope (l_max 2), the same without it (l_max 1), the triclinic cell of tests/triclinic_reference.py with the envelope,
and the enveloped box once more at a finite, non-symmetric strain (|eps| = 0.05): the reference accepts a finite eps and the
Hessian there has the (I + eps) factors the kernels have.

Central differences with |v|_max = |Xi|_max = 1 at h = 1e-5 and h = 3e-6:
  (g(eps + h Xi) - g(eps - h Xi)) / 2h = (Lambda Xi, B Xi),   (g(pos + h v) - g(pos - h v)) / 2h = (H v, Lambda^T v),
g = (dE/dpos, dE/deps).  Truncation h^2 / 6 times the third derivative, ~ (1 / d_min)^2 ~ 1e3 relative at the closest pairs of
such a cloud (d_min ~ 0.03): ~ 2e-8 and 2e-9 in pos, less in eps (a strain step h moves an edge by h |r| <= 0.3 h); rounding
~ 1e-16 / h times the cancellation of the sums.  Bound 1e-6 for both quotients against autograd and against each other, per
tensor, in the norm max |a - b| / max |b|.  The symmetries B[ab,cd] = B[cd,ab] and <v, Lambda Xi> = <Lambda^T v, Xi> are exact
identities of the graph in fp64 up to the rounding of the sums: bound 1e-10."""
import functools

import numpy as np
import pytest
import torch

import models  # noqa: F401
import strain_hessian_reference as SR
import triclinic_reference as TR
from scalable_e3_gnn_amd.segnn import SEGNN

N, H, LAYERS, R = 40, 16, 2, 0.3
IN = "1x0e+1x1o"
EPS = np.array([[0.05, -0.03125, 0.015625], [0.0234375, -0.046875, 0.0390625], [-0.0078125, 0.02734375, 0.03515625]])
CASES = {"l2-box-envelope": (2, "box", True, None), "l1-box": (1, "box", False, None),
         "l2-cell-envelope": (2, "cell", True, None), "l2-box-envelope-strained": (2, "box", True, EPS)}
STEPS = (1e-5, 3e-6)


def _graph(pos, cell):
    """radius graph of the periodic cell (rows = lattice vectors; minimum image), dst-sorted, src ascending"""
    n = len(pos)
    rel = TR.min_image64_cell((pos[None, :, :] - pos[:, None, :]).reshape(-1, 3), cell).reshape(n, n, 3)   # [dst, src]
    adj = ((rel ** 2).sum(-1) < R * R) & ~np.eye(n, dtype=bool)
    dst, src = np.nonzero(adj)
    return np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n))]).astype(np.int64), src.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _case(name):
    lmax, mode, env, eps = CASES[name]
    rng = np.random.default_rng(140 + sorted(CASES).index(name))
    cell = TR.T if mode == "cell" else np.eye(3)
    pos = rng.random((N, 3)) @ cell
    x = rng.standard_normal((N, 4))
    rowptr, src = _graph(pos, cell)
    kw = {"cell": cell} if mode == "cell" else {"L": (1.0, 1.0, 1.0)}
    if env:
        kw["envelope"] = (R, 6)
    torch.manual_seed(150 + lmax)
    net = SEGNN(IN, H, "1x0e", LAYERS, lmax=lmax, **({"envelope": 6} if env else {}))   # host only: parameters, no forward
    params = {k: v.detach().double().numpy() for k, v in net.state_dict().items()}
    args = lambda p: (params, H, LAYERS, lmax, IN, x, p, rowptr, src)
    e0 = np.zeros((3, 3)) if eps is None else eps
    ref = SR.Reference(*args(pos), eps=e0, **kw)
    v, xi = rng.uniform(-1, 1, (N, 3)), rng.uniform(-1, 1, (3, 3))
    return args, kw, pos, e0, len(src), (v, xi), ref


def _check(name, what, quot, want):
    """quot {h: (d g_pos, d g_eps)} against want = (h_pos, h_strain)"""
    for t, label in enumerate(("pos", "strain")):
        errs = {h: SR.rel_max(q[t], want[t]) for h, q in quot.items()}
        both = SR.rel_max(quot[STEPS[0]][t], quot[STEPS[1]][t])
        print(f"\n{name}, difference in {what}, h_{label}: max |.| = {np.abs(want[t]).max():.3e}; central difference vs autograd "
              + ", ".join(f"h = {h:g}: {e:.1e}" for h, e in errs.items()) + f"; the two quotients {both:.1e}")
        assert np.abs(want[t]).max() > 0
        assert max(errs.values()) <= 1e-6 and both <= 1e-6, (name, what, label, errs, both)


@pytest.mark.parametrize("name", list(CASES))
def test_autograd_vs_central_difference_in_the_strain(name):
    args, kw, pos, e0, E, (v, xi), ref = _case(name)
    assert 150 <= E <= 500, E
    quot = {}
    for h in STEPS:
        (ap, ae), (bp, be) = SR.first64(*args(pos), eps=e0 + h * xi, **kw), SR.first64(*args(pos), eps=e0 - h * xi, **kw)
        quot[h] = ((ap - bp) / (2 * h), (ae - be) / (2 * h))
    _check(name, "eps", quot, ref.hvp(xi=xi))


@pytest.mark.parametrize("name", list(CASES))
def test_autograd_vs_central_difference_in_the_positions(name):
    args, kw, pos, e0, E, (v, xi), ref = _case(name)
    quot = {}
    for h in STEPS:
        (ap, ae), (bp, be) = SR.first64(*args(pos + h * v), eps=e0, **kw), SR.first64(*args(pos - h * v), eps=e0, **kw)
        quot[h] = ((ap - bp) / (2 * h), (ae - be) / (2 * h))
    _check(name, "pos", quot, ref.hvp(v=v))


@pytest.mark.parametrize("name", list(CASES))
def test_symmetries(name):
    _, _, _, _, _, (v, xi), ref = _case(name)
    born, coupling = ref.elastic(1.0)
    sym_b = np.abs(born - born.transpose(2, 3, 0, 1)).max() / np.abs(born).max()
    lam_xi, _ = ref.hvp(xi=xi)
    _, lamt_v = ref.hvp(v=v)
    a, b = float((v * lam_xi).sum()), float((lamt_v * xi).sum())
    sym_l = abs(a - b) / (np.abs(v).sum() * np.abs(lam_xi).max())                   # |<v, .>| <= |v|_1 max |.|
    both = SR.rel_max(np.einsum("ikab,ab->ik", coupling, xi), lam_xi)                # elastic() is hvp on the unit Xi
    print(f"\n{name}: max |B| = {np.abs(born).max():.3e}, |B[ab,cd] - B[cd,ab]| / max |B| = {sym_b:.1e}; "
          f"|<v, L Xi> - <L^T v, Xi>| / (|v|_1 max |L Xi|) = {sym_l:.1e}; coupling . Xi vs hvp(Xi) {both:.1e}")
    assert sym_b <= 1e-10 and sym_l <= 1e-10 and both <= 1e-10, (sym_b, sym_l, both)


def test_zero_strain_is_the_unstrained_reference():
    """at eps = 0 the first derivative in pos and H v are those of tests/hessian_reference.py: the strain is inserted, nothing
    else changed"""
    import hessian_reference as HR
    args, kw, pos, _, _, (v, xi), ref = _case("l2-cell-envelope")
    plain = HR.Reference(*args(pos), **kw)
    assert SR.rel_max(-ref.first()[0], plain.forces()) <= 1e-14
    assert SR.rel_max(ref.hvp(v=v)[0], plain.hvp(v)) <= 1e-12


def test_fp32_reference_is_the_same_code():
    """the fp32 run (the yardstick of the GPU tests) agrees with fp64 to fp32 rounding: it is the same expression"""
    args, kw, pos, e0, _, (v, xi), ref = _case("l2-box-envelope")
    got = SR.Reference(*args(pos), eps=e0, dtype=torch.float32, **kw).hvp(v=v, xi=xi)
    want = ref.hvp(v=v, xi=xi)
    errs = [SR.rel_max(g, w) for g, w in zip(got, want)]
    print(f"\nfp32 restatement vs fp64: h_pos {errs[0]:.1e}, h_strain {errs[1]:.1e}")
    assert all(0 < e <= 1e-3 for e in errs), errs

"""The yardstick of the Hessian tests checked on its own (no GPU): ``hessian_reference.Reference.hvp`` -- autograd through the
forces of ``force_loss_reference.energy_forces`` -- against a central difference of those forces on the fixed edge set, the
symmetry <u, H v> = <v, H u>, and H (uniform translation) = 0.  So the reference cannot be wrong along with the kernels it
judges.

40 nodes in the unit cube at r = 0.45 (an enveloped case in the periodic unit box at r = 0.3 beside the plain ones), H = 16,
2 layers, fp64.  Central difference (F(x + h v) - F(x - h v)) / 2h = -H v with |v|_max = 1 at h = 1e-5 and h = 3e-6: the
truncation is h^2 / 6 times the third derivative of F, which for the harmonics' 1 / d^k terms is ~ (1 / d_min)^2 ~ 1e3 relative
to H v at the closest pairs of such a cloud (d_min ~ 0.03): ~ 2e-8 and 2e-9; the rounding is ~ 1e-16 / h ~ 1e-11 .. 3e-11 times
the cancellation of the force sums.  Bound 1e-6 for both quotients against autograd and against each other; symmetry and
translation are exact identities of the graph in fp64 up to the rounding of sums over ~300 edges through 2 layers: bound 1e-10
relative to max |H v|.  Measured: 5.6e-8 .. 1.2e-7 at h = 1e-5 and 5.0e-9 .. 1.1e-8 at h = 3e-6 (the h^2 law), symmetry below
2e-17, translation exactly 0 (the tangent v_src - v_dst of a uniform field is 0)."""
import functools

import numpy as np
import pytest
import torch

import models  # noqa: F401
import force_loss_reference as FR
import hessian_reference as HR
import pbc_reference as P
from scalable_e3_gnn_amd.segnn import SEGNN

N, H, LAYERS = 40, 16, 2
IN = "1x0e+1x1o"
CASES = {"l1": (1, False), "l2": (2, False), "l2-envelope-box": (2, True)}


def _periodic_graph(pos, r):
    """radius graph of the periodic unit box (minimum image), dst-sorted, src ascending"""
    n = len(pos)
    rel = P.min_image64((pos[None, :, :] - pos[:, None, :]).reshape(-1, 3), (1.0, 1.0, 1.0)).reshape(n, n, 3)   # [dst, src]
    adj = ((rel ** 2).sum(-1) < r * r) & ~np.eye(n, dtype=bool)
    dst, src = np.nonzero(adj)
    return np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=len(pos)))]).astype(np.int64), src.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _case(name):
    lmax, env = CASES[name]
    rng = np.random.default_rng(40 + sorted(CASES).index(name))
    pos = rng.random((N, 3))
    x = rng.standard_normal((N, 4))
    kw = {}
    if env:
        rowptr, src = _periodic_graph(pos, 0.3)
        kw = {"L": (1.0, 1.0, 1.0), "envelope": (0.3, 6)}
    else:
        rowptr, src = FR.brute_graph(pos, 0.45)
    torch.manual_seed(50 + lmax)
    net = SEGNN(IN, H, "1x0e", LAYERS, lmax=lmax, **({"envelope": 6} if env else {}))   # host only: parameters, no forward
    params = {k: v.detach().double().numpy() for k, v in net.state_dict().items()}
    args = lambda p: (params, H, LAYERS, lmax, IN, x, p, rowptr, src)
    ref = HR.Reference(*args(pos), **kw)
    u, v = rng.uniform(-1, 1, (2, N, 3))
    Hu, Hv = ref.hvp(np.stack([u, v]))
    return args, kw, pos, len(src), (u, v, Hu, Hv), ref


@pytest.mark.parametrize("name", list(CASES))
def test_autograd_hvp_vs_central_difference_of_the_forces(name):
    args, kw, pos, E, (u, v, Hu, Hv), _ = _case(name)
    assert 150 <= E <= 500, E
    quot = {h: -(HR.forces64(*args(pos + h * v), **kw) - HR.forces64(*args(pos - h * v), **kw)) / (2 * h)
            for h in (1e-5, 3e-6)}
    errs = {h: HR.rel_max(q, Hv) for h, q in quot.items()}
    both = HR.rel_max(quot[1e-5], quot[3e-6])
    print(f"\n{name}: E = {E} edges, max |H v| = {np.abs(Hv).max():.3e}; central difference vs autograd "
          + ", ".join(f"h = {h:g}: {e:.1e}" for h, e in errs.items()) + f"; the two quotients {both:.1e}")
    assert np.abs(Hv).max() > 0
    assert max(errs.values()) <= 1e-6 and both <= 1e-6, (errs, both)


@pytest.mark.parametrize("name", list(CASES))
def test_symmetry_and_translation(name):
    _, _, _, _, (u, v, Hu, Hv), ref = _case(name)
    top = max(np.abs(Hu).max(), np.abs(Hv).max())
    asym = abs(float((u * Hv).sum()) - float((v * Hu).sum())) / (top * np.abs(u).sum())   # |<u, .>| <= |u|_1 max|.|
    shift = np.broadcast_to(np.array([0.3, -1.0, 0.7]), (N, 3))
    trans = np.abs(ref.hvp(shift)).max() / top
    print(f"\n{name}: |<u, Hv> - <v, Hu>| / (|u|_1 max|Hv|) = {asym:.1e}, max |H translation| / max |H v| = {trans:.1e}")
    assert asym <= 1e-10 and trans <= 1e-10, (asym, trans)


def test_fp32_reference_is_the_same_code():
    """the fp32 run (the yardstick of the GPU tests) agrees with fp64 to fp32 rounding: it is the same expression"""
    args, kw, pos, _, (u, v, Hu, Hv), _ = _case("l2")
    got = HR.Reference(*args(pos), dtype=torch.float32, **kw).hvp(v)
    err = HR.rel_max(got, Hv)
    print(f"\nfp32 restatement vs fp64: {err:.1e}")
    assert 0 < err <= 1e-3, err

"""Second derivatives of the torch restatement of the energy models in the joint coordinates (pos, eps): the yardstick of the
strain-Hessian tests (tests/test_strain_hessian_reference_host.py, tests/test_elastic_gpu.py).  TEST INFRASTRUCTURE ONLY.

The energy is the one of ``force_loss_reference.energy_forces`` (open box, box, cell, envelope); that file stays as it is.  The
one change is a leaf strain ``eps`` [3,3] applied to every edge vector of the undeformed graph as in tests/virial_reference.py,
r' = r + eps r with r the minimum image of x_src - x_dst: ``energy_forces`` hands its edge vectors to
``oracle.segnn_oracle.sh_component_torch`` and to nothing else, so for the length of the call that one function is replaced by
itself composed with r -> (I + eps) r.  Y, d, the envelope and A are then those of r'; the set of d = 0 edges is that of r
(I + eps is regular).  ``eps`` may be finite.  The position leaf is recovered as in tests/hessian_reference.py.

With g_pos = dE/dpos and G = dE/deps (both with a graph), the Hessian applied to cotangents (v, Xi) is the gradient of
<v, g_pos> + <Xi, G> in (pos, eps):  h_pos = H v + Lambda Xi,  h_strain = Lambda^T v + B Xi.  fp64 is the reference, the same
code in fp32 the yardstick of what fp32 arithmetic costs."""
import numpy as np
import torch

import force_loss_reference as FR
from hessian_reference import position_leaf, rel_max  # noqa: F401  (rel_max: the norm of every test)
from oracle import segnn_oracle as S


class Reference:
    """One evaluation of ``force_loss_reference.energy_forces`` (same arguments) at the strain ``eps`` [3,3] (None: zero)."""

    def __init__(self, *args, eps=None, dtype=torch.float64, **kw):
        self.dtype = dtype
        e0 = np.zeros((3, 3)) if eps is None else np.asarray(eps, np.float64).reshape(3, 3)
        self.eps = torch.as_tensor(e0).to(dtype).clone().requires_grad_(True)
        M = torch.eye(3, dtype=dtype) + self.eps
        plain = S.sh_component_torch
        S.sh_component_torch = lambda lmax, rel: plain(lmax, rel @ M.T)        # r'_a = r_a + eps[a, b] r_b
        try:
            E, F, leaves = FR.energy_forces(*args, dtype=dtype, **kw)
        finally:
            S.sh_component_torch = plain
        self.E = E.sum()
        self.gpos = -F                                                          # dE/dpos, with its graph
        self.pos = position_leaf(F, leaves)
        (self.geps,) = torch.autograd.grad(self.E, [self.eps], create_graph=True)

    def first(self):
        """-> dE/dpos [N,3], dE/deps [3,3], fp64 numpy"""
        return self.gpos.detach().double().numpy(), self.geps.detach().double().numpy()

    def hvp(self, v=None, xi=None):
        """v [N,3] | [K,N,3] | None, xi [3,3] | [K,3,3] | None (arrays) -> (h_pos, h_strain) with the leading K of the input
        (none when the input has none), fp64 numpy"""
        single = (v if v is not None else xi).ndim == 2
        vs = np.asarray(v, np.float64).reshape(-1, *self.gpos.shape) if v is not None else None
        xs = np.asarray(xi, np.float64).reshape(-1, 3, 3) if xi is not None else None
        K = len(vs) if vs is not None else len(xs)
        hp, hs = [], []
        for k in range(K):
            outs, cots = [], []
            if vs is not None:
                outs.append(self.gpos)
                cots.append(torch.as_tensor(vs[k]).to(self.dtype))
            if xs is not None:
                outs.append(self.geps)
                cots.append(torch.as_tensor(xs[k]).to(self.dtype))
            a, b = torch.autograd.grad(outs, [self.pos, self.eps], cots, retain_graph=True)
            hp.append(a.double().numpy())
            hs.append(b.double().numpy())
        hp, hs = np.stack(hp), np.stack(hs)
        return (hp[0], hs[0]) if single else (hp, hs)

    def elastic(self, V):
        """-> born [3,3,3,3] = (1/V) d2E/deps_ab deps_cd, coupling [N,3,3,3] = d2E/dpos_ik deps_ab, fp64 numpy"""
        hp, hs = self.hvp(xi=np.eye(9).reshape(9, 3, 3))                        # hp[(a,b), i, k], hs[(c,d), a, b]
        N = hp.shape[1]
        return hs.reshape(3, 3, 3, 3).transpose(2, 3, 0, 1) / V, hp.reshape(3, 3, N, 3).transpose(2, 3, 0, 1)


def first64(*args, **kw):
    """fp64 (dE/dpos, dE/deps) alone (for a difference quotient), numpy"""
    return Reference(*args, dtype=torch.float64, **kw).first()

"""Hessian-vector products of the torch restatement of the energy models: the yardstick of the Hessian tests
(tests/test_hessian_reference_host.py, tests/test_hessian_gpu.py).  TEST INFRASTRUCTURE ONLY.

``force_loss_reference.energy_forces`` returns the forces F = -dE/dpos WITH their graph, but not the position leaf that graph
ends in; that file stays as it is, so the leaf is recovered from the graph: it is the one leaf of shape [N,3] that is not among
the parameter leaves the function returns.  H v = d<v, dE/dpos>/dpos = the gradient of <-v, F> in that leaf (H is symmetric:
the vector-Jacobian product of dE/dpos is H v), on the FIXED edge set the function was given.  fp64 is the reference, the same
code in fp32 the yardstick of what fp32 arithmetic costs."""
import numpy as np
import torch

import force_loss_reference as FR


def position_leaf(F, leaves):
    """The leaf tensor of shape ``F.shape`` in the graph of ``F`` that is none of ``leaves`` (the parameters)."""
    known = {id(t) for t in leaves.values()}
    seen, stack, found = set(), [F.grad_fn], []
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        var = getattr(fn, "variable", None)          # AccumulateGrad: a leaf
        if var is not None and id(var) not in known and tuple(var.shape) == tuple(F.shape):
            found.append(var)
        stack.extend(f for f, _ in fn.next_functions)
    assert len(found) == 1, f"{len(found)} candidate position leaves"
    return found[0]


class Reference:
    """One evaluation of ``force_loss_reference.energy_forces`` (same arguments) that answers H v for any number of v."""

    def __init__(self, *args, dtype=torch.float64, **kw):
        self.dtype = dtype
        self.E, self.F, leaves = FR.energy_forces(*args, dtype=dtype, **kw)
        self.pos = position_leaf(self.F, leaves)

    def forces(self):
        return self.F.detach().double().numpy()

    def hvp(self, v):
        """v [N,3] or [K,N,3] (graph order, array) -> H v of the same shape, fp64 numpy"""
        v = np.array(v, np.float64)
        vs = v.reshape(-1, *self.F.shape)
        out = [torch.autograd.grad(self.F, [self.pos], -torch.as_tensor(t).to(self.dtype), retain_graph=True)[0]
               for t in vs]
        return torch.stack(out).double().numpy().reshape(v.shape)


def forces64(*args, **kw):
    """fp64 forces alone (for a difference quotient), numpy"""
    return FR.energy_forces(*args, dtype=torch.float64, **kw)[1].detach().numpy()


def rel_max(got, want):
    """max |got - want| / max |want|"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))

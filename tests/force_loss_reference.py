"""Torch restatement of the energy models that can be differentiated TWICE: the yardstick of the force-loss tests
(tests/test_force_loss_reference_host.py, tests/test_force_loss_gpu.py).  TEST INFRASTRUCTURE ONLY.

The layer sequence is the one of ``oracle.segnn_oracle.energy_forces_torch`` (plain model) and of
``envelope_reference.energy_forces_strain`` (enveloped model), built from ``oracle.tp_oracle.forward_torch_cpu`` and
``oracle.segnn_oracle.sh_component_torch``, in any dtype (fp64: the reference; fp32: the yardstick of what fp32 arithmetic
costs).  Open, box and cell graphs: the lattice shift of every edge is a constant, taken from the fp64 minimum image
(``pbc_reference.min_image64`` / ``triclinic_reference.min_image64_cell``).  The forces come from
``autograd.grad(..., create_graph=True)``, so a loss on energies and forces has parameter gradients.

Edges with d = 0 are left out of the geometric terms: their Y is [1, 0, ...] and their d is 0, constants (the library's
contract: such an edge gives no force and no tangent)."""
import numpy as np
import torch

import pbc_reference as P
import triclinic_reference as TR
from envelope_reference import envelope64
from oracle import segnn_oracle as S
from oracle import tp_oracle as T


def brute_graph(pos, r):
    """open radius graph of a small cloud -> rowptr [N + 1], src [E] (dst-sorted, src ascending, no self edge)"""
    pos = np.asarray(pos, np.float64)
    d2 = ((pos[:, None] - pos[None]) ** 2).sum(-1)
    adj = (d2 < r * r) & ~np.eye(len(pos), dtype=bool)
    dst, src = np.nonzero(adj)
    return np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=len(pos)))]).astype(np.int64), src.astype(np.int64)


def energy_forces(params, H, num_layers, lmax, in_irreps, x, pos, rowptr, src, dtype=torch.float64, L=None, cell=None,
                  envelope=None, mol=None, n_mol=1):
    """-> (E [n_mol], F [N,3] = -dE/dpos WITH a graph, {name: parameter leaf}).  ``L``: box lengths per axis (0 = open) or
    ``cell`` [3,3] (rows = lattice vectors); ``envelope`` = (r_c, p) or None; ``mol`` [N] structure of every node (None: one
    structure).  Everything in graph order."""
    hid = f"{H}x0e+{H}x1o" + (f"+{H}x2e" if lmax == 2 else "")
    gated = f"{H}x0e+{lmax * H}x0e+{H}x1o" + (f"+{H}x2e" if lmax == 2 else "")
    rowptr_t, src_t = torch.as_tensor(np.asarray(rowptr)).long(), torch.as_tensor(np.asarray(src)).long()
    N = rowptr_t.numel() - 1
    deg = rowptr_t[1:] - rowptr_t[:-1]
    dst_t = torch.repeat_interleave(torch.arange(N), deg)
    E = src_t.numel()
    ny = (lmax + 1) ** 2
    pos64 = np.asarray(pos, np.float64)
    raw = pos64[src_t.numpy()] - pos64[dst_t.numpy()]
    image = P.min_image64(raw, L) if L is not None else TR.min_image64_cell(raw, cell) if cell is not None else raw
    shift = torch.as_tensor(image - raw).to(dtype)                     # whole periods: constant
    nz = torch.as_tensor(np.nonzero(np.linalg.norm(image, axis=1) > 0)[0]).long()
    pos_t = torch.as_tensor(pos64).to(dtype).requires_grad_(True)
    Pm = {k: torch.as_tensor(np.asarray(v)).to(dtype).requires_grad_(k.split(".")[-1].startswith("weights_"))
          for k, v in params.items()}
    rel = (pos_t[src_t] - pos_t[dst_t] + shift)[nz]
    Ynz, dnz = S.sh_component_torch(lmax, rel)
    Y0 = torch.zeros(E, ny, dtype=dtype)
    Y0[:, 0] = 1.0
    Y = Y0.index_copy(0, nz, Ynz)
    d = torch.zeros(E, dtype=dtype).index_copy(0, nz, dnz)
    if envelope is None:
        w = None
        A = torch.cat([torch.ones(N, 1, dtype=dtype),
                       torch.zeros(N, ny - 1, dtype=dtype).index_add(0, dst_t, Y[:, 1:]) / deg.clamp_min(1)[:, None].to(dtype)], 1)
    else:
        w = envelope64(d, float(envelope[0]), int(envelope[1]))
        Sw = torch.zeros(N, ny, dtype=dtype).index_add(0, dst_t, w[:, None] * Y)
        A = torch.cat([torch.ones(N, 1, dtype=dtype), Sw[:, 1:] / (1.0 + Sw[:, :1])], 1)

    def tp2(prefix, in1, in2, ii, oi):
        W = {c: Pm[f"{prefix}.weights_{c}"] for c in T.CLASSES if f"{prefix}.weights_{c}" in Pm}
        Nn = {c: Pm[f"{prefix}.norm_{c}"] for c in T.CLASSES if f"{prefix}.norm_{c}" in Pm}
        for c in T.CLASSES:
            Nn.setdefault(c, torch.ones(0, dtype=dtype))
        return T.forward_torch_cpu(ii, oi, lmax, in1, in2, W, Nn)

    def g(t):
        out = [torch.nn.functional.silu(t[:, :H])]
        g0, c0 = H, H + lmax * H
        for l in range(1, lmax + 1):
            wd = 2 * l + 1
            out.append((torch.sigmoid(t[:, g0:g0 + H])[:, :, None] * t[:, c0:c0 + H * wd].reshape(-1, H, wd)).reshape(-1, H * wd))
            g0 += H
            c0 += H * wd
        return torch.cat(out, 1)

    h = tp2("embed", torch.as_tensor(np.asarray(x)).to(dtype), A, in_irreps, hid)
    for l in range(num_layers):
        pre = f"layers.{l}"
        m = torch.cat([h[dst_t], h[src_t], d[:, None]], 1)
        m = g(tp2(pre + ".msg1", m, Y, f"{hid}+{hid}+1x0e", gated))
        m = g(tp2(pre + ".msg2", m, Y, hid, gated))
        a = torch.zeros_like(h).index_add(0, dst_t, m if w is None else w[:, None] * m)
        u = g(tp2(pre + ".upd1", torch.cat([h, a], 1), A, f"{hid}+{hid}", gated))
        h = h + tp2(pre + ".upd2", u, A, hid, hid)
    e_node = tp2("readout", h, A, hid, "1x0e")[:, 0]
    seg = torch.zeros(N, dtype=torch.long) if mol is None else torch.as_tensor(np.asarray(mol)).long()
    energy = torch.zeros(n_mol, dtype=dtype).index_add(0, seg, e_node)
    (gpos,) = torch.autograd.grad(energy.sum(), [pos_t], create_graph=True)
    return energy, -gpos, {k: v for k, v in Pm.items() if v.requires_grad}


def parameter_gradients(loss, leaves, retain_graph=False):
    """{name: dL/dtheta as fp64 numpy}"""
    names = list(leaves)
    grads = torch.autograd.grad(loss, [leaves[k] for k in names], retain_graph=retain_graph)
    return {k: g_.double().numpy() for k, g_ in zip(names, grads)}


def linear_loss(c):
    """L = 0.3 sum E + sum <c, F>, c [N,3] (array or tensor) in the order of F"""
    return lambda E, F: 0.3 * E.sum() + (torch.as_tensor(c).to(F.dtype).to(F.device) * F).sum()


def matching_loss(E_star, F_star):
    """L = mean((F - F*)^2) + mean((E - E*)^2)"""
    def loss(E, F):
        Fs, Es = torch.as_tensor(F_star).to(F.dtype).to(F.device), torch.as_tensor(E_star).to(E.dtype).to(E.device)
        return ((F - Fs) ** 2).mean() + ((E - Es) ** 2).mean()
    return loss


def worst(got, want):
    """{name: max |got - want| / max |want|} -> the per-tensor errors"""
    return {k: float(np.abs(np.asarray(got[k], np.float64) - want[k]).max() / max(np.abs(want[k]).max(), 1e-300)) for k in want}

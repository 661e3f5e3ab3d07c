"""fp64 restatement of the cutoff envelope (include/e3gnn.h, e3_cutoff_envelope) and of the enveloped energy models, used by
tests/test_envelope_host.py and tests/test_envelope_gpu.py.  TEST INFRASTRUCTURE ONLY.

The layer sequence is the one of ``virial_reference.energy_forces_strain`` with two changes: every message is weighted by
w_e = u_p(d_e / r_c) in the aggregation, a_i = sum_e w_e m_e, and the node attribute is the enveloped one,
A_i = [1, sum_e w_e Y_e[1:] / (1 + sum_e w_e)].  The edge vectors are the minimum image in a box ``L`` or a general ``cell``
(or plain differences), strained by a leaf eps per structure; d_e is the length of the strained vector."""
import numpy as np


def envelope64(d, r_c, p):
    """u_p(min(d / r_c, 1)) in the Horner form of the header; torch fp64, differentiable w.r.t. d."""
    import torch
    x = torch.clamp(d / r_c, max=1.0)
    s = torch.full_like(x, (p + 1) * p / 2.0)
    for k in range(p - 2, -1, -1):
        s = s * x + (k + 2) * (k + 1) / 2.0
    return (1.0 - x) ** 3 * s


def envelope_expanded64(d, r_c, p):
    """The same polynomial expanded (DimeNet): 1 - (p+1)(p+2)/2 x^p + p(p+2) x^(p+1) - p(p+1)/2 x^(p+2).  Cancels near x = 1."""
    import torch
    x = torch.clamp(d / r_c, max=1.0)
    return 1.0 - (p + 1) * (p + 2) / 2.0 * x ** p + p * (p + 2.0) * x ** (p + 1) - p * (p + 1) / 2.0 * x ** (p + 2)


def envelope_derivative64(d, r_c, p):
    """du/dd = -(p (p+1) (p+2) / 2) x^(p-1) (1 - x)^2 / r_c."""
    import torch
    x = torch.clamp(d / r_c, max=1.0)
    return -(p * (p + 1) * (p + 2) / 2.0) * x ** (p - 1) * (1.0 - x) ** 2 / r_c


def energy_forces_strain(params, H, num_layers, lmax, in_irreps, x, pos, rowptr, src, r_c, p, L=None, cell=None,
                         structure=None, S=1, eps=None, per_structure=False):
    """-> energy (float, or [S] array with ``per_structure``), forces [N,3] = -dE/dpos, dE/deps [S,3,3] of the ENVELOPED
    model.  ``r_c``, ``p``: the envelope; ``L`` box lengths per axis (0 or None = open) or ``cell`` [3,3] (rows = lattice
    vectors); ``structure`` [N] (graph order, None = every row is 0), ``eps`` [S,3,3] (None = zero)."""
    import torch
    from oracle import segnn_oracle as Sg
    from oracle import tp_oracle as T
    hid = f"{H}x0e+{H}x1o" + (f"+{H}x2e" if lmax == 2 else "")
    gated = f"{H}x0e+{lmax * H}x0e+{H}x1o" + (f"+{H}x2e" if lmax == 2 else "")
    rowptr_t, src_t = torch.as_tensor(np.asarray(rowptr)).long(), torch.as_tensor(np.asarray(src)).long()
    N = rowptr_t.numel() - 1
    deg = rowptr_t[1:] - rowptr_t[:-1]
    dst_t = torch.repeat_interleave(torch.arange(N), deg)
    sid = torch.zeros(N, dtype=torch.long) if structure is None else torch.as_tensor(np.asarray(structure)).long()
    pos = torch.as_tensor(np.asarray(pos), dtype=torch.float64).clone().requires_grad_(True)
    e0 = np.zeros((S, 3, 3)) if eps is None else np.asarray(eps, np.float64).reshape(S, 3, 3)
    eps_t = torch.as_tensor(e0, dtype=torch.float64).clone().requires_grad_(True)
    P = {k: torch.as_tensor(v, dtype=torch.float64) for k, v in params.items()}
    rel = pos[src_t] - pos[dst_t]
    raw = rel.detach().numpy()
    if cell is not None:  # the shift is constant
        c = np.asarray(cell, np.float64)
        rel = rel - torch.as_tensor(np.rint(raw @ np.linalg.inv(c)) @ c)
    elif L is not None:
        Ln = np.asarray(L, np.float64)
        rel = rel - torch.as_tensor(np.where(Ln > 0, Ln * np.round(raw / np.where(Ln > 0, Ln, 1.0)), 0.0))
    rel = rel + torch.einsum("eab,eb->ea", eps_t[sid[dst_t]], rel)
    Y, d = Sg.sh_component_torch(lmax, rel)
    w = envelope64(d, float(r_c), int(p))
    ny = (lmax + 1) ** 2
    Sw = torch.zeros(N, ny, dtype=torch.float64).index_add(0, dst_t, w[:, None] * Y)
    A = torch.cat([torch.ones(N, 1, dtype=torch.float64), Sw[:, 1:] / (1.0 + Sw[:, :1])], 1)

    def tp2(prefix, in1, in2, ii, oi):
        W = {c: P[f"{prefix}.weights_{c}"] for c in T.CLASSES if f"{prefix}.weights_{c}" in P}
        Nn = {c: P[f"{prefix}.norm_{c}"] for c in T.CLASSES if f"{prefix}.norm_{c}" in P}
        for c in T.CLASSES:
            Nn.setdefault(c, torch.ones(0, dtype=torch.float64))
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

    h = tp2("embed", torch.as_tensor(np.asarray(x), dtype=torch.float64), A, in_irreps, hid)
    for l in range(num_layers):
        pre = f"layers.{l}"
        m = torch.cat([h[dst_t], h[src_t], d[:, None]], 1)
        m = g(tp2(pre + ".msg1", m, Y, f"{hid}+{hid}+1x0e", gated))
        m = g(tp2(pre + ".msg2", m, Y, hid, gated))
        a = torch.zeros_like(h).index_add(0, dst_t, w[:, None] * m)
        u = g(tp2(pre + ".upd1", torch.cat([h, a], 1), A, f"{hid}+{hid}", gated))
        h = h + tp2(pre + ".upd2", u, A, hid, hid)
    e_node = tp2("readout", h, A, hid, "1x0e")[:, 0]
    energy = e_node.sum()
    gpos, geps = torch.autograd.grad(energy, [pos, eps_t])
    if per_structure:
        e_out = torch.zeros(S, dtype=torch.float64).index_add(0, sid, e_node.detach()).numpy()
    else:
        e_out = float(energy.detach())
    return e_out, -gpos.numpy(), geps.numpy()

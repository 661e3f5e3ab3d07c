"""fp64 torch autograd restatement of the strained energy (include/e3gnn.h, e3_edge_geometry_strained), used by
tests/test_virial_reference_host.py and tests/test_stress_gpu.py.  TEST INFRASTRUCTURE ONLY.

The layer sequence is the one of ``pbc_reference.energy_forces_pbc``; the one change is a leaf strain ``eps`` [S,3,3]
applied to every edge vector of the undeformed graph, r' = r + eps[s] r with r the minimum image of x_src - x_dst (plain
x_src - x_dst on open axes) and s the structure of the edge's dst row.  Y, d and A are formed from r'."""
import numpy as np


def energy_forces_strain(params, H, num_layers, lmax, in_irreps, x, pos, rowptr, src, L=None, structure=None, S=1,
                         eps=None, per_structure=False):
    """-> energy (float, or [S] array with ``per_structure``), forces [N,3] = -dE/dpos, dE/deps [S,3,3] (of the total
    energy; eps_s only moves the edges of structure s).  ``structure`` [N] (graph order, None = every row is 0), ``eps``
    [S,3,3] (None = zero), ``L`` box lengths per axis (0 or None = open)."""
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
    Lt = torch.as_tensor(np.zeros(3) if L is None else np.asarray(L, np.float64))
    shift = torch.where(Lt > 0, Lt * torch.round(rel.detach() / torch.where(Lt > 0, Lt, 1.0)), 0.0)
    rel = rel - shift
    rel = rel + torch.einsum("eab,eb->ea", eps_t[sid[dst_t]], rel)
    Y, d = Sg.sh_component_torch(lmax, rel)
    ny = (lmax + 1) ** 2
    A = torch.cat([torch.ones(N, 1, dtype=torch.float64),
                   torch.zeros(N, ny - 1, dtype=torch.float64).index_add(0, dst_t, Y[:, 1:]) / deg.clamp_min(1)[:, None]], 1)

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
            w = 2 * l + 1
            out.append((torch.sigmoid(t[:, g0:g0 + H])[:, :, None] * t[:, c0:c0 + H * w].reshape(-1, H, w)).reshape(-1, H * w))
            g0 += H
            c0 += H * w
        return torch.cat(out, 1)

    h = tp2("embed", torch.as_tensor(np.asarray(x), dtype=torch.float64), A, in_irreps, hid)
    for l in range(num_layers):
        p = f"layers.{l}"
        m = torch.cat([h[dst_t], h[src_t], d[:, None]], 1)
        m = g(tp2(p + ".msg1", m, Y, f"{hid}+{hid}+1x0e", gated))
        m = g(tp2(p + ".msg2", m, Y, hid, gated))
        a = torch.zeros_like(h).index_add(0, dst_t, m)
        u = g(tp2(p + ".upd1", torch.cat([h, a], 1), A, f"{hid}+{hid}", gated))
        h = h + tp2(p + ".upd2", u, A, hid, hid)
    e_node = tp2("readout", h, A, hid, "1x0e")[:, 0]
    energy = e_node.sum()
    gpos, geps = torch.autograd.grad(energy, [pos, eps_t])
    if per_structure:
        e_out = torch.zeros(S, dtype=torch.float64).index_add(0, sid, e_node.detach()).numpy()
    else:
        e_out = float(energy.detach())
    return e_out, -gpos.numpy(), geps.numpy()

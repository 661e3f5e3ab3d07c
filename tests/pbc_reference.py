"""numpy / torch restatements of the periodic box (include/e3gnn.h, e3_rg_sort_count_pbc and e3_edge_geometry_pbc), used
by tests/test_periodic_*.py.  TEST INFRASTRUCTURE ONLY.

The graph restatement is bit for bit: float32 numpy arithmetic rounds every operation, as the kernels do with
``__fsub_rn`` / ``__fmul_rn``; the Morton order comes from ``oracle/graph_oracle.order`` on the wrapped coordinates."""
import numpy as np

from oracle import graph_oracle as G

f32 = np.float32


def axes_of(periodic):
    if isinstance(periodic, (bool, int)):
        return [bool(periodic)] * 3
    return [bool(a) for a in periodic]


def box_lengths(lo, hi, periodic):
    """L_a = fl32(hi_a - lo_a) on periodic axes, 0 on open axes (the ``box`` of the *_pbc entries)."""
    ax = axes_of(periodic)
    return np.array([f32(f32(hi[a]) - f32(lo[a])) if ax[a] else 0.0 for a in range(3)], dtype=f32)


def wrap(pos, lo, hi, periodic):
    """w = p - L floor((p - lo) / L), then one correction step into [lo, hi) -- periodic axes only."""
    p = np.array(pos, dtype=f32, copy=True)
    ax = axes_of(periodic)
    for a in range(3):
        if not ax[a]:
            continue
        lo_a, hi_a = f32(lo[a]), f32(hi[a])
        L = f32(hi_a - lo_a)
        invL = f32(f32(1.0) / L)
        x = p[:, a]
        w = x - L * np.floor((x - lo_a) * invL)
        w = np.where(w >= hi_a, w - L, np.where(w < lo_a, w + L, w)).astype(f32)
        p[:, a] = w
    return p


def edges_of(sp, r, L, chunk=256):
    """CSR by dst of the one-step minimum-image edge test on wrapped, ordered positions ``sp`` (L = 0: open axis)."""
    sp = np.asarray(sp, dtype=f32)
    N = sp.shape[0]
    L = np.asarray(L, dtype=f32)
    hL = np.where(L > 0, f32(0.5) * L, f32(np.inf)).astype(f32)
    r2 = f32(f32(r) * f32(r))
    rowptr = np.zeros(N + 1, np.int64)
    srcs = []
    for i0 in range(0, N, chunk):
        i1 = min(N, i0 + chunk)
        d = sp[i0:i1, None, :] - sp[None, :, :]
        for a in range(3):
            da = d[..., a]
            d[..., a] = np.where(da > hL[a], da - L[a], np.where(da < -hL[a], da + L[a], da))
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        adj = d2 <= r2
        adj[np.arange(i1 - i0), np.arange(i0, i1)] = False
        rr, cc = np.nonzero(adj)
        rowptr[i0 + 1:i1 + 1] = np.cumsum(np.bincount(rr, minlength=i1 - i0))
        rowptr[i0 + 1:i1 + 1] += rowptr[i0]
        srcs.append(cc.astype(np.int32))
    src = np.concatenate(srcs) if srcs else np.zeros(0, np.int32)
    return rowptr.astype(np.int32), src


def graph_pbc(pos, lo, hi, r, periodic):
    """-> perm, pos4 [N,4] (wrapped, new order), rowptr, src: what radius_graph(..., periodic=) must return."""
    w = wrap(pos, lo, hi, periodic)
    perm, _ = G.order(w, G.params(lo, hi, r))
    sp = w[perm]
    rowptr, src = edges_of(sp, r, box_lengths(lo, hi, periodic))
    pos4 = np.concatenate([sp, np.zeros((len(sp), 1), f32)], 1)
    return perm, pos4, rowptr, src


def min_image64(rel, L):
    """fp64 minimum image of edge vectors [E,3] (L = 0: open axis)."""
    rel = np.array(rel, dtype=np.float64, copy=True)
    for a in range(3):
        if L[a] > 0:
            rel[:, a] -= float(L[a]) * np.round(rel[:, a] / float(L[a]))
    return rel


def sh64(lmax, rel):
    """fp64 component-normalised real SH [E,(lmax+1)^2] and lengths of edge vectors (basis of oracle/cg.py)."""
    d = np.linalg.norm(rel, axis=1)
    u = rel / np.maximum(d, 1e-300)[:, None]
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    parts = [np.ones((len(d), 1)), np.sqrt(3.0) * u]
    if lmax == 2:
        s3 = np.sqrt(3.0)
        parts.append(np.sqrt(5.0) * np.stack([s3 * x * y, s3 * y * z, (2 * z * z - x * x - y * y) / 2, s3 * z * x,
                                              s3 / 2 * (x * x - y * y)], 1))
    return np.concatenate(parts, 1), d


def tile27(pos, L):
    """The cloud [N,3] tiled 3 x 3 x 3 by the box vectors -> [27 N, 3] (copy k = offset index), index of the centre copy."""
    offs = [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)]
    out = np.concatenate([pos + np.asarray(o, np.float64) * np.asarray(L, np.float64) for o in offs], 0)
    return out, offs.index((0, 0, 0))


def energy_forces_pbc(params, H, num_layers, lmax, in_irreps, x, pos, rowptr, src, L):
    """fp64 torch autograd of the energy (sum of the 1x0e readout over the nodes) on minimum-image edge vectors:
    the layer sequence of ``segnn_oracle.energy_forces_torch`` with rel = minimum image of pos[src] - pos[dst]
    (the shift is constant).  -> energy, forces [N,3]."""
    import torch
    from oracle import segnn_oracle as S
    from oracle import tp_oracle as T
    hid = f"{H}x0e+{H}x1o" + (f"+{H}x2e" if lmax == 2 else "")
    gated = f"{H}x0e+{lmax * H}x0e+{H}x1o" + (f"+{H}x2e" if lmax == 2 else "")
    rowptr_t, src_t = torch.as_tensor(rowptr).long(), torch.as_tensor(src).long()
    N = rowptr_t.numel() - 1
    deg = rowptr_t[1:] - rowptr_t[:-1]
    dst_t = torch.repeat_interleave(torch.arange(N), deg)
    pos = torch.as_tensor(pos, dtype=torch.float64).clone().requires_grad_(True)
    P = {k: torch.as_tensor(v, dtype=torch.float64) for k, v in params.items()}
    rel = pos[src_t] - pos[dst_t]
    Lt = torch.as_tensor(np.asarray(L, np.float64))
    shift = torch.where(Lt > 0, Lt * torch.round(rel.detach() / torch.where(Lt > 0, Lt, 1.0)), 0.0)
    Y, d = S.sh_component_torch(lmax, rel - shift)
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

    h = tp2("embed", torch.as_tensor(x, dtype=torch.float64), A, in_irreps, hid)
    for l in range(num_layers):
        p = f"layers.{l}"
        m = torch.cat([h[dst_t], h[src_t], d[:, None]], 1)
        m = g(tp2(p + ".msg1", m, Y, f"{hid}+{hid}+1x0e", gated))
        m = g(tp2(p + ".msg2", m, Y, hid, gated))
        a = torch.zeros_like(h).index_add(0, dst_t, m)
        u = g(tp2(p + ".upd1", torch.cat([h, a], 1), A, f"{hid}+{hid}", gated))
        h = h + tp2(p + ".upd2", u, A, hid, hid)
    energy = tp2("readout", h, A, hid, "1x0e")[:, 0].sum()
    (gpos,) = torch.autograd.grad(energy, [pos])
    return float(energy.detach()), -gpos.numpy()

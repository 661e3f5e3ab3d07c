"""numpy / torch restatements of the general periodic cell (include/e3gnn.h, e3_rg_sort_count_cell and the *_cell
entries), used by tests/test_triclinic_*.py.  TEST INFRASTRUCTURE ONLY.

The graph restatement is bit for bit: float32 numpy arithmetic rounds every operation, as the kernels do with
``__fsub_rn`` / ``__fmul_rn`` / ``__fadd_rn``; the derived quantities (G, heights, volume) repeat the library's fp64
expressions in the same order; the Morton order comes from ``oracle/graph_oracle.order`` on the grid points q."""
import numpy as np

from oracle import graph_oracle as G

f32 = np.float32

# the cells of the tests: T (dyadic entries: whole-lattice shifts of points on the 2^-16 grid are exact in fp32),
# T' = M T (the same lattice), and a fixed rotation
T = np.array([[1.0, 0.0, 0.0], [0.25, 0.875, 0.0], [0.125, -0.25, 0.75]])
M = np.array([[1, 1, 0], [0, 1, 1], [0, 0, 1]], np.float64)
TP = M @ T


def rotation():
    """A fixed proper rotation (Rodrigues, axis (1,2,3)/sqrt14, angle 0.7), fp64."""
    k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * (K @ K)


def derive(cell):
    """-> G [3,3] fp32 (= fl32 of cell^-1), heights [3] fp32, volume fp32: the fp64 expressions of the library
    (cofactors over the determinant, from the fp32 entries), rounded once."""
    a = np.asarray(cell, f32).astype(np.float64).reshape(9)
    c00 = a[4] * a[8] - a[5] * a[7]; c01 = a[5] * a[6] - a[3] * a[8]; c02 = a[3] * a[7] - a[4] * a[6]
    c10 = a[2] * a[7] - a[1] * a[8]; c11 = a[0] * a[8] - a[2] * a[6]; c12 = a[1] * a[6] - a[0] * a[7]
    c20 = a[1] * a[5] - a[2] * a[4]; c21 = a[2] * a[3] - a[0] * a[5]; c22 = a[0] * a[4] - a[1] * a[3]
    det = (a[0] * c00 + a[1] * c01) + a[2] * c02
    g = np.array([c00 / det, c10 / det, c20 / det, c01 / det, c11 / det, c21 / det, c02 / det, c12 / det, c22 / det])
    hgt = np.array([1.0 / np.sqrt((g[c] * g[c] + g[3 + c] * g[3 + c]) + g[6 + c] * g[6 + c]) for c in range(3)])
    return g.astype(f32).reshape(3, 3), hgt.astype(f32), f32(abs(det))


def frac(v, g):
    """fl(fl(fl(v_0 G[0,a]) + fl(v_1 G[1,a])) + fl(v_2 G[2,a])) for a = 0..2; v [...,3] fp32."""
    v = np.asarray(v, f32)
    return np.stack([(v[..., 0] * g[0, a] + v[..., 1] * g[1, a]) + v[..., 2] * g[2, a] for a in range(3)], -1).astype(f32)


def shift(v, n, cell):
    """v_c - fl(fl(fl(n_0 cell[0,c]) + fl(n_1 cell[1,c])) + fl(n_2 cell[2,c])); n [...,3] fp32 whole numbers."""
    n = np.asarray(n, f32)
    return np.stack([v[..., c] - ((n[..., 0] * cell[0, c] + n[..., 1] * cell[1, c]) + n[..., 2] * cell[2, c])
                     for c in range(3)], -1).astype(f32)


def wrap(pos, cell, origin):
    cell = np.asarray(cell, f32)
    g, _, _ = derive(cell)
    o = np.asarray(origin, f32)
    p = np.asarray(pos, f32)
    w = shift(p, np.floor(frac(p - o, g)), cell)
    s = frac(w - o, g)
    for a in range(3):
        up, down = s[:, a] >= 1, s[:, a] < 0
        w = np.where(up[:, None], w - cell[a], np.where(down[:, None], w + cell[a], w)).astype(f32)
    return w


def grid_points(w, cell, origin):
    """q_a = fl(s_a(w) h_a)."""
    g, hgt, _ = derive(cell)
    return (frac(np.asarray(w, f32) - np.asarray(origin, f32), g) * hgt).astype(f32)


def edges_of(sp, r, cell, chunk=128):
    """CSR by dst of the rint minimum-image edge test on wrapped, ordered positions (the shift is the identity where the
    kernel skips it)."""
    sp = np.asarray(sp, f32)
    cell = np.asarray(cell, f32)
    g, _, _ = derive(cell)
    N = sp.shape[0]
    r2 = f32(f32(r) * f32(r))
    rowptr = np.zeros(N + 1, np.int64)
    srcs = []
    for i0 in range(0, N, chunk):
        i1 = min(N, i0 + chunk)
        d = (sp[i0:i1, None, :] - sp[None, :, :]).astype(f32)
        d = shift(d, np.rint(frac(d, g)), cell)
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        adj = d2 <= r2
        adj[np.arange(i1 - i0), np.arange(i0, i1)] = False
        rr, cc = np.nonzero(adj)
        rowptr[i0 + 1:i1 + 1] = np.cumsum(np.bincount(rr, minlength=i1 - i0))
        rowptr[i0 + 1:i1 + 1] += rowptr[i0]
        srcs.append(cc.astype(np.int32))
    src = np.concatenate(srcs) if srcs else np.zeros(0, np.int32)
    return rowptr.astype(np.int32), src


def graph_cell(pos, cell, r, origin=(0.0, 0.0, 0.0)):
    """-> perm, pos4 [N,4] (wrapped, new order), rowptr, src: what radius_graph(..., cell=, origin=) must return."""
    cell = np.asarray(cell, f32)
    _, hgt, _ = derive(cell)
    w = wrap(pos, cell, origin)
    perm, _ = G.order(grid_points(w, cell, origin), G.params([0.0, 0.0, 0.0], hgt, r))
    sp = w[perm]
    rowptr, src = edges_of(sp, r, cell)
    return perm, np.concatenate([sp, np.zeros((len(sp), 1), f32)], 1), rowptr, src


# ---------------------------------------------------------------------------------------------------------------------
# fp64
# ---------------------------------------------------------------------------------------------------------------------
def min_image64_cell(rel, cell):
    """fp64 minimum image of edge vectors [E,3]: rel - rint(rel cell^-1) cell."""
    rel = np.asarray(rel, np.float64)
    cell = np.asarray(cell, np.float64)
    return rel - np.rint(rel @ np.linalg.inv(cell)) @ cell


def tile27(pos, cell):
    """The cloud [N,3] tiled 3 x 3 x 3 by the lattice vectors -> [27 N, 3], index of the centre copy."""
    cell = np.asarray(cell, np.float64)
    offs = [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)]
    out = np.concatenate([np.asarray(pos, np.float64) + np.asarray(o, np.float64) @ cell for o in offs], 0)
    return out, offs.index((0, 0, 0))


def brute_pairs64(w, cell, r, tie=1e-6, chunk=256):
    """fp64 search over the 27 lattice images of wrapped points -> (sorted codes i * N + j of the directed pairs with
    |d| <= r, the same for the pairs within ``tie`` of the cutoff)."""
    w = np.asarray(w, np.float64)
    cell = np.asarray(cell, np.float64)
    N = len(w)
    offs = np.array([(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)], np.float64) @ cell
    inside, ties = [], []
    for i0 in range(0, N, chunk):
        i1 = min(N, i0 + chunk)
        d = w[i0:i1, None, :] - w[None, :, :]
        dist2 = np.full(d.shape[:2], np.inf)
        for o in offs:
            e = d + o
            np.minimum(dist2, np.einsum("ijc,ijc->ij", e, e), out=dist2)
        dist = np.sqrt(dist2)
        dist[np.arange(i1 - i0), np.arange(i0, i1)] = np.inf
        ii, jj = np.nonzero(dist <= r + tie)
        dd = dist[ii, jj]
        code = (ii + i0).astype(np.int64) * N + jj
        ties.append(code[np.abs(dd - r) <= tie])
        inside.append(code[dd <= r])
    return np.sort(np.concatenate(inside)), np.sort(np.concatenate(ties))


def energy_forces_strain_cell(params, H, num_layers, lmax, in_irreps, x, pos, rowptr, src, cell, eps=None):
    """fp64 torch autograd of the energy (sum of the 1x0e readout over the nodes) on the cell's minimum-image edge
    vectors, strained by one leaf eps [3,3]: the layer sequence of ``virial_reference.energy_forces_strain`` with
    rel = d - rint(d cell^-1) cell, d = pos[src] - pos[dst] (the shift is constant), then r' = rel + eps rel.
    -> energy, forces [N,3] = -dE/dpos, dE/deps [3,3]."""
    import torch
    from oracle import segnn_oracle as Sg
    from oracle import tp_oracle as Tp
    hid = f"{H}x0e+{H}x1o" + (f"+{H}x2e" if lmax == 2 else "")
    gated = f"{H}x0e+{lmax * H}x0e+{H}x1o" + (f"+{H}x2e" if lmax == 2 else "")
    rowptr_t, src_t = torch.as_tensor(np.asarray(rowptr)).long(), torch.as_tensor(np.asarray(src)).long()
    N = rowptr_t.numel() - 1
    deg = rowptr_t[1:] - rowptr_t[:-1]
    dst_t = torch.repeat_interleave(torch.arange(N), deg)
    pos = torch.as_tensor(np.asarray(pos), dtype=torch.float64).clone().requires_grad_(True)
    eps_t = torch.as_tensor(np.zeros((3, 3)) if eps is None else np.asarray(eps, np.float64)).clone().requires_grad_(True)
    P = {k: torch.as_tensor(v, dtype=torch.float64) for k, v in params.items()}
    rel = pos[src_t] - pos[dst_t]
    rel = rel - torch.as_tensor(rel.detach().numpy() - min_image64_cell(rel.detach().numpy(), cell))
    rel = rel + rel @ eps_t.T
    Y, d = Sg.sh_component_torch(lmax, rel)
    ny = (lmax + 1) ** 2
    A = torch.cat([torch.ones(N, 1, dtype=torch.float64),
                   torch.zeros(N, ny - 1, dtype=torch.float64).index_add(0, dst_t, Y[:, 1:]) / deg.clamp_min(1)[:, None]], 1)

    def tp2(prefix, in1, in2, ii, oi):
        W = {c: P[f"{prefix}.weights_{c}"] for c in Tp.CLASSES if f"{prefix}.weights_{c}" in P}
        Nn = {c: P[f"{prefix}.norm_{c}"] for c in Tp.CLASSES if f"{prefix}.norm_{c}" in P}
        for c in Tp.CLASSES:
            Nn.setdefault(c, torch.ones(0, dtype=torch.float64))
        return Tp.forward_torch_cpu(ii, oi, lmax, in1, in2, W, Nn)

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
    energy = tp2("readout", h, A, hid, "1x0e")[:, 0].sum()
    gpos, geps = torch.autograd.grad(energy, [pos, eps_t])
    return float(energy.detach()), -gpos.numpy(), geps.numpy()

"""numpy / torch twin of the image rows of a small periodic cell (include/e3gnn.h, "Image rows"; cell_images.py), the cases
of tests/test_cell_images_*.py and their fp64 oracles.  TEST INFRASTRUCTURE ONLY.

The selection twin is bit for bit: float32 numpy arithmetic rounds every operation, as the kernels do with the ``__f*_rn``
intrinsics; wrap / frac / shift are those of ``triclinic_reference``.  The brute-force lattice sum is fp64 over one shell
more than the selection uses, so an image the selection drops but an edge needs shows up as a missing pair."""
import itertools

import numpy as np

import triclinic_reference as TR

f32 = np.float32
MAX_SHELLS = 7

# name -> cell rows, N, r, seed, shells, the smallest supercell with 2 r < every height, images, edges (checked on the CPU in
# fp64: the slab rule keeps every needed image and no pair lies closer to r than the gap)
CASES = {
    "tri5":   dict(cell=[[1, 0, 0], [.3, 1.1, 0], [.2, -.25, .9]], N=5, r=1.25, seed=1, shells=(2, 2, 2), tile=(3, 3, 3),
                   images=271, edges=200, gap=3.6e-3),
    "sc1":    dict(cell=[[1, 0, 0], [0, 1, 0], [0, 0, 1]], N=1, r=1.5, seed=2, shells=(2, 2, 2), tile=(4, 4, 4),
                   images=63, edges=18, gap=8.6e-2),
    "mixed":  dict(cell=[[4, 0, 0], [.5, 1.2, 0], [0, .3, 4.5]], N=12, r=1.8, seed=3, shells=(1, 2, 1), tile=(1, 4, 1),
                   images=156, edges=180, gap=3.0e-3),
    "flat":   dict(cell=[[1, 0, 0], [.9, .5, 0], [.1, .2, 1.3]], N=3, r=1.1, seed=4, shells=(3, 3, 1), tile=(5, 5, 2),
                   images=237, edges=86, gap=3.3e-3),
    "fcc2":   dict(cell=[[0, .5, .5], [.5, 0, .5], [.5, .5, 0]], N=2, r=0.9, seed=6, shells=(2, 2, 2), tile=(4, 4, 4),
                   images=187, edges=50, gap=3.8e-4),
    "big300": dict(cell=[[3, 0, 0], [.4, 3.2, 0], [.3, -.2, 2.9]], N=300, r=0.8, seed=5, shells=(1, 1, 1), tile=(1, 1, 1),
                   images=774, edges=6918, gap=8.7e-5),
}
SMALL = ("tri5", "sc1", "mixed", "flat", "fcc2")

# `far`: heights of about 100 r, so the margin rho is dominated by the cell size.  Per axis a: a pair straddling the face at
# fractions 2^-12 and 1 - 2^-12, and a particle ON the face (fraction 0) with two partners straight across it along the
# face normal, at 0.99985 r (an edge through the image) and 1.00015 r (none): 1.5e-4 r from the cutoff on either side.
FAR_CELL = [[100.0, 0.0, 0.0], [3.0, 101.0, 0.0], [-2.0, 4.0, 99.0]]
FAR_R = 1.0


def far_positions():
    cell = np.asarray(FAR_CELL, np.float64)
    ginv = np.linalg.inv(cell)
    out = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        normal = ginv[:, a] / np.linalg.norm(ginv[:, a])
        s = np.zeros(3)
        s[b], s[c] = 0.25 + 0.125 * a, 0.5
        for sa in (2.0 ** -12, 1.0 - 2.0 ** -12):
            t = s.copy()
            t[a] = sa
            out.append(t @ cell)
        s[b] = 0.625
        on_face = s @ cell
        out.append(on_face)
        partner = np.array([0.0, 0.0, 0.0])
        partner[b] = 0.375
        partner[c] = 0.75
        partner = partner @ cell
        out += [on_face - 0.99985 * FAR_R * normal + cell[a]]
        out += [partner, partner - 1.00015 * FAR_R * normal + cell[a]]
    return np.asarray(out)


def case(name):
    """-> (cell [3,3] fp64, pos [N,3] fp64 inside the cell, r)"""
    if name == "far":
        return np.asarray(FAR_CELL, np.float64), far_positions(), FAR_R
    c = CASES[name]
    cell = np.asarray(c["cell"], np.float64)
    frac = np.random.default_rng(c["seed"]).integers(0, 1 << 12, (c["N"], 3)) / 4096.0
    return cell, frac @ cell, c["r"]


ALL = tuple(CASES) + ("far",)


def plan(cell, origin, r):
    """-> (shells [3] int, rho fp32): rho = r + 2^-18 (r + sum |cell| + sum |origin|) in fp64 in the library's order, rounded
    up to fp32; m_a = max(1, ceil(rho / h_a)); ValueError above MAX_SHELLS."""
    cell32, o32 = np.asarray(cell, f32).reshape(9), np.asarray(origin, f32)
    size = np.float64(f32(r))
    for v in cell32:
        size = size + abs(np.float64(v))
    for v in o32:
        size = size + abs(np.float64(v))
    rho64 = np.float64(f32(r)) + size * (1.0 / 262144.0)
    rho = f32(rho64)
    if np.float64(rho) < rho64:
        rho = np.nextafter(rho, f32(np.inf))
    _, hgt, _ = TR.derive(cell32.reshape(3, 3))
    m = [max(1, int(np.ceil(np.float64(rho) / np.float64(h)))) for h in hgt]
    if max(m) > MAX_SHELLS:
        raise ValueError(f"more than {MAX_SHELLS} image shells")
    return m, rho


def select(pos, cell, origin, r):
    """-> (pos_w [N,3] fp32, owner [G] int32, shift [G,3] int32, image_pos [G,3] fp32) in (owner, shift) order"""
    cell32, o32 = np.asarray(cell, f32).reshape(3, 3), np.asarray(origin, f32)
    m, rho = plan(cell32, o32, r)
    g, hgt, _ = TR.derive(cell32)
    w = TR.wrap(np.asarray(pos, f32).reshape(-1, 3), cell32, o32)
    s = TR.frac((w - o32).astype(f32), g)
    keep = []                                        # per axis [N, 2 m + 1]
    for a in range(3):
        n = np.arange(-m[a], m[a] + 1).astype(f32)
        t = (s[:, a:a + 1] + n[None, :]).astype(f32)
        lo = (t * hgt[a]).astype(f32) >= -rho
        hi = ((t - f32(1)).astype(f32) * hgt[a]).astype(f32) <= rho
        keep.append(lo & hi)
    owner, shift = [], []
    for i in range(len(w)):
        for n0, n1, n2 in itertools.product(*(range(-m[a], m[a] + 1) for a in range(3))):
            if (n0, n1, n2) != (0, 0, 0) and keep[0][i, n0 + m[0]] and keep[1][i, n1 + m[1]] and keep[2][i, n2 + m[2]]:
                owner.append(i)
                shift.append((n0, n1, n2))
    owner = np.asarray(owner, np.int32)
    shift = np.asarray(shift, np.int32).reshape(-1, 3)
    image_pos = TR.shift(w[owner], (-shift).astype(f32), cell32) if len(owner) else np.zeros((0, 3), f32)
    return w, owner, shift, image_pos


def brute_edges64(w, cell, r, shells):
    """fp64 lattice sum over one shell more than ``shells`` on wrapped positions -> (set of (j, n0, n1, n2, i): image n of j
    within r of i, self pair excluded; the smallest | |d| - r | met)"""
    w, cell = np.asarray(w, np.float64), np.asarray(cell, np.float64)
    edges, gap = set(), np.inf
    idx = np.arange(len(w))
    for n in itertools.product(*(range(-m - 1, m + 2) for m in shells)):
        d = np.linalg.norm(w[None, :, :] + np.asarray(n, np.float64) @ cell - w[:, None, :], axis=-1)   # [i, j]
        if n == (0, 0, 0):
            d[idx, idx] = np.inf
        gap = min(gap, np.abs(d - r).min())
        ii, jj = np.nonzero(d <= r)
        edges.update((int(j), *n, int(i)) for i, j in zip(ii, jj))
    return edges, float(gap)


def supercell(pos_w, cell, tile):
    """The cloud tiled k_0 x k_1 x k_2, first tile first -> (pos [k N, 3] fp64, cell of the supercell [3,3])"""
    cell = np.asarray(cell, np.float64)
    offs = [np.asarray(n, np.float64) @ cell for n in itertools.product(*(range(k) for k in tile))]
    return np.concatenate([np.asarray(pos_w, np.float64) + o for o in offs]), cell * np.asarray(tile, np.float64)[:, None]


def min_image_graph64(pos, cell, r):
    """brute-force minimum-image graph of a cell with 2 r < every height -> rowptr [N + 1], src [E] (dst-sorted, src
    ascending, no self edge), fp64"""
    pos, cell = np.asarray(pos, np.float64), np.asarray(cell, np.float64)
    N = len(pos)
    d = TR.min_image64_cell((pos[None, :, :] - pos[:, None, :]).reshape(-1, 3), cell).reshape(N, N, 3)   # [dst, src]
    adj = (np.linalg.norm(d, axis=-1) <= r) & ~np.eye(N, dtype=bool)
    dst, src = np.nonzero(adj)
    return np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=N))]).astype(np.int64), src.astype(np.int64)


def row_map_numpy(source):
    """CSR of the image rows by owner, ascending inside a row -> (ptr [M + 1], rows [G])"""
    source = np.asarray(source, np.int64)
    img = np.nonzero(source != np.arange(len(source)))[0]
    order = np.argsort(source[img], kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(source[img], minlength=len(source)))])
    return ptr.astype(np.int32), img[order].astype(np.int32)

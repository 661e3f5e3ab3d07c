"""numpy restatement of the capped radius graph (include/e3gnn.h, "Capped rows": radius_graph(..., max_neighbors=k)), used by
tests/test_capped_graph_*.py.  TEST INFRASTRUCTURE ONLY.

Input is a reference UNCAPPED graph of the mode -- ``oracle.graph_oracle.graph``, ``pbc_reference.graph_pbc`` or
``triclinic_reference.graph_cell`` -- i.e. ordered (and wrapped) positions, ``rowptr`` and ``src``.  The d2 of every edge is
recomputed in float32 numpy arithmetic, which rounds every operation on its own as the kernels do, with the image shift of
the mode; per row the k smallest ``(d2, src)`` are kept and written back in ascending ``src``."""
import numpy as np

import triclinic_reference as R

f32 = np.float32


def edge_d2(sp, rowptr, src, box=None, cell=None):
    """fp32 d2 of every edge, the same bits as the edge test: d = x_dst - x_src, then the one-step shift of a box (``box`` =
    L per axis, 0 on an open axis: d > L/2 -> d - L, d < -L/2 -> d + L), or the rint shift of a ``cell``, then
    (dx dx + dy dy) + dz dz."""
    sp = np.asarray(sp, f32)[:, :3]
    rowptr = np.asarray(rowptr, np.int64)
    dst = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    d = (sp[dst] - sp[np.asarray(src, np.int64)]).astype(f32)
    if cell is not None:
        cell = np.asarray(cell, f32)
        g, _, _ = R.derive(cell)
        d = R.shift(d, np.rint(R.frac(d, g)), cell)
    elif box is not None:
        L = np.asarray(box, f32)
        hL = np.where(L > 0, f32(0.5) * L, f32(np.inf)).astype(f32)
        for a in range(3):
            da = d[:, a]
            d[:, a] = np.where(da > hL[a], da - L[a], np.where(da < -hL[a], da + L[a], da))
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert d2.dtype == f32
    return d2, dst


def cap(sp, rowptr, src, k, box=None, cell=None):
    """-> rowptr_capped [N+1] int32, src_capped int32, truncated rows, full edge count."""
    rowptr = np.asarray(rowptr, np.int64)
    src = np.asarray(src, np.int64)
    d2, dst = edge_d2(sp, rowptr, src, box, cell)
    order = np.lexsort((src, d2, dst))           # by row, then d2, then the source id
    rank = np.arange(len(src)) - rowptr[dst[order]]
    kept = np.sort(order[rank < k])              # edge order = ascending src inside each row
    deg = np.diff(rowptr)
    rowptr_c = np.concatenate([[0], np.cumsum(np.minimum(deg, k))])
    return rowptr_c.astype(np.int32), src[kept].astype(np.int32), int((deg > k).sum()), int(deg.sum())


def knn64(sp, r, k):
    """Plain fp64 k nearest inside r on ordered positions (open box, tiny N; meaningful only without fp32 ties)
    -> rowptr, src."""
    p = np.asarray(sp, np.float64)[:, :3]
    d = p[:, None, :] - p[None, :, :]
    dist2 = np.einsum("ijc,ijc->ij", d, d)
    np.fill_diagonal(dist2, np.inf)
    rows, counts = [], [0]
    for i in range(len(p)):
        inside = np.nonzero(dist2[i] <= float(f32(r)) ** 2)[0]
        best = inside[np.argsort(dist2[i, inside], kind="stable")[:k]]
        rows.append(np.sort(best))
        counts.append(counts[-1] + len(best))
    return np.asarray(counts, np.int32), np.concatenate(rows).astype(np.int32)

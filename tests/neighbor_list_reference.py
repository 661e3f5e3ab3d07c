"""numpy restatement of the Verlet-list entries (include/e3gnn.h, e3_nl_update / _pbc / _cell), used by
tests/test_neighbor_list_*.py.  TEST INFRASTRUCTURE ONLY.

Bit for bit: float32 numpy arithmetic rounds every operation, as the kernels do with ``__fsub_rn`` / ``__fmul_rn`` /
``__fadd_rn``; the cell's frac / shift are those of tests/triclinic_reference.py."""
import numpy as np

import triclinic_reference as TR

f32 = np.float32


def threshold(skin):
    """thr = fl(h h), h = fl(0.5 skin (1 - 2^-10)) of the fp32 skin."""
    h = f32(f32(0.5) * f32(skin)) * f32(1.0 - 2.0 ** -10)
    return f32(h * h)


def min_image(d, box=None, cell=None):
    """The rint minimum image of vectors d [...,3] fp32: per periodic axis fl(d - fl(L rint(fl(d invL)))), invL = fl(1 / L)
    (L = 0: open axis, the identity); in a cell shift(d, rint(frac(d))); the identity without a box or cell."""
    d = np.asarray(d, f32)
    if cell is not None:
        cell = np.asarray(cell, f32).reshape(3, 3)
        g, _, _ = TR.derive(cell)
        return TR.shift(d, np.rint(TR.frac(d, g)), cell)
    if box is None:
        return d
    out = d.copy()
    for a in range(3):
        L = f32(box[a])
        if L > 0:
            invL = f32(f32(1.0) / L)
            out[..., a] = d[..., a] - L * np.rint(d[..., a] * invL)
    return out.astype(f32)


def norm2(d):
    """fl(fl(fl(x x) + fl(y y)) + fl(z z)): the builder's sum order."""
    d = np.asarray(d, f32)
    return ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(f32)


def update(pos, perm, ref_pos4, rowptr, src, r, box=None, cell=None):
    """-> pos4_out [N,4], rowptr_out [N+1] int32, src_out, dst_out [E_r] int32, stats [2] uint32."""
    pos = np.asarray(pos, f32).reshape(-1, 3)
    perm, rowptr, src = np.asarray(perm, np.int64), np.asarray(rowptr, np.int64), np.asarray(src, np.int64)
    N = len(perm)
    cur = pos[perm]
    pos4 = np.concatenate([cur, np.zeros((N, 1), f32)], 1)
    stats = np.zeros(2, np.uint32)
    if N == 0:
        return pos4, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), stats
    with np.errstate(invalid="ignore", over="ignore"):
        disp = min_image(cur - np.asarray(ref_pos4, f32)[:, :3], box, cell)
        stats[0] = (norm2(disp).view(np.uint32) & np.uint32(0x7fffffff)).max()
        dst = np.repeat(np.arange(N), np.diff(rowptr))
        rel = min_image(cur[src] - cur[dst], box, cell)
        keep = norm2(rel) <= f32(f32(r) * f32(r))
    rowptr_out = np.concatenate([[0], np.cumsum(np.bincount(dst[keep], minlength=N))]).astype(np.int32)
    stats[1] = rowptr_out[-1]
    return pos4, rowptr_out, src[keep].astype(np.int32), dst[keep].astype(np.int32), stats


def max_d2(stats):
    """stats[0] as the float it holds (nan for a NaN pattern)."""
    return float(np.asarray(stats[:1], np.uint32).view(f32)[0])


# ---------------------------------------------------------------------------------------------------------------------
# fp64
# ---------------------------------------------------------------------------------------------------------------------
def pair_distances64(pos, box=None, cell=None):
    """[N,N] fp64 minimum-image distances of all pairs (inf on the diagonal); valid below half the smallest height."""
    p = np.asarray(pos, np.float64)
    d = (p[:, None, :] - p[None, :, :]).reshape(-1, 3)
    if cell is not None:
        d = TR.min_image64_cell(d, cell)
    elif box is not None:
        for a in range(3):
            if box[a] > 0:
                d[:, a] -= float(box[a]) * np.round(d[:, a] / float(box[a]))
    dist = np.sqrt((d * d).sum(1)).reshape(len(p), len(p))
    np.fill_diagonal(dist, np.inf)
    return dist


def pairs_of(perm, dst, src):
    """The directed pairs (dst, src) in caller ids, as sorted codes dst * N + src."""
    perm = np.asarray(perm, np.int64)
    return np.sort(perm[np.asarray(dst, np.int64)] * len(perm) + perm[np.asarray(src, np.int64)])


def pairs_within64(dist, r):
    ii, jj = np.nonzero(dist <= r)
    return np.sort(ii.astype(np.int64) * dist.shape[0] + jj)

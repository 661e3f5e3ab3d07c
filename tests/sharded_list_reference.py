"""numpy restatement of the fused prune + split entry (include/e3gnn.h, e3_nl_update_split) and of the ghost-position
update of the halo (sharding.Halo.displacement / update_positions), used by tests/test_sharded_list_*.py.
TEST INFRASTRUCTURE ONLY.

Bit for bit: float32 numpy arithmetic rounds every operation, as the kernels do with ``__fsub_rn`` / ``__fmul_rn`` /
``__fadd_rn``.  The prune is tests/neighbor_list_reference.py's open mode with the ghost rows emptied."""
import numpy as np

import neighbor_list_reference as NR

f32 = np.float32


def update_split(pos, perm, ref_pos4, rowptr, src, is_ghost, r):
    """-> pos4_out [N,4], rowptr_out [N+1] int32, (src, dst) kept, (src, dst) interior, (src, dst) boundary (int32 each),
    stats [4] uint32 = {bits of max d2 over all rows, E_kept, E_interior, E_boundary}."""
    pos = np.asarray(pos, f32).reshape(-1, 3)
    perm, rowptr, src = np.asarray(perm, np.int64), np.asarray(rowptr, np.int64), np.asarray(src, np.int64)
    ghost = np.asarray(is_ghost).astype(bool)
    N = len(perm)
    cur = pos[perm]
    pos4 = np.concatenate([cur, np.zeros((N, 1), f32)], 1)
    stats = np.zeros(4, np.uint32)
    empty = np.zeros(0, np.int32)
    if N == 0:
        return pos4, np.zeros(1, np.int32), (empty, empty), (empty, empty), (empty, empty), stats
    with np.errstate(invalid="ignore", over="ignore"):
        stats[0] = (NR.norm2(cur - np.asarray(ref_pos4, f32)[:, :3]).view(np.uint32) & np.uint32(0x7fffffff)).max()
        dst = np.repeat(np.arange(N), np.diff(rowptr))
        keep = (NR.norm2(cur[src] - cur[dst]) <= f32(f32(r) * f32(r))) & ~ghost[dst]
    s, d = src[keep], dst[keep]
    rowptr_out = np.concatenate([[0], np.cumsum(np.bincount(d, minlength=N))]).astype(np.int32)
    gs = ghost[s]
    lists = [(s[m].astype(np.int32), d[m].astype(np.int32)) for m in (np.ones_like(gs), ~gs, gs)]
    stats[1:] = [len(lists[0][0]), len(lists[1][0]), len(lists[2][0])]
    return pos4, rowptr_out, lists[0], lists[1], lists[2], stats


def displacement(pos, build_pos, lo, hi, mask):
    """Halo.displacement: d = fl(pos - build_pos), on the periodic axes of ``mask`` fl(d - fl(L rint(fl(d invL))))."""
    d = (np.asarray(pos, f32) - np.asarray(build_pos, f32)).astype(f32)
    box = [f32(f32(hi[a]) - f32(lo[a])) if (mask >> a) & 1 else f32(0.0) for a in range(3)]
    return NR.min_image(d, box)


def continued(pos, build_pos, build_local, lo, hi, mask):
    """The owned rows of Halo.update_positions: ``pos`` on an open axis, fl(build_local + displacement) on a periodic one."""
    d = displacement(pos, build_pos, lo, hi, mask)
    out = np.asarray(pos, f32).copy()
    for a in range(3):
        if (mask >> a) & 1:
            out[:, a] = np.asarray(build_local, f32)[:, a] + d[:, a]
    return out

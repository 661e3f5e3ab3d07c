"""numpy twin of the image rows of a BATCH of periodic cells (include/e3gnn.h, "Image rows", Batches;
cell_images.BatchedCellImages) and the batches of tests/test_batched_cells_*.py.  TEST INFRASTRUCTURE ONLY.

The twin is ``cell_images_reference.plan`` / ``select`` per structure, merged into the batched order: particles in the
caller's order, images by (owner in the caller's order, shift lexicographic).  Bit for bit, as the single-cell twin.

A batch has ONE cutoff, the cases of ``cell_images_reference`` have one each: every case is scaled by 1 / r_case, so the batch
runs at r = 1 and every count the cases record (shells, images, edges; all of them invariant under the scale) must come out
again -- the host test checks that on the twin, the device test on the kernels.  ``far`` has r = 1 and is not scaled."""
import numpy as np

import cell_images_reference as R

f32 = np.float32
BATCH_R = 1.0
EMPTY_CELL = [[2.0, 0.0, 0.0], [0.25, 1.75, 0.0], [0.0, -0.5, 2.5]]   # the structure without atoms


def scaled_case(name):
    """-> (cell [3,3] fp64, pos [N,3] fp64 inside the cell) of a case scaled to r = BATCH_R"""
    cell, pos, r = R.case(name)
    return cell * (BATCH_R / r), pos * (BATCH_R / r)


def origin_of(b):
    """a different non-zero origin for every structure (fp32-exact)"""
    return [0.375 - 0.25 * b, -1.25 + 0.5 * b, 2.5 - 0.125 * b]


def make_batch(names, empty_at=None, seed=11, order=None):
    """The structures ``names`` (one id each, in ``order`` if given: order[k] = the id of names[k]), with a structure without
    atoms at id ``empty_at``; every structure at its own origin and moved by whole lattice vectors, the atoms interleaved by a
    fixed permutation so that no structure is contiguous.
    -> dict(cells [B,3,3] fp64, origins [B,3], pos [N,3] fp32, batch [N] int64, names {id: name}, B)"""
    ids = list(order) if order is not None else [k + (empty_at is not None and k >= empty_at) for k in range(len(names))]
    B = len(names) + (empty_at is not None)
    assert sorted(ids + ([empty_at] if empty_at is not None else [])) == list(range(B))
    cells, origins = [None] * B, [origin_of(b) for b in range(B)]
    if empty_at is not None:
        cells[empty_at] = np.asarray(EMPTY_CELL, np.float64)
    rng = np.random.default_rng(seed)
    pos, batch = [], []
    for name, b in zip(names, ids):
        cell, p = scaled_case(name)
        n = rng.integers(-3, 4, (len(p), 3)).astype(np.float64)
        cells[b] = cell
        pos.append((p + np.asarray(origins[b]) + n @ cell).astype(f32))
        batch.append(np.full(len(p), b, np.int64))
    pos, batch = np.concatenate(pos), np.concatenate(batch)
    mix = np.random.default_rng(seed + 1).permutation(len(pos))
    return dict(cells=np.stack(cells), origins=np.asarray(origins, np.float64), pos=pos[mix], batch=batch[mix],
                names=dict(zip(ids, names)), B=B)


def plan_batch(cells, origins, r):
    """-> (shells [B][3], rho [B] fp32), per structure ``cell_images_reference.plan``"""
    out = [R.plan(c, o, r) for c, o in zip(cells, origins)]
    return [list(m) for m, _ in out], [rho for _, rho in out]


def select_batch(pos, batch, cells, origins, r):
    """-> (pos_w [N,3] fp32, owner [G] int32, shift [G,3] int32, image_pos [G,3] fp32, per {b: (idx, w, owner, shift,
    image_pos)} of the single-cell twin on structure b alone, idx = its particles in the caller's order)"""
    pos, batch = np.asarray(pos, f32).reshape(-1, 3), np.asarray(batch, np.int64)
    pos_w = np.zeros_like(pos)
    owner, shift, image_pos, per = [], [], [], {}
    for b in range(len(cells)):
        idx = np.nonzero(batch == b)[0]
        w, o, s, p = R.select(pos[idx], cells[b], origins[b], r)
        per[b] = (idx, w, o, s, p)
        pos_w[idx] = w
        owner.append(idx[o].astype(np.int32))
        shift.append(s)
        image_pos.append(p)
    owner, shift, image_pos = np.concatenate(owner), np.concatenate(shift), np.concatenate(image_pos)
    order = np.argsort(owner, kind="stable")          # inside one owner the shifts keep their lexicographic order
    return pos_w, owner[order], shift[order], image_pos[order], per

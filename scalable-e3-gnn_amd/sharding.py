"""Spatial sharding of the point cloud across GPUs (one process per GPU, RCCL over xGMI).

Builder-defined (the reference has no distributed code).  The domain is cut into a grid of axis-aligned
boxes, one per rank (``GridHalo``); a node's messages need neighbours within the cutoff ``r``, so each rank also holds
*ghost* copies of the particles of the (up to 26) adjacent boxes that lie within ``r`` of its own box.  The halo is a list of
*entries* ``(peer q, offset d, translation t)`` (``image_entries``), one per adjacent box: ``coords(me) + d`` is the adjacent
box, wrapped modulo ``dims`` on periodic axes, and ``t`` (whole box lengths per axis) moves q's box next to mine at offset
``d``.  In an open box every entry has ``t = 0`` and its own peer, in ascending rank order.

  * ``setup``      — once per graph build: the owner of a boundary particle sends it (position + input features) to every
                     entry whose box + r holds it; the local cloud is ``[owned | ghosts of entry 0 | of entry 1 | ...]``.
  * ``split_graph``— once per graph build: edges INTO ghost rows are dropped (their sums would be thrown away), the rest is
                     split into *interior* edges (owned src: computable before the layer's exchange has landed) and
                     *boundary* edges (ghost src).  On a GPU one HIP launch pair classifies and compacts (``e3_split_edges``).
  * ``update_positions`` — once per step between two builds (``sharded_list.ShardedNeighborList``): the current positions
                     and features travel along the entries, send lists and counts of the last ``setup`` -- no selection, no
                     count exchange, no host read; owned rows continue their build-time local coordinates across periodic
                     faces, a ghost is its owner's local position plus the entry's shift.  ``generation`` counts the setups.
  * ``migrate``    — once per rebuild, before the ``setup``: every owned particle whose owner (``owner_of``) is another rank
                     moves there with everything the caller keeps per particle, as rows of one int32 row table
                     (``pack_rows``); the split by owner is one HIP launch pair with one host read (``csrc/e3_migrate.hip``,
                     on CPU tensors ``migrate_rows_torch``), the counts are agreed on in one ``all_gather``, the rows travel
                     in one message per ordered pair of ranks.  Bumps ``generation`` and drops the setup state when anything
                     moved; otherwise the inputs themselves come back.
  * ``start`` / ``finish`` — once per layer: the refreshed features of the boundary particles are posted (grouped
                     isend/irecv), the interior edges' message kernel runs meanwhile, ``finish`` waits and writes the ghost
                     rows of ``h`` IN PLACE (inference only: see ``finish``), then the boundary edges run.
  * ``refresh``    — once per layer when a gradient is needed: the same exchange, blocking and OUT of place
                     (``csrc/e3_halo_grad.hip``), as an autograd node whose backward sends the ghost rows' gradients back
                     along the same entries and sums them into their owners' rows in a fixed order; ``reduce_ghosts`` does
                     that for a per-row quantity such as dE/dpos, ``all_reduce_grads`` sums parameter gradients.

The exchange above needs only the entry table and is the base class ``Halo``.  Three layouts add their geometry and selection:

  * ``SlabHalo``   — slabs along x (grid N x 1 x 1): what ``bench.py --gpus N`` uses for WEAK scaling (N unit cubes side by
                     side, 1 M particles each): a face costs r / 1 = 1.8 % ghosts per side, every rank has <= 2 neighbours.
  * ``GridHalo((2, 2, 2), ...)`` — octants of ONE box, i.e. the top level of the Morton order (each octant is one contiguous
                     Morton key range): the STRONG-scaling layout.  A unit cube cut 8 ways costs ~3 r / (1/2)
                     = 11 % ghosts per rank spread over 7 neighbours (7 xGMI links) against 2 r / (1/8) = 29 % over 2 links
                     for slabs of width 1/8; tests/test_sharding_gloo.py prints both.  Boxes are equal-VOLUME.
  * ``MortonHalo(MortonPartition(lo, hi, r, world).fit(pos))`` -- equal-COUNT Morton key ranges for a non-uniform cloud in
                     an open box.  The box is cut into a power-of-two grid of cells at least ``r`` wide, a
                     particle's key is the Morton interleave of its cell (the graph builder's fp32 ``cell_of``), and rank q
                     owns the keys in ``[s_q, s_{q+1})``; ``fit`` takes the splitters from the global key histogram (one
                     ``all_reduce``), ``s_q`` = the smallest key k with ``P * #(key < k) >= q N``.  A cell is never split,
                     so ``|n_q - N/P| < max(hist)``: every rank is within the fullest cell of the mean.  The regions are not
                     boxes; the halo has one entry per other rank (translation 0), and an owned particle p goes to rank q iff
                     q owns a cell of ``[cell(fl32(p - r)), cell(fl32(p + r))]`` on every axis.  Rounding is monotone, so
                     every p' within r of p on every axis lies in one of those cells: a rank's ghosts are a superset of what
                     its owned rows need, with the open halo's rounding contract (a pair within about one ulp of the cutoff
                     may differ; exact for dyadic inputs).  On ROCm tensors the selection is one HIP launch pair
                     (``csrc/e3_morton_halo.hip``), on CPU tensors ``select_morton_torch``, bit for bit the same.  Peers
                     with nothing to exchange cost one count message per ``setup`` and nothing per layer.  Not covered:
                     periodic boxes (``GridHalo(periodic=)`` is the route), splitting ONE over-full cell (the bound above
                     is as good as the fullest cell is small; ``max_bits`` caps the grid at 2^7 cells per axis), and
                     ``bench.py --gpus N``, which keeps its slabs.

Open box: an entry's ghosts are the owned particles in ``[blo - r, bhi + r)`` of the peer's box, bounds in the positions'
dtype, one torch mask and ONE ``nonzero`` over all entries; positions and features keep their dtypes.

Periodic boxes (``GridHalo(..., periodic=)``, per axis, as ``radius_graph(periodic=)``): an offset never leaves the grid on
a periodic axis, so with one or two boxes along it the same peer appears in several entries with different shifts, and a
rank can be its own peer.  The owner sends a particle, shifted by ``-t``, to every image box whose r-neighbourhood holds it.
``setup`` wraps the owned positions (the graph builder's formula) and the local graph is an OPEN graph over
``[wrapped owned | ghost images]``: its edge vectors are the minimum images, and ``split_graph`` / ``start`` / ``finish``
work unchanged.  Rounding contract: the sharded periodic graph has exactly the edges of ``radius_graph(periodic=True)`` over
the whole cloud when the image shifts are exact in fp32 (e.g. dyadic coordinates with a dyadic box length); otherwise a pair
within about 1 ulp of the cutoff may differ, and edge vectors agree to fp32 rounding.  On ROCm tensors the selection is one
HIP launch pair (``csrc/e3_halo.hip``); on CPU tensors (gloo rehearsal) a torch restatement of the same predicate and order
(``select_images_torch``).

Self entries are served by local copies, never by ``torch.distributed`` (world 1 needs no process group).  The others are
point-to-point traffic between adjacent boxes (``batch_isend_irecv`` = grouped ncclSend/ncclRecv on RCCL: every pair talks
over its own xGMI link; no ring, no collective over all ranks), posted per peer in tag order.  Host syncs: two per graph
build (the selection -- open: the ``nonzero``; periodic and Morton ranges: one read of the counts --, one read of the outgoing
and incoming counts), one per graph in ``split_graph`` (three edge counts), none per layer; ``MortonPartition.fit`` reads the
key histogram once.
"""
from __future__ import annotations

import ctypes
import itertools
from dataclasses import dataclass

import numpy as np
import torch
import torch.distributed as dist

from .radius_graph import periodic_mask

# neighbour offsets; the index of the RECEIVER-side offset is the P2POp tag of an entry's messages (gloo matches by tag, RCCL
# by order: the ops with one peer are posted in tag order, so both pair the entries of a peer correctly)
OFFSETS = list(itertools.product((-1, 0, 1), repeat=3))


def _f32(v) -> float:
    return float(np.float32(v))


def image_entries(dims, lo, hi, periodic, rank):
    """Halo entries of ``rank`` in a ``dims`` grid of boxes over ``[lo, hi)``: ``[(peer, d, t), ...]`` in ``OFFSETS`` order,
    ``t`` the translation (fp32 multiples of ``L_a = fl32(hi_a - lo_a)``) with ``box(peer) + t`` = the box adjacent to
    ``rank``'s at offset ``d``.  Open axes: an offset that leaves the grid has no entry.  Needs no process group."""
    dims = tuple(int(v) for v in dims)
    mask = periodic_mask(periodic, 0.0, lo, hi)
    px, py, pz = dims
    me = (rank // (py * pz), (rank // pz) % py, rank % pz)
    L = [_f32(_f32(hi[a]) - _f32(lo[a])) for a in range(3)]
    out = []
    for d in OFFSETS:
        if d == (0, 0, 0):
            continue
        c, t = [], []
        for a in range(3):
            v = me[a] + d[a]
            k = v // dims[a] if (mask >> a) & 1 else 0
            if not 0 <= v - k * dims[a] < dims[a]:
                break
            c.append(v - k * dims[a])
            t.append(_f32(k * L[a]) if k else 0.0)
        else:
            out.append(((c[0] * py + c[1]) * pz + c[2], d, tuple(t)))
    return out


def check_cutoff(dims, lo, hi, periodic, r):
    """``ValueError`` unless ``r`` <= the box width on every axis with more than one box and ``2 r < L`` on every
    periodic axis (``radius_graph.periodic_mask``)."""
    periodic_mask(periodic, r, lo, hi)
    for a in range(3):
        if int(dims[a]) > 1:
            w = (float(hi[a]) - float(lo[a])) / int(dims[a])
            if r > w:
                raise ValueError(f"cutoff {r} exceeds the box width {w} on axis {a}: ghosts would come from beyond the "
                                 f"adjacent boxes")


def _wrap_torch(pos, lo, hi, mask):
    """The graph builder's wrap (include/e3gnn.h, e3_rg_sort_count_pbc) restated in fp32 torch ops, each rounded once."""
    out = pos.clone()
    for a in range(3):
        if not (mask >> a) & 1:
            continue
        lo_a, hi_a = _f32(lo[a]), _f32(hi[a])
        L = _f32(hi_a - lo_a)
        invL = float(np.float32(1.0) / np.float32(L))
        x = pos[:, a]
        w = x - L * torch.floor((x - lo_a) * invL)
        out[:, a] = torch.where(w >= hi_a, w - L, torch.where(w < lo_a, w + L, w))
    return out


def _check_f32_pos(pos, what):
    if pos.dtype != torch.float32 or pos.dim() != 2 or pos.shape[1] != 3:
        raise TypeError(f"{what} positions must be [n,3] float32, got {tuple(pos.shape)} {pos.dtype}")


def _select_on_device(kind, what, dev, n, n_groups, count_head, fill_head, rows=(), workspace=None):
    """The two-pass device selection of ``select_images`` (``kind`` "halo") and ``select_morton`` ("morton"): workspace
    query, ``e3_<kind>_select_count(*count_head, counts, workspace ...)``, the ONE host read of the per-group counts,
    ``e3_<kind>_select_fill(*fill_head, total, idx, *more, workspace ...)`` with one ``(shape, dtype)`` in ``rows`` for every
    further per-hit output.  -> (counts (list of ``n_groups`` ints), [idx [total] int32, *more])."""
    from . import _lib
    lib = _lib.load()
    names = [f"e3_{kind}_select_{part}" for part in ("workspace_bytes", "count", "fill")]
    counts = torch.zeros(max(n_groups, 1), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        wbytes = int(getattr(lib, names[0])(n, n_groups))
        if wbytes < 0:
            raise RuntimeError(f"{names[0]}: unsupported size (n = {n}, {n_groups} {what})")
        if workspace is None or workspace.numel() < wbytes:
            workspace = torch.empty(max(wbytes, 16), dtype=torch.uint8, device=dev)
        ws = (workspace.data_ptr(), wbytes, torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(getattr(lib, names[1])(*count_head, counts.data_ptr(), *ws), names[1])
        cnt = [int(v) for v in counts[:n_groups].tolist()] if n_groups else []      # the one host read of the selection
        total = sum(cnt)
        out = [torch.empty((max(total, 1), *shape), dtype=dt, device=dev) for shape, dt in (((), torch.int32), *rows)]
        _lib.check(getattr(lib, names[2])(*fill_head, total, *[t.data_ptr() for t in out], *ws), names[2])
    return cnt, [t[:total] for t in out]


def _in_boxes(pos, elo, ehi):
    """(entry, index) of every position inside ``[elo_e, ehi_e)`` on all three axes, entry-major, then by index."""
    m = ((pos[None, :, :] >= elo[:, None, :]) & (pos[None, :, :] < ehi[:, None, :])).all(-1)   # [ne, n]
    return m.nonzero(as_tuple=True)


def select_images_torch(pos, lo, hi, periodic, r, entries):
    """Torch restatement of ``e3_halo_select_count`` / ``_fill`` (any device): -> (pos_wrapped [n,3] fp32, idx [total]
    int64, counts (list of int), ghost_pos [total,3] fp32).  ``entries``: ``[(lo3, hi3, shift3), ...]`` fp32 values."""
    mask = periodic_mask(periodic, r, lo, hi)
    _check_f32_pos(pos, "periodic halo")
    dev = pos.device
    pw = _wrap_torch(pos, lo, hi, mask)
    ne = len(entries)
    if ne == 0 or pos.shape[0] == 0:
        return pw, torch.empty(0, dtype=torch.long, device=dev), [0] * ne, torch.empty((0, 3), dtype=torch.float32, device=dev)
    elo = torch.tensor([e[0] for e in entries], dtype=torch.float32, device=dev)
    ehi = torch.tensor([e[1] for e in entries], dtype=torch.float32, device=dev)
    esh = torch.tensor([e[2] for e in entries], dtype=torch.float32, device=dev)
    ent, idx = _in_boxes(pw, elo, ehi)
    counts = [int(v) for v in torch.bincount(ent, minlength=ne).tolist()]
    return pw, idx, counts, pw[idx] + esh[ent]


def select_images(pos, lo, hi, periodic, r, entries):
    """Wrap the owned positions and select the ghost images of every entry: ``select_images_torch``'s result, bit for bit.
    ROCm tensors: the HIP pair ``e3_halo_select_count`` / ``_fill`` (one host read of the counts); CPU tensors: the torch
    restatement."""
    if not pos.is_cuda:
        return select_images_torch(pos, lo, hi, periodic, r, entries)
    from . import _lib
    mask = periodic_mask(periodic, r, lo, hi)
    _check_f32_pos(pos, "periodic halo")
    pos = pos.contiguous()
    dev, n, ne = pos.device, pos.shape[0], len(entries)
    arr = (_lib.HaloEntry * max(ne, 1))()
    for i, (elo, ehi, esh) in enumerate(entries):
        for a in range(3):
            arr[i].lo[a], arr[i].hi[a], arr[i].shift[a] = elo[a], ehi[a], esh[a]
    args = (_lib.Float3(*lo), _lib.Float3(*hi), mask, float(r), arr, ne)
    pw = torch.empty((n, 3), dtype=torch.float32, device=dev)
    cnt, (idx, ghost) = _select_on_device("halo", "entries", dev, n, ne, (pos.data_ptr(), n, *args, pw.data_ptr()),
                                          (pw.data_ptr(), n, *args), rows=[((3,), torch.float32)])
    return pw, idx.long(), cnt, ghost


# ---------------------------------------------------------------------------------------------------------------------
# migration between ranks: the row table, its split by owner (csrc/e3_migrate.hip) and the torch restatement
# ---------------------------------------------------------------------------------------------------------------------
_MIGRATE_TAG = len(OFFSETS)   # P2POp tag of a migration message: above every halo entry's tag


def _row_words(tensors):
    """Validate the per-particle tensors of a migration (positions first) -> their widths in 32-bit words."""
    n = tensors[0].shape[0] if tensors[0].dim() else -1
    words = []
    for k, t in enumerate(tensors):
        what = f"tensor {k} ({tuple(t.shape)} {t.dtype})"
        if t.requires_grad:
            raise ValueError(f"{what} requires grad: migration is outside the autograd graph (its outputs are new leaves); "
                             "pass a detached tensor")
        row_bytes = (t.shape[1] if t.dim() == 2 else 1) * t.element_size()
        if t.dim() not in (1, 2) or not t.is_contiguous() or t.is_complex() or row_bytes == 0 or row_bytes % 4:
            raise ValueError(f"{what}: a row table takes contiguous [n] or [n, k] tensors whose row is a multiple of 4 bytes")
        if t.shape[0] != n or t.device != tensors[0].device:
            raise ValueError(f"{what}: every tensor needs the {n} rows and the device of the positions")
        words.append(row_bytes // 4)
    return words


def pack_rows(pos, *rows):
    """The per-particle tensors of the caller, viewed as 32-bit words and concatenated column-wise, positions first ->
    (table int32 [n, W], layout).  Bit-exact; ``unpack_rows`` is the inverse.  Accepted: contiguous ``[n]`` or ``[n, k]``
    tensors whose row is a multiple of 4 bytes (fp32 / int32 of any ``k``, int64 / fp64 of any ``k``, fp16 / bf16 with even
    ``k``), none requiring grad; anything else is a ``ValueError`` naming the tensor's position and dtype."""
    tensors = (pos, *rows)
    words = _row_words(tensors)
    n = pos.shape[0]
    cols = []
    for t in tensors:
        t = t.detach().reshape(n, t.shape[1] if t.dim() == 2 else 1)
        try:
            cols.append(t.view(torch.int32))
        except RuntimeError:                      # a narrow dtype at an odd storage offset: the view needs 4-byte alignment
            cols.append(t.clone().view(torch.int32))
    layout = [(t.dtype, tuple(t.shape[1:]), w) for t, w in zip(tensors, words)]
    return torch.cat(cols, 1), layout


def unpack_rows(table, layout):
    """The inverse of ``pack_rows``: -> the list of per-particle tensors (new contiguous tensors, the table's bits)."""
    n, out, o = table.shape[0], [], 0
    if table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != sum(w for _, _, w in layout):
        raise ValueError(f"a row table of this layout is int32 [n, {sum(w for _, _, w in layout)}], got "
                         f"{tuple(table.shape)} {table.dtype}")
    for dtype, tail, w in layout:
        # a copy at storage offset 0 (a slice of a table of one row or none is "contiguous" where it lies)
        out.append(table[:, o:o + w].clone(memory_format=torch.contiguous_format).view(dtype).reshape(n, *tail))
        o += w
    return out


def migrate_rows_torch(table, owner, rank, world):
    """Torch restatement of ``e3_migrate_count`` / ``_fill`` (any device; the CPU twin of the kernel): the rows of ``table``
    [n, W] split by ``owner`` [n] -> (stay [n_stay, W]: the rows with ``owner == rank`` in their original order; send
    [n_leave, W]: the rows of the other ranks, grouped by destination ascending, ascending original index inside a group;
    counts [world] int64, ``counts[rank] = n_stay``; n_invalid: the rows whose owner is outside ``[0, world)``, which are in
    neither output)."""
    owner = owner.long()
    valid = (owner >= 0) & (owner < world)
    stay = table[owner == rank]
    idx = (valid & (owner != rank)).nonzero().flatten()
    send = table[idx[torch.sort(owner[idx], stable=True).indices]]
    counts = torch.bincount(owner[valid], minlength=world)[:world]
    return stay, send, counts, int(owner.numel() - int(valid.sum()))


def _migrate_count(owner, rank, world, workspace=None):
    """``e3_migrate_count`` and the ONE host read of the pack: owner int32 [n] on a ROCm device -> (the ``world + 1``
    counts, the last one the invalid owners; the workspace, for ``_migrate_fill``)."""
    from . import _lib
    lib = _lib.load()
    dev, n = owner.device, owner.numel()
    counts = torch.zeros(world + 1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        wbytes = int(lib.e3_migrate_workspace_bytes(n, world))
        if wbytes < 0:
            raise RuntimeError(f"e3_migrate_workspace_bytes: unsupported size (n = {n}, {world} ranks)")
        if workspace is None or workspace.numel() < wbytes or workspace.device != dev:
            workspace = torch.empty(max(wbytes, 16), dtype=torch.uint8, device=dev)
        _lib.check(lib.e3_migrate_count(owner.data_ptr(), n, world, rank, counts.data_ptr(), workspace.data_ptr(),
                                        workspace.numel(), torch.cuda.current_stream(dev).cuda_stream), "e3_migrate_count")
        return [int(v) for v in counts.tolist()], workspace


def _migrate_fill(table, owner, rank, world, cnt, workspace, stay):
    """``e3_migrate_fill`` after ``_migrate_count``: the stayers into ``stay`` [>= cnt[rank], W], -> send [n_leave, W]."""
    from . import _lib
    dev, (n, W) = table.device, table.shape
    n_send = sum(cnt[:world]) - cnt[rank]
    send = torch.empty((n_send, W), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().e3_migrate_fill(
            table.data_ptr(), owner.data_ptr(), n, W, world, rank, (ctypes.c_int32 * (world + 1))(*cnt), stay.shape[0], n_send,
            stay.data_ptr() if stay.shape[0] else None, send.data_ptr() if n_send else None, workspace.data_ptr(),
            workspace.numel(), torch.cuda.current_stream(dev).cuda_stream), "e3_migrate_fill")
    return send


def migrate_rows(table, owner, rank, world, workspace=None):
    """``migrate_rows_torch``'s result, bit for bit.  ROCm tensors and at most ``MORTON_MAX_RANKS`` ranks: the HIP pair
    ``e3_migrate_count`` / ``_fill`` (csrc/e3_migrate.hip; one host read of the counts); CPU tensors, or more ranks: the
    torch restatement."""
    if not table.is_cuda or world > MORTON_MAX_RANKS:
        return migrate_rows_torch(table, owner, rank, world)
    table, owner = table.contiguous(), owner.to(torch.int32).contiguous()
    cnt, workspace = _migrate_count(owner, rank, world, workspace)
    stay = torch.empty((cnt[rank], table.shape[1]), dtype=torch.int32, device=table.device)
    send = _migrate_fill(table, owner, rank, world, cnt, workspace, stay)
    return stay, send, torch.tensor(cnt[:world], dtype=torch.int64, device=table.device), cnt[world]


@dataclass
class SplitGraph:
    """Edge lists of a sharded graph, all sorted by dst (CSR order) in the graph's local (Morton) numbering."""
    graph: object                 # RadiusGraph with the edges into ghost rows removed (rowptr / src / dst consistent)
    interior: tuple               # (src int32 [Ei], dst int32 [Ei]): owned src
    boundary: tuple               # (src int32 [Eb], dst int32 [Eb]): ghost src
    dropped: int                  # edges into ghost rows that were removed


def split_graph(is_ghost, g) -> SplitGraph:
    """Drop the edges of ``g`` into the rows marked in ``is_ghost`` [N] bool (ghost or image rows) and split the rest by
    the ownership of their src (``Halo.split_graph``, ``cell_images.CellImages.split_graph``)."""
    from .radius_graph import RadiusGraph
    src, dst = g.src, g.dst
    N, E = g.rowptr.numel() - 1, int(src.numel())
    if src.is_cuda:
        # one classification + compaction on the device (csrc/e3_shard.hip); ONE host read for the three counts
        from . import _lib
        lib = _lib.load()
        dev = src.device
        ghost8 = is_ghost.to(torch.uint8)
        rowptr2 = torch.empty(N + 1, dtype=torch.int32, device=dev)
        outs = [torch.empty(max(E, 1), dtype=torch.int32, device=dev) for _ in range(6)]
        counts = torch.empty(4, dtype=torch.int32, device=dev)
        work = torch.empty(int(lib.e3_split_edges_workspace_bytes(N)), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.e3_split_edges(g.rowptr.data_ptr(), src.data_ptr(), ghost8.data_ptr(), N, E,
                                          rowptr2.data_ptr(), *[o.data_ptr() for o in outs], counts.data_ptr(),
                                          work.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "e3_split_edges")
        ek, ei, eb = (int(v) for v in counts[:3].tolist())
        g2 = RadiusGraph(g.perm, g.pos4, rowptr2, outs[0][:ek], ek, g.grid)
        object.__setattr__(g2, "_dst", outs[1][:ek])
        return SplitGraph(g2, (outs[2][:ei], outs[3][:ei]), (outs[4][:eb], outs[5][:eb]), E - ek)
    keep = ~is_ghost[dst.long()]
    src_k, dst_k = src[keep], dst[keep]
    deg = (g.rowptr[1:] - g.rowptr[:-1]).clone()
    deg[is_ghost] = 0
    rowptr = torch.zeros_like(g.rowptr)
    rowptr[1:] = torch.cumsum(deg, 0)
    g2 = RadiusGraph(g.perm, g.pos4, rowptr, src_k.contiguous(), int(src_k.numel()), g.grid)
    object.__setattr__(g2, "_dst", dst_k.contiguous())
    ghost_src = is_ghost[src_k.long()]
    interior = (src_k[~ghost_src].contiguous(), dst_k[~ghost_src].contiguous())
    boundary = (src_k[ghost_src].contiguous(), dst_k[ghost_src].contiguous())
    return SplitGraph(g2, interior, boundary, int(src.numel() - src_k.numel()))


def halo_refresh_torch(h, recv, recv_idx):
    """Torch restatement of ``e3_halo_refresh`` (any device): the ghost rows ``recv_idx`` of a copy of ``h`` <- ``recv``."""
    return h.clone().index_copy_(0, recv_idx, recv)


def halo_reduce_torch(g, back, recv_idx, send_idx):
    """Torch restatement of ``e3_halo_reduce`` (any device): ``g`` with its ghost rows zeroed, plus ``back[k]`` added to row
    ``send_idx[k]``."""
    return g.clone().index_fill_(0, recv_idx, 0).index_add_(0, send_idx, back)


def _rows(t):
    return t if t.stride(-1) == 1 or t.shape[0] == 0 else t.contiguous()


def halo_refresh(h, recv, slot, recv_idx):
    """``out[i] = slot[i] < 0 ? h[i] : recv[slot[i]]`` -> a new contiguous [n, D] tensor (``recv_idx``: the rows with a
    slot, in slot order).  ROCm tensors: ``e3_halo_refresh`` (csrc/e3_halo_grad.hip; row-strided views are read in place);
    CPU tensors: ``halo_refresh_torch``."""
    if not h.is_cuda:
        return halo_refresh_torch(h, recv, recv_idx)
    from . import _lib
    h, recv = _rows(h), _rows(recv)
    n, D = h.shape
    out = torch.empty((n, D), dtype=h.dtype, device=h.device)
    with torch.cuda.device(h.device):
        _lib.check(_lib.load().e3_halo_refresh(
            h.data_ptr(), h.stride(0), recv.data_ptr() if recv.shape[0] else None, max(recv.stride(0), D), recv.shape[0],
            slot.data_ptr(), n, D, _lib.dtype_code(h.dtype), out.data_ptr(), D,
            torch.cuda.current_stream(h.device).cuda_stream), "e3_halo_refresh")
    return out


def halo_reduce(g, back, slot, red_ptr, red_k, recv_idx, send_idx):
    """``out[i] = (slot[i] < 0 ? g[i] : 0) + sum of back[k] over the k of row i`` (``red_ptr`` / ``red_k``: ``send_idx``
    grouped by row, k ascending) -> a new contiguous [n, D] tensor.  ROCm tensors: ``e3_halo_reduce``; CPU tensors:
    ``halo_reduce_torch``."""
    if not g.is_cuda:
        return halo_reduce_torch(g, back, recv_idx, send_idx)
    from . import _lib
    g, back = _rows(g), _rows(back)
    n, D = g.shape
    out = torch.empty((n, D), dtype=g.dtype, device=g.device)
    nb = back.shape[0]
    with torch.cuda.device(g.device):
        _lib.check(_lib.load().e3_halo_reduce(
            g.data_ptr(), g.stride(0), back.data_ptr() if nb else None, max(back.stride(0), D), nb, slot.data_ptr(),
            red_ptr.data_ptr(), red_k.data_ptr() if nb else None, n, D, _lib.dtype_code(g.dtype), out.data_ptr(), D,
            torch.cuda.current_stream(g.device).cuda_stream), "e3_halo_reduce")
    return out


class _HaloRefreshFn(torch.autograd.Function):
    """``Halo.refresh``: forward = exchange + ``halo_refresh``, backward = reverse exchange + ``halo_reduce``."""

    @staticmethod
    def forward(ctx, h, anchor, halo):
        ctx.halo = halo
        return halo._forward(h)

    @staticmethod
    def backward(ctx, g):
        return ctx.halo._reverse(g), torch.zeros_like(ctx.halo.anchor), None


def all_reduce_sum(t, group=None):
    """Sum of ``t`` over the ranks of ``group`` -> a new tensor on ``t``'s device (host-staged under gloo, as the halo's
    transfers are); ``t`` itself without a process group."""
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return t
    buf = t.cpu() if t.is_cuda and dist.get_backend(group) == "gloo" else t.clone()
    dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
    return buf.to(t.device)


def all_reduce_grads(module, group=None):
    """Sum the parameter gradients of ``module`` over the ranks of ``group`` in place (one all-reduce of the flattened
    gradients; a parameter without a gradient on this rank counts as zero and gets one).  After ``loss.backward()`` on
    every rank, with the training-mode energy of ``ShardedEnergyModel`` in the loss, every rank holds dE_total/dtheta.
    Without a process group (world 1) nothing is exchanged."""
    params = [p for p in module.parameters() if p.requires_grad]
    if not params:
        return
    for p in params:
        if p.grad is None:
            p.grad = torch.zeros_like(p)
    flat = all_reduce_sum(torch.cat([p.grad.reshape(-1) for p in params]), group)
    o = 0
    for p in params:
        p.grad.copy_(flat[o:o + p.numel()].view_as(p.grad))
        o += p.numel()


def _world_rank(group):
    return (dist.get_world_size(group), dist.get_rank(group)) if dist.is_initialized() else (1, 0)


class Halo:
    """The entry-based ghost exchange every layout shares: it needs nothing but the entry table.

    ``images`` lists the halo's entries ``(peer, d, t)`` (module docstring); ``send_counts`` / ``recv_counts`` are per
    entry and ``neighbours`` is the sorted distinct peers other than this rank.  A layout supplies ``_check_cutoff(pos, r)``
    (raises before any transfer), ``owner_of(pos)`` and ``_select(pos, r)`` -> (owned positions as the local cloud holds
    them, indices sent [total], per-entry counts, positions sent), the particles grouped by entry, ascending within one."""

    periodic = 0    # axis bit mask of the axes that wrap; only a GridHalo has any

    def __init__(self, group, entries, send_tags, recv_tags):
        """``send_tags[e]`` / ``recv_tags[e]``: P2POp tag of what this rank sends for entry ``e`` / receives into it."""
        self.group = group
        self.world, self.rank = _world_rank(group)
        self.n_owned = 0
        self.generation = 0         # bumped by every ``setup``: how a ShardedNeighborList notices a foreign one
        self.bytes_last_exchange = 0
        self.anchor = None          # see ``refresh``: the leaf that keeps every refresh in a backward pass
        self._grad_maps = None
        self._build_pos = None      # the stored setup state: None before the first ``setup`` and after a ``migrate`` that moved
        # the last ``migrate``: rows sent to / received from every rank, and the particles that changed rank anywhere
        self.migrated_out, self.migrated_in, self.migrated = [0] * self.world, [0] * self.world, 0
        self._migrate_ws = None
        ent = self.images = entries
        self.neighbours = sorted({q for q, _, _ in ent if q != self.rank})
        at = {d: e for e, (_, d, _) in enumerate(ent)}
        # self entry e receives what this rank sends for its entry (me, -d)
        self._self_pairs = [(e, at[tuple(-v for v in d)]) for e, (q, d, _) in enumerate(ent) if q == self.rank]
        self._remote = [e for e, (q, _, _) in enumerate(ent) if q != self.rank]
        # per peer, in tag order
        self._send_ops = sorted((ent[e][0], send_tags[e], e) for e in self._remote)
        self._recv_ops = sorted((ent[e][0], recv_tags[e], e) for e in self._remote)

    # -- p2p helpers ----------------------------------------------------------------------------------
    def _post(self, sends, recvs, reverse=False):
        """Grouped send / recv of the remote entries (``sends[e]`` / ``recvs[e]`` by entry index), per peer in tag order;
        empty messages are skipped on both ends (the sizes were agreed on in ``setup``).  ``reverse``: the way back
        (``_reverse``) -- what entry ``e`` RECEIVED goes back to its peer under the entry's receive tag, and what was sent
        for ``e`` is answered under its send tag, so the two ends pair up exactly as they do on the way out."""
        send_ops, recv_ops = (self._recv_ops, self._send_ops) if reverse else (self._send_ops, self._recv_ops)
        ops = [dist.P2POp(dist.isend, sends[e], q, self.group, tag=tag) for q, tag, e in send_ops if sends[e].numel()]
        ops += [dist.P2POp(dist.irecv, recvs[e], q, self.group, tag=tag) for q, tag, e in recv_ops if recvs[e].numel()]
        return dist.batch_isend_irecv(ops) if ops else []

    def _gloo(self):
        return dist.get_backend(self.group) == "gloo"

    def _start(self, sends, recvs, reverse=False):
        """Serve the self entries by local copies and post the remote ones -> ``(works, staged, posted)`` for ``_wait``.
        gloo has no device transport: device tensors are staged through host memory (rehearsal mode only); ``staged`` lists
        the (device recv, host recv) pairs and ``posted`` keeps the send buffers referenced until the wait.  ``reverse``:
        ``sends[e]`` holds what entry ``e`` received and ``recvs[e]`` takes the answer to what was sent for ``e``."""
        for e, m in self._self_pairs:
            if reverse:
                recvs[m].copy_(sends[e])
            else:
                recvs[e].copy_(sends[m])
        if not self._remote:
            return [], [], sends
        staged = []
        if sends[0].is_cuda and self._gloo():
            sends = {e: sends[e].cpu() for e in self._remote}
            host = {e: torch.empty(recvs[e].shape, dtype=recvs[e].dtype) for e in self._remote}
            staged = [(recvs[e], host[e]) for e in self._remote]
            recvs = host
        return self._post(sends, recvs, reverse), staged, sends

    @staticmethod
    def _wait(works, staged, posted):
        for w in works:
            w.wait()
        for d, s in staged:
            d.copy_(s)

    # -- once per graph build -------------------------------------------------------------------------
    def setup(self, pos: torch.Tensor, feats: torch.Tensor, r: float):
        """pos [n,3], feats [n,F] of the owned particles -> (local_pos, local_feats) = ``[owned | ghosts]``, the ghosts in
        entry order (``images``).  Positions and features travel in their own dtypes (periodic: positions fp32, the owned
        ones wrapped)."""
        self._check_cutoff(pos, r)                                        # ValueError before any transfer
        dev = pos.device
        n = pos.shape[0]
        self.generation += 1
        self._build_pos = pos.detach().clone()                            # the caller's coordinates (``update_positions``)
        pos, idx, cnt, gpos = self._select(pos, r)                        # host sync #1
        self._build_local = pos                                           # ... and the owned rows of the local cloud
        self._send_shift = None
        # the counts: on the CPU for gloo, else on the device; self entries are local copies; ONE read of [out | in]
        cdev = dev if self._remote and not self._gloo() else torch.device("cpu")
        co = torch.as_tensor(cnt, dtype=torch.int64).to(cdev)
        ci = torch.zeros_like(co)
        for w in self._post(co[:, None], ci[:, None]):
            w.wait()
        both = torch.cat([co, ci]).tolist()                                # host sync #2
        ne = len(self.images)
        self.send_counts, self.recv_counts = both[:ne], both[ne:]
        for e, m in self._self_pairs:
            self.recv_counts[e] = self.send_counts[m]
        self.n_owned, self.n_ghost = n, sum(self.recv_counts)
        self.sel = idx                         # original indices of the particles sent, grouped by entry
        self._send_idx = idx
        out = []
        for t, send in ((pos, gpos), (feats, feats[idx])):
            ghosts = torch.empty((self.n_ghost, t.shape[1]), dtype=t.dtype, device=dev)
            self._wait(*self._start(list(send.split(self.send_counts)), list(ghosts.split(self.recv_counts))))
            out.append(torch.cat([t, ghosts], 0))
        self._recv_idx = torch.arange(n, n + self.n_ghost, device=dev)
        self.owned_new = torch.arange(n, device=dev)
        self._grad_maps = None                  # built by ``renumber`` (or on first use in the setup numbering)
        if self.anchor is None or self.anchor.device != dev:
            self.anchor = torch.zeros((), dtype=torch.float32, device=dev, requires_grad=True)
        return out[0], out[1]

    # -- once per step between two builds --------------------------------------------------------------
    def _check_like_build(self, pos):
        if self._build_pos is None:
            raise RuntimeError("the halo holds no setup state (none yet, or a migrate has moved particles since): call "
                               "setup first")
        if pos.shape != self._build_pos.shape or pos.device != self._build_pos.device:
            raise ValueError(f"positions {tuple(pos.shape)} on {pos.device}: the last setup saw "
                             f"{tuple(self._build_pos.shape)} on {self._build_pos.device}")

    def displacement(self, pos: torch.Tensor) -> torch.Tensor:
        """``pos`` [n,3] (the owned particles, the order of the last ``setup``) -> their displacement since that ``setup``
        [n,3]: ``d = pos - pos_at_build``, and on every periodic axis of a ``GridHalo`` its minimum image in the rint form
        of ``e3_nl_update`` (include/e3gnn.h), ``fl(d - fl(L rint(fl(d invL))))``, every fp32 operation rounded once: a
        caller that re-wraps its coordinates has not moved."""
        self._check_like_build(pos)
        d = pos - self._build_pos
        for a in range(3):
            if (self.periodic >> a) & 1:
                L = _f32(_f32(self.hi[a]) - _f32(self.lo[a]))
                invL = float(np.float32(1.0) / np.float32(L))
                d[:, a] = d[:, a] - L * torch.round(d[:, a] * invL)      # torch.round is rint (half to even)
        return d

    def update_positions(self, pos: torch.Tensor, feats: torch.Tensor | None = None, disp: torch.Tensor | None = None):
        """The local cloud of the last ``setup`` at the current positions, along the stored entries: no selection, no count
        exchange, no host read.  pos [n,3] (feats [n,F]) of the owned particles in the order ``setup`` saw -> (local_pos,
        local_feats | None) = ``[owned | ghosts]`` in ``setup``'s order.

        Owned rows hold the continuation of the build-time local coordinates: ``pos`` itself on an open axis, and on a
        periodic axis ``fl(ref + displacement)`` (``displacement``) with ``ref`` the wrapped coordinate ``setup`` returned
        -- the image of the current position nearest to where the particle was in the local cloud, so a re-wrapped
        coordinate or a particle that crosses a periodic face moves nothing discontinuously (the local cloud is an open
        graph: an owned row may leave ``[lo, hi)``).  Ghost rows hold ``fl(owner's local position + the entry's shift)``,
        the shift ``setup`` used: zero for open and Morton halos, ``-t`` for periodic images.  ``feats`` travel the same
        way, unshifted.  ``disp``: ``displacement(pos)`` when the caller has it already.  Every rank of the group calls
        it (it is an exchange); who owns what is frozen since the ``setup``."""
        self._check_like_build(pos)
        local = pos
        if self.periodic:
            d = self.displacement(pos) if disp is None else disp
            local = pos.clone()
            for a in range(3):
                if (self.periodic >> a) & 1:
                    local[:, a] = self._build_local[:, a] + d[:, a]
        send = local[self.sel]
        if any(v != 0.0 for _, _, t in self.images for v in t):
            if self._send_shift is None:
                # per sent row the shift of its entry; sizes are host integers since ``setup``: an upload, not a read
                esh = torch.tensor([[-v if v else 0.0 for v in t] for _, _, t in self.images], dtype=local.dtype)
                self._send_shift = esh.repeat_interleave(torch.tensor(self.send_counts), 0).to(local.device)
            send = send + self._send_shift
        out = []
        for t, snd in ((local, send),) + (() if feats is None else ((feats, feats[self.sel]),)):
            ghosts = torch.empty((self.n_ghost, t.shape[1]), dtype=t.dtype, device=t.device)
            self._wait(*self._start(list(snd.split(self.send_counts)), list(ghosts.split(self.recv_counts))))
            out.append(torch.cat([t, ghosts], 0))
        return out[0], (out[1] if feats is not None else None)

    # -- once per rebuild, before the setup: particles that changed owner change rank -------------------
    def migrate(self, pos: torch.Tensor, *rows: torch.Tensor):
        """Move every owned particle whose owner (``owner_of``) is another rank to that rank, with everything the caller
        keeps per particle: pos [n,3] and any number of ``rows`` ([n] or [n, k], ``pack_rows``) -> ``(pos, *rows)`` of the
        particles this rank owns now.  A collective: every rank of the group calls it with the same number of ``rows`` and
        the same row widths.

        Ownership is computed on the caller's coordinates (periodic axes may be unwrapped: ``owner_of`` wraps) and the
        positions travel as the caller's bits.  Order of the result: the stayers in their original relative order, then
        the arrivals by source rank ascending, each in the sender's original order.  The split is one device pack
        (``e3_migrate_count``, ONE host read of the counts, ``e3_migrate_fill``; ``migrate_rows_torch`` on CPU tensors and
        above ``MORTON_MAX_RANKS`` ranks), the counts are agreed on in one ``all_gather`` (host-staged under gloo), the rows
        travel in one message per ordered pair of ranks with a non-zero count, straight into the new table.

        Nobody moved on any rank: the inputs themselves come back, ``generation`` and the setup state stay.  Otherwise
        ``generation`` is bumped (a ``ShardedNeighborList`` rebuilds) and the setup state is dropped: ``displacement`` and
        ``update_positions`` raise until the next ``setup``.  A position that is not finite has no owner: EVERY rank raises
        ``ValueError`` before any row is sent.  ``migrated_out[q]`` / ``migrated_in[q]``: rows sent to / received from rank
        ``q``; ``migrated``: the particles that changed rank anywhere.

        Re-balancing a ``MortonHalo`` is ``halo.partition.fit(pos, halo.group)`` followed by ``halo.migrate(...)``: the
        splitters are read when they are used.  Outside the autograd graph: the outputs are new leaves."""
        world, rank = self.world, self.rank
        tensors = (pos, *rows)
        _row_words(tensors)                                               # ValueError before any collective
        if pos.dim() != 2 or pos.shape[1] != 3:
            raise ValueError(f"positions must be [n,3], got {tuple(pos.shape)}")
        dev = pos.device
        owner = self.owner_of(pos)
        owner = torch.where(torch.isfinite(pos).all(1), owner, torch.full_like(owner, -1)).to(torch.int32)
        on_device = pos.is_cuda and world <= MORTON_MAX_RANKS
        if on_device:
            cnt, self._migrate_ws = _migrate_count(owner, rank, world, self._migrate_ws)   # the one host read of the pack
        else:
            valid = (owner >= 0) & (owner < world)
            cnt = torch.bincount(owner[valid].long(), minlength=world)[:world].tolist()
            cnt.append(pos.shape[0] - sum(cnt))
        # every rank's count row: who sends how many to whom, and whether anybody had a row without an owner
        matrix = [cnt]
        if world > 1:
            cdev = torch.device("cpu") if self._gloo() else dev
            gathered = [torch.empty(world + 1, dtype=torch.int64, device=cdev) for _ in range(world)]
            dist.all_gather(gathered, torch.tensor(cnt, dtype=torch.int64, device=cdev), group=self.group)
            matrix = torch.stack(gathered).tolist()
        n_bad = sum(row[world] for row in matrix)
        if n_bad:
            raise ValueError(f"Halo.migrate: {n_bad} particle(s) have no owner among the {world} rank(s) (a position is not "
                             "finite?): nothing was moved")
        others = [q for q in range(world) if q != rank]
        self.migrated_out = [0 if q == rank else cnt[q] for q in range(world)]
        self.migrated_in = [0 if q == rank else matrix[q][rank] for q in range(world)]
        self.migrated = sum(matrix[p][q] for p in range(world) for q in range(world) if p != q)
        if not self.migrated:
            return tensors
        table, layout = pack_rows(*tensors)
        n_stay, n_in = cnt[rank], sum(self.migrated_in)
        new = torch.empty((n_stay + n_in, table.shape[1]), dtype=torch.int32, device=dev)
        if on_device:
            send = _migrate_fill(table, owner, rank, world, cnt, self._migrate_ws, new[:n_stay])
        else:
            stay, send, _, _ = migrate_rows_torch(table, owner, rank, world)
            new[:n_stay] = stay
        sends = list(send.split([cnt[q] for q in others]))
        recvs = list(new[n_stay:].split([matrix[q][rank] for q in others]))
        staged = []
        if pos.is_cuda and self._gloo():                                  # gloo has no device transport (``_start``)
            sends = [t.cpu() for t in sends]
            host = [torch.empty(t.shape, dtype=t.dtype) for t in recvs]
            staged, recvs = list(zip(recvs, host)), host
        ops = [dist.P2POp(dist.isend, t, q, self.group, tag=_MIGRATE_TAG) for q, t in zip(others, sends) if t.numel()]
        ops += [dist.P2POp(dist.irecv, t, q, self.group, tag=_MIGRATE_TAG) for q, t in zip(others, recvs) if t.numel()]
        self._wait(dist.batch_isend_irecv(ops) if ops else [], staged, sends)
        self.generation += 1
        self._build_pos = self._build_local = None
        return tuple(unpack_rows(new, layout))

    def renumber(self, perm: torch.Tensor):
        """The graph builder renumbers the local cloud (``perm[new] = old``): translate the halo index lists."""
        inv = torch.empty_like(perm, dtype=torch.long)
        inv[perm.long()] = torch.arange(perm.numel(), device=perm.device)
        n = self.n_owned
        self._send_idx = inv[self.sel]
        self._recv_idx = inv[n:n + self.n_ghost]   # new ids of the ghosts, arrival order
        self.owned_new = inv[:n]                    # new ids of the owned particles, in their original order
        self.is_ghost = torch.zeros(perm.numel(), dtype=torch.bool, device=perm.device)
        self.is_ghost[self._recv_idx] = True
        self._grad_maps = self._build_grad_maps(perm.numel())
        return self

    def _build_grad_maps(self, n_local):
        """Index maps of ``refresh`` / ``reduce_ghosts`` in the current numbering (once per graph build) -> (slot [n_local]
        int32: -1 for an owned row, else the row's position in the received buffer; red_ptr [n_local + 1], red_k [total
        sent] int32: the send list grouped by its target row, positions ascending inside a row)."""
        dev = self._recv_idx.device
        slot = torch.full((n_local,), -1, dtype=torch.int32, device=dev)
        slot[self._recv_idx] = torch.arange(self.n_ghost, dtype=torch.int32, device=dev)
        red_k = torch.sort(self._send_idx, stable=True).indices.to(torch.int32)
        red_ptr = torch.zeros(n_local + 1, dtype=torch.int32, device=dev)
        red_ptr[1:] = torch.cumsum(torch.bincount(self._send_idx, minlength=n_local), 0)
        return slot, red_ptr, red_k

    def _maps(self):
        if self._grad_maps is None:
            self._grad_maps = self._build_grad_maps(self.n_owned + self.n_ghost)
        return self._grad_maps

    def ghost_fraction(self) -> float:
        return self.n_ghost / max(1, self.n_owned)

    def split_graph(self, g) -> SplitGraph:
        """Drop the edges into ghost rows and split the rest by the ownership of their src (see the module docstring).
        ``g``: the RadiusGraph of the local cloud (after ``renumber(g.perm)``)."""
        return split_graph(self.is_ghost, g)

    # -- once per layer -------------------------------------------------------------------------------
    def start(self, h: torch.Tensor):
        """Post this layer's ghost refresh (boundary rows of ``h`` to the neighbours) and return a token for ``finish``.
        Kernels launched between the two calls overlap the transfer as long as they do not read ghost rows."""
        D = h.shape[1]
        recv = torch.empty((self.n_ghost, D), dtype=h.dtype, device=h.device)
        send = h[self._send_idx].contiguous()
        # self entries are local copies, not exchanged bytes
        self.bytes_last_exchange = sum(self.send_counts[e] for e in self._remote) * D * h.element_size()
        return recv, self._start(list(send.split(self.send_counts)), list(recv.split(self.recv_counts)))

    def finish(self, h: torch.Tensor, token) -> torch.Tensor:
        """Wait for the transfer and write the ghost rows of ``h`` in place (one indexed copy, no clone of ``h``).
        Inference only: a tensor autograd has saved for backward must not be overwritten."""
        if torch.is_grad_enabled() and h.requires_grad:
            raise RuntimeError("the halo refresh writes ghost rows in place: not differentiable (run under torch.no_grad())")
        recv, pending = token
        self._wait(*pending)
        if recv.shape[0]:
            h.index_copy_(0, self._recv_idx, recv)
        return h

    def exchange(self, h: torch.Tensor) -> torch.Tensor:
        """Blocking form: overwrite the ghost rows of ``h`` (local numbering) with the owners' current values, in place."""
        return self.finish(h, self.start(h))

    def ghost_rows(self) -> torch.Tensor:
        """Local (graph-order) ids of the ghost rows."""
        return self._recv_idx

    # -- once per layer, differentiable ---------------------------------------------------------------
    def _forward(self, h: torch.Tensor) -> torch.Tensor:
        """The blocking refresh, out of place: the owners' current rows arrive as in ``start`` and ONE pass writes
        ``[owned rows of h | received rows]`` (``halo_refresh``); ``h`` is not written, its ghost rows are not read."""
        recv = torch.empty((self.n_ghost, h.shape[1]), dtype=h.dtype, device=h.device)
        send = h[self._send_idx]
        self.bytes_last_exchange = sum(self.send_counts[e] for e in self._remote) * h.shape[1] * h.element_size()
        self._wait(*self._start(list(send.split(self.send_counts)), list(recv.split(self.recv_counts))))
        return halo_refresh(h, recv, self._maps()[0], self._recv_idx)

    def _reverse(self, t: torch.Tensor) -> torch.Tensor:
        """The transpose of the refresh: the ghost rows of ``t`` [n_local, C] travel back along the entries they came by
        (every receive list is a send and vice versa, same tags, empty messages skipped on both ends, self entries by
        local copies) and are summed into their owners' rows (``halo_reduce``) -> [n_local, C], ghost rows zero."""
        back = torch.empty((self._send_idx.numel(), t.shape[1]), dtype=t.dtype, device=t.device)
        ghosts = t[self._recv_idx]
        self._wait(*self._start(list(ghosts.split(self.recv_counts)), list(back.split(self.send_counts)), reverse=True))
        return halo_reduce(t, back, *self._maps(), self._recv_idx, self._send_idx)

    def refresh(self, h: torch.Tensor) -> torch.Tensor:
        """Differentiable ghost refresh: -> a new ``[n_local, D]`` tensor, the owned rows of ``h`` and the owners' current
        values in the ghost rows (``exchange`` out of place).  fp32 or fp64.  Backward: the ghost rows of the incoming
        gradient go back to their owners (``_reverse``) and are added to the owned rows' own gradient, in a fixed order.
        First order only.

        Every rank has to run the backward of every refresh exactly once per backward pass -- its peers wait for the
        messages -- whatever the rank owns.  Autograd runs a node only if it lies between the differentiated output and
        one of the requested ``inputs``; so every refresh also takes ``halo.anchor``, a 0-d leaf that requires grad (its
        gradient is zero): the output always requires grad, and a caller of ``torch.autograd.grad(..., inputs=...)``
        puts ``halo.anchor`` among the inputs (``ShardedEnergyModel`` does).  ``backward()`` without ``inputs`` needs
        nothing.  The result must be USED by what is differentiated on every rank -- an empty sum over no owned rows
        counts -- and the halo must not be set up again between the forward and the backward."""
        if h.dtype not in (torch.float32, torch.float64):
            raise RuntimeError(f"the differentiable refresh is fp32 / fp64, got {h.dtype}")
        return _HaloRefreshFn.apply(h, self.anchor, self)

    def reduce_ghosts(self, t: torch.Tensor) -> torch.Tensor:
        """``t`` [n_local, C] in graph order (e.g. dE/dpos of the local cloud, C = 3: an image's position is its owner's
        plus a constant, so the Jacobian is the identity) -> [n_owned, C] in the caller's owned order: every owned row's
        own value plus the values of all its ghost copies on all ranks.  A collective of the halo: every rank calls it,
        in the same order relative to other exchanges (it is not an autograd node: call it after ``autograd.grad``)."""
        if t.dtype not in (torch.float32, torch.float64):
            raise RuntimeError(f"reduce_ghosts is fp32 / fp64, got {t.dtype}")
        return self._reverse(t.detach().contiguous())[self.owned_new]


class GridHalo(Halo):
    """Ghost-cell halo of a ``dims = (px, py, pz)`` grid of equal boxes covering ``[lo, hi)``; rank = (ix py + iy) pz + iz.

    ``periodic`` (bool or 3 bools, validated by ``radius_graph.periodic_mask``): those axes wrap at ``[lo, hi)``; positions
    must then be fp32, and ``setup`` returns the owned ones wrapped.  Works without a process group at world 1 (dims
    (1, 1, 1) with periodic axes: a pure self-halo)."""

    def __init__(self, dims, lo, hi, group=None, periodic=False):
        world, rank = _world_rank(group)
        self.dims = tuple(int(d) for d in dims)
        if self.dims[0] * self.dims[1] * self.dims[2] != world:
            raise ValueError(f"grid {self.dims} needs {self.dims[0] * self.dims[1] * self.dims[2]} ranks, the group has {world}")
        self.lo = [float(v) for v in lo]
        self.hi = [float(v) for v in hi]
        self.periodic = periodic_mask(periodic, 0.0, self.lo, self.hi)   # axis bit mask; 0 = open box
        self._axes = tuple(bool((self.periodic >> a) & 1) for a in range(3))
        ent = image_entries(self.dims, self.lo, self.hi, self._axes, rank)
        # tag = index of the RECEIVER-side offset: -d for what I send, d for what I receive
        super().__init__(group, ent, [OFFSETS.index(tuple(-v for v in d)) for _, d, _ in ent],
                         [OFFSETS.index(d) for _, d, _ in ent])

    def coords(self, rank):
        px, py, pz = self.dims
        return rank // (py * pz), (rank // pz) % py, rank % pz

    def box(self, rank):
        c = self.coords(rank)
        w = [(self.hi[a] - self.lo[a]) / self.dims[a] for a in range(3)]
        return [self.lo[a] + c[a] * w[a] for a in range(3)], [self.lo[a] + (c[a] + 1) * w[a] for a in range(3)]

    def owner_of(self, pos: torch.Tensor) -> torch.Tensor:
        """Rank that owns each position (positions outside [lo, hi) are clamped into the edge boxes; periodic axes: the
        positions are wrapped first, in fp32, as ``setup`` wraps them)."""
        if self.periodic:
            pos = _wrap_torch(pos.float(), self.lo, self.hi, self.periodic)
        idx = []
        for a in range(3):
            w = (self.hi[a] - self.lo[a]) / self.dims[a]
            idx.append(((pos[:, a] - self.lo[a]) / w).floor().long().clamp_(0, self.dims[a] - 1))
        return (idx[0] * self.dims[1] + idx[1]) * self.dims[2] + idx[2]

    def _selection(self, r):
        """fp32 selection bounds and shift of every entry, sender side: the owned particles in ``[blo + t - r, bhi + t + r)``
        of the peer's box go to it, at ``p - t``."""
        out = []
        for q, _, t in self.images:
            blo, bhi = self.box(q)
            out.append(([_f32(blo[a] + t[a] - r) for a in range(3)], [_f32(bhi[a] + t[a] + r) for a in range(3)],
                        [-t[a] if t[a] else 0.0 for a in range(3)]))
        return out

    def _select(self, pos, r):
        if self.periodic:
            return select_images(pos, self.lo, self.hi, self._axes, r, self._selection(r))
        if not self.images:
            return pos, torch.empty(0, dtype=torch.long, device=pos.device), [], pos[:0]
        # bounds in pos.dtype: per axis a superset of the r-ball
        blo = torch.tensor([self.box(q)[0] for q, _, _ in self.images], dtype=pos.dtype, device=pos.device)
        bhi = torch.tensor([self.box(q)[1] for q, _, _ in self.images], dtype=pos.dtype, device=pos.device)
        ent, idx = _in_boxes(pos, blo - r, bhi + r)
        return pos, idx, torch.bincount(ent, minlength=len(self.images)), pos[idx]

    def _check_cutoff(self, pos, r):
        check_cutoff(self.dims, self.lo, self.hi, self._axes, r)

    def local_bounds(self, r):
        """Box for the local ``radius_graph`` call: this rank's box widened by ``2 r`` (it holds the ghosts and images)."""
        blo, bhi = self.box(self.rank)
        return [v - 2 * r for v in blo], [v + 2 * r for v in bhi]


class SlabHalo(GridHalo):
    """Slabs along x: rank k owns ``x in [slab_lo, slab_hi)`` (given at ``setup``), unbounded in y and z."""

    def __init__(self, group=None):
        world = _world_rank(group)[0]
        super().__init__((world, 1, 1), (0.0, -1e30, -1e30), (float(world), 1e30, 1e30), group)
        self.left = self.rank - 1 if self.rank > 0 else None
        self.right = self.rank + 1 if self.rank < self.world - 1 else None

    def setup(self, pos, feats, slab_lo: float, slab_hi: float, r: float):
        w = float(slab_hi) - float(slab_lo)
        self.lo[0] = float(slab_lo) - self.rank * w
        self.hi[0] = self.lo[0] + self.world * w
        out = super().setup(pos, feats, r)
        by = {d: c for (_, d, _), c in zip(self.images, self.recv_counts)}
        self.n_ghost_left, self.n_ghost_right = by.get((-1, 0, 0), 0), by.get((1, 0, 0), 0)
        return out

    def migrate(self, pos, *rows):
        raise NotImplementedError("SlabHalo has no bounds until setup, so it has no owner to migrate to: use a GridHalo "
                                  "(world, 1, 1) over the whole domain")


# ---------------------------------------------------------------------------------------------------------------------
# equal-COUNT Morton key ranges (open boxes): MortonPartition (ownership) + MortonHalo (ghosts of regions that are not boxes)
# ---------------------------------------------------------------------------------------------------------------------
MORTON_MAX_RANKS = 64     # E3_MORTON_MAX_RANKS of include/e3gnn.h: the destinations of a particle are one 64-bit mask


def _spread3(v: torch.Tensor) -> torch.Tensor:
    """csrc/e3_common.h ``spread3`` on an integer tensor: 10 bits -> every third bit."""
    v = v & 0x3FF
    v = (v | (v << 16)) & 0x030000FF
    v = (v | (v << 8)) & 0x0300F00F
    v = (v | (v << 4)) & 0x030C30C3
    v = (v | (v << 2)) & 0x09249249
    return v


def _compact3(v: np.ndarray) -> np.ndarray:
    v = v & 0x09249249
    v = (v | (v >> 2)) & 0x030C30C3
    v = (v | (v >> 4)) & 0x0300F00F
    v = (v | (v >> 8)) & 0x030000FF
    v = (v | (v >> 16)) & 0x3FF
    return v


def _cells_torch(x, lo_a, inv_a, n_a):
    """The graph builder's ``cell_of`` of one fp32 coordinate column, each operation rounded once -> int64."""
    return torch.floor((x - lo_a) * inv_a).clamp_(0, n_a - 1).long()


def _morton_grid_args(lo, hi, n_cells):
    lo32, hi32 = [_f32(v) for v in lo], [_f32(v) for v in hi]
    L = [_f32(np.float32(hi32[a]) - np.float32(lo32[a])) for a in range(3)]
    inv = [float(np.float32(n_cells[a]) / np.float32(L[a])) for a in range(3)]
    return lo32, hi32, inv


def morton_keys_torch(pos, lo, hi, n_cells):
    """Torch restatement of ``e3_morton_keys`` (any device): Morton cell key of every fp32 position -> int64 [n]."""
    _check_f32_pos(pos, "Morton partition")
    lo32, _, inv = _morton_grid_args(lo, hi, n_cells)
    c = [_cells_torch(pos[:, a], lo32[a], inv[a], int(n_cells[a])) for a in range(3)]
    return _spread3(c[0]) | (_spread3(c[1]) << 1) | (_spread3(c[2]) << 2)


def morton_keys(pos, lo, hi, n_cells):
    """``morton_keys_torch``'s result, bit for bit; ROCm tensors: the HIP kernel ``e3_morton_keys``."""
    if not pos.is_cuda:
        return morton_keys_torch(pos, lo, hi, n_cells)
    from . import _lib
    _check_f32_pos(pos, "Morton partition")
    lib = _lib.load()
    pos = pos.contiguous()
    n = pos.shape[0]
    keys = torch.empty(n, dtype=torch.int32, device=pos.device)
    with torch.cuda.device(pos.device):
        _lib.check(lib.e3_morton_keys(pos.data_ptr(), n, _lib.Float3(*lo), _lib.Float3(*hi), _lib.Int3(*n_cells),
                                      keys.data_ptr(), torch.cuda.current_stream(pos.device).cuda_stream), "e3_morton_keys")
    return keys.long()


def select_morton_torch(pos, lo, hi, n_cells, r, splitters, self_rank):
    """Torch restatement of ``e3_morton_select_count`` / ``_fill`` (any device): -> (idx [total] int64, counts (list of
    ``len(splitters) - 1`` ints)).  Owned particle ``p`` goes to rank ``q != self_rank`` iff ``q`` owns a cell of
    ``[cell(fl32(p - r)), cell(fl32(p + r))]`` on every axis; grouped by rank, ascending ids inside a group."""
    _check_f32_pos(pos, "Morton halo")
    P = len(splitters) - 1
    dev, n = pos.device, pos.shape[0]
    if n == 0 or P == 1:
        return torch.empty(0, dtype=torch.long, device=dev), [0] * P
    lo32, _, inv = _morton_grid_args(lo, hi, n_cells)
    r32 = _f32(r)
    c0 = [_cells_torch(pos[:, a] - r32, lo32[a], inv[a], int(n_cells[a])) for a in range(3)]
    c1 = [_cells_torch(pos[:, a] + r32, lo32[a], inv[a], int(n_cells[a])) for a in range(3)]
    span = torch.stack([(c1[a] - c0[a]).max() for a in range(3)]).tolist()      # <= 2 (3 under adverse rounding) per axis
    inner = torch.as_tensor(list(splitters[1:P]), dtype=torch.long, device=dev)
    ids = torch.arange(n, device=dev)
    mask = torch.zeros((P, n), dtype=torch.bool, device=dev)
    for dz in range(span[2] + 1):
        for dy in range(span[1] + 1):
            for dx in range(span[0] + 1):
                x, y, z = c0[0] + dx, c0[1] + dy, c0[2] + dz
                ok = (x <= c1[0]) & (y <= c1[1]) & (z <= c1[2])
                key = _spread3(x) | (_spread3(y) << 1) | (_spread3(z) << 2)
                owner = torch.searchsorted(inner, key, right=True)
                mask[owner[ok], ids[ok]] = True
    mask[self_rank] = False
    dest, idx = mask.nonzero(as_tuple=True)
    return idx, [int(v) for v in torch.bincount(dest, minlength=P).tolist()]


def select_morton(pos, lo, hi, n_cells, r, splitters, self_rank, workspace=None):
    """``select_morton_torch``'s result, bit for bit.  ROCm tensors: the HIP pair ``e3_morton_select_count`` / ``_fill``
    (csrc/e3_morton_halo.hip; one host read of the counts); CPU tensors: the torch restatement.  ``workspace``: an optional
    uint8 device tensor of at least ``e3_morton_select_workspace_bytes`` bytes to reuse."""
    if not pos.is_cuda:
        return select_morton_torch(pos, lo, hi, n_cells, r, splitters, self_rank)
    from . import _lib
    _check_f32_pos(pos, "Morton halo")
    pos = pos.contiguous()
    n, P = pos.shape[0], len(splitters) - 1
    spl = (ctypes.c_int32 * (P + 1))(*[int(v) for v in splitters])
    args = (_lib.Float3(*lo), _lib.Float3(*hi), _lib.Int3(*[int(v) for v in n_cells]), float(r), spl, P, int(self_rank))
    head = (pos.data_ptr(), n, *args)
    cnt, (idx,) = _select_on_device("morton", "ranks", pos.device, n, P, head, head, workspace=workspace)
    return idx.long(), cnt


class MortonPartition:
    """Equal-count ownership of a non-uniform cloud in the open box ``[lo, hi)``: the box is cut into ``grid = (nx, ny, nz)``
    cells, per axis the largest power of two with ``n_a r <= L_a`` (``L_a = fl32(hi_a - lo_a)``: a cell is never narrower
    than ``r``) and ``n_a <= 2**max_bits``; a particle's cell is the graph builder's (``cell_of``, fp32), its key the Morton
    interleave of the cell, and rank ``q`` owns the keys in ``[splitters[q], splitters[q + 1])``.  ``fit`` chooses the
    splitters from the global key histogram: ``s_q`` = the smallest key ``k`` with ``P * #(key < k) >= q N``.  A cell is never
    split between ranks, so every rank's count is within the fullest cell of ``N / P``: ``|n_q - N/P| < max(hist)``.
    Equal neighbours in ``splitters`` are legal (that rank owns nothing)."""

    def __init__(self, lo, hi, r, world, max_bits=6, periodic=False):
        if periodic_mask(periodic, 0.0, [float(v) for v in lo], [float(v) for v in hi]):
            raise NotImplementedError("Morton key ranges cover open boxes only; periodic boxes are sharded by "
                                      "GridHalo(periodic=)")
        self.world = int(world)
        if not 1 <= self.world <= MORTON_MAX_RANKS:
            raise ValueError(f"MortonPartition supports 1..{MORTON_MAX_RANKS} ranks, got {world}")
        if not 0 <= int(max_bits) <= 7:
            raise ValueError(f"max_bits must be in [0, 7], got {max_bits}")
        self.r = float(r)
        if not (np.isfinite(self.r) and self.r > 0.0):
            raise ValueError(f"cutoff must be positive and finite, got {r}")
        self.lo, self.hi = [_f32(v) for v in lo], [_f32(v) for v in hi]
        grid = []
        for a in range(3):
            L = np.float32(self.hi[a]) - np.float32(self.lo[a])
            if not (np.isfinite(self.lo[a]) and np.isfinite(self.hi[a]) and np.isfinite(L) and L > 0):
                raise ValueError(f"box [{lo[a]}, {hi[a]}) on axis {a} is empty or not finite")
            n = 1
            # L / n is exact for a power of two, so this is n r <= L without rounding
            while 2 * n <= 2 ** int(max_bits) and L / np.float32(2 * n) >= np.float32(self.r):
                n *= 2
            grid.append(n)
        self.grid = tuple(grid)
        self.bits = max(n.bit_length() - 1 for n in grid)
        self.n_keys = 8 ** self.bits
        self.splitters = None
        self.counts = None
        self.hist_max = 0

    def cell_width(self, a):
        return float(np.float32(np.float32(self.hi[a]) - np.float32(self.lo[a])) / np.float32(self.grid[a]))

    def keys(self, pos: torch.Tensor) -> torch.Tensor:
        """Morton cell key of every position (int64 [n]; ROCm tensors: ``e3_morton_keys``)."""
        return morton_keys(pos, self.lo, self.hi, self.grid)

    def fit(self, pos_owned: torch.Tensor, group=None):
        """Choose the splitters from the particles this process holds (any subset; with a process group the histograms of
        all ranks are summed, host-staged under gloo as the halo's transfers are).  One host read.  -> self."""
        hist = torch.bincount(self.keys(pos_owned), minlength=self.n_keys)
        hist = all_reduce_sum(hist, group).cpu()
        P, N = self.world, int(hist.sum())
        below = torch.zeros(self.n_keys + 1, dtype=torch.int64)             # below[k] = number of particles with key < k
        below[1:] = torch.cumsum(hist, 0)
        s = torch.searchsorted(below * P, torch.arange(1, P, dtype=torch.int64) * N)   # smallest k: P below[k] >= q N
        self.splitters = [0] + [int(v) for v in s.tolist()] + [self.n_keys]
        self.counts = [int(below[self.splitters[q + 1]] - below[self.splitters[q]]) for q in range(P)]
        self.hist_max = int(hist.max())
        return self

    def _fitted(self):
        if self.splitters is None:
            raise RuntimeError("MortonPartition.fit has not been called")

    def owner_of(self, pos: torch.Tensor) -> torch.Tensor:
        """Rank that owns each position (positions outside the box are clamped into the edge cells)."""
        self._fitted()
        inner = torch.as_tensor(self.splitters[1:self.world], dtype=torch.long, device=pos.device)
        return torch.searchsorted(inner, self.keys(pos), right=True)

    def owned_cell_bounds(self, rank):
        """Bounding box of the cells ``rank`` owns -> (lo3, hi3), or None when it owns no cell of the grid."""
        self._fitted()
        k = np.arange(self.splitters[rank], self.splitters[rank + 1], dtype=np.int64)
        c = np.stack([_compact3(k >> a) for a in range(3)], 1)
        c = c[(c < np.asarray(self.grid)).all(1)]
        if not len(c):
            return None
        w = [self.cell_width(a) for a in range(3)]
        return ([self.lo[a] + int(c[:, a].min()) * w[a] for a in range(3)],
                [self.lo[a] + (int(c[:, a].max()) + 1) * w[a] for a in range(3)])


class MortonHalo(Halo):
    """Ghost halo of a fitted ``MortonPartition``: one entry per other rank, in ascending rank order, translation 0.  An
    owned particle is sent to every rank that owns a cell of ``[cell(p - r), cell(p + r)]`` (``select_morton``): cells are
    at least ``r`` wide and rounding is monotone, so a rank's ghosts are a superset of what its owned rows need.  After
    ``setup`` everything is ``Halo``'s code; ``neighbours`` then lists the peers with a non-zero count in either
    direction, and a peer with nothing to exchange costs one count message per ``setup`` and nothing per layer."""

    def __init__(self, partition: MortonPartition, group=None):
        partition._fitted()
        self.partition = partition
        world, rank = _world_rank(group)
        if partition.world != world:
            raise ValueError(f"the partition was made for {partition.world} ranks, the group has {world}")
        self.lo, self.hi = list(partition.lo), list(partition.hi)
        ent = [(q, (0, 0, 0), (0.0, 0.0, 0.0)) for q in range(world) if q != rank]
        super().__init__(group, ent, [0] * len(ent), [0] * len(ent))     # one message per peer and direction: tag 0

    def _check_cutoff(self, pos, r):
        _check_f32_pos(pos, "Morton halo")
        part = self.partition
        if not (np.isfinite(r) and r > 0.0):
            raise ValueError(f"cutoff must be positive and finite, got {r}")
        for a in range(3):
            if part.grid[a] > 1 and np.float32(r) > np.float32(part.cell_width(a)):
                raise ValueError(f"cutoff {r} exceeds the cell width {part.cell_width(a)} of the Morton partition on axis "
                                 f"{a}: ghosts would come from beyond the adjacent cells")

    def _select(self, pos, r):
        part = self.partition
        idx, cnt = select_morton(pos, part.lo, part.hi, part.grid, r, part.splitters, self.rank)
        cnt = [c for q, c in enumerate(cnt) if q != self.rank]
        return pos, idx, cnt, pos[idx]

    def setup(self, pos: torch.Tensor, feats: torch.Tensor, r: float):
        """``Halo.setup`` with the Morton selection: fp32 positions (``TypeError`` otherwise), features of any dtype;
        ``ValueError`` when ``r`` exceeds the partition's cell width on an axis with more than one cell."""
        out = super().setup(pos, feats, r)
        self.neighbours = [q for (q, _, _), s, c in zip(self.images, self.send_counts, self.recv_counts) if s or c]
        return out

    def local_bounds(self, r):
        """Box for the local ``radius_graph`` call: the bounding box of the owned cells widened by ``2 r`` (a rank that owns
        no cell: the whole domain)."""
        b = self.partition.owned_cell_bounds(self.rank)
        if b is None:
            return list(self.lo), list(self.hi)
        return [v - 2 * r for v in b[0]], [v + 2 * r for v in b[1]]

    def owner_of(self, pos: torch.Tensor) -> torch.Tensor:
        return self.partition.owner_of(pos)

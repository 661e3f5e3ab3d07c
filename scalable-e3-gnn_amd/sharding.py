"""Spatial sharding of the point cloud across GPUs (one process per GPU, RCCL over xGMI).

Builder-defined (the reference has no distributed code).  The domain is cut into a grid of axis-aligned
boxes, one per rank (``GridHalo``); a node's messages need neighbours within the cutoff ``r``, so each rank also holds
*ghost* copies of the particles of the (up to 26) adjacent boxes that lie within ``r`` of its own box:

  * ``setup``      — once per graph build: boundary particles (positions + input features) go to the adjacent boxes; the
                     local cloud is ``[owned | ghosts from neighbour 0 | ghosts from neighbour 1 | ...]``.
  * ``split_graph``— once per graph build: edges INTO ghost rows are dropped (their sums would be thrown away), the rest is
                     split into *interior* edges (owned src: computable before the layer's exchange has landed) and
                     *boundary* edges (ghost src).  On a GPU one HIP launch pair classifies and compacts (``e3_split_edges``).
  * ``start`` / ``finish`` — once per layer: the refreshed features of the boundary particles are posted (grouped
                     isend/irecv), the interior edges' message kernel runs meanwhile, ``finish`` waits and writes the ghost
                     rows of ``h`` IN PLACE (inference only: see ``finish``), then the boundary edges run.

Two layouts are built on it:

  * ``SlabHalo``   — slabs along x (grid N x 1 x 1): what ``bench.py --gpus N`` uses for WEAK scaling (N unit cubes side by
                     side, 1 M particles each): a face costs r / 1 = 1.8 % ghosts per side, every rank has <= 2 neighbours.
  * ``GridHalo((2, 2, 2), ...)`` — octants of ONE box, i.e. the top level of the Morton order (each octant is one contiguous
                     Morton key range): the STRONG-scaling layout.  A unit cube cut 8 ways costs ~3 r / (1/2)
                     = 11 % ghosts per rank spread over 7 neighbours (7 xGMI links) against 2 r / (1/8) = 29 % over 2 links
                     for slabs of width 1/8; tests/test_sharding_gloo.py prints both.  (Equal-COUNT Morton ranges for a
                     non-uniform cloud are not implemented: boxes are equal-volume.)

Periodic boxes (``GridHalo(..., periodic=)``, per axis, as ``radius_graph(periodic=)``): the halo is made of *ghost
images*.  An entry ``(peer q, offset d)`` replaces a neighbour: ``coords(me) + d`` is wrapped modulo ``dims`` on the periodic
axes, and the entry's translation ``t`` (whole box lengths per axis) moves q's box next to mine at offset ``d``.  The owner of
a particle sends it, shifted by ``-t``, to every image box whose r-neighbourhood holds it, so the same peer can appear several
times with different shifts, and with one or two boxes along an axis a rank is its own neighbour (self entries are served
by local copies, never by ``torch.distributed``).  ``setup`` wraps the owned positions (the graph builder's formula) and
the local graph is an OPEN graph over ``[wrapped owned | ghost images]``: its edge vectors are the minimum images, and
``split_graph`` / ``start`` / ``finish`` work unchanged.  Rounding contract: the sharded periodic graph has exactly the edges
of ``radius_graph(periodic=True)`` over the whole cloud when the image shifts are exact in fp32 (e.g. dyadic coordinates
with a dyadic box length); otherwise a pair within about 1 ulp of the cutoff may differ, and edge vectors agree to fp32
rounding.  On ROCm tensors the selection is one HIP launch pair (``csrc/e3_halo.hip``); on CPU tensors (gloo rehearsal) a
torch restatement of the same predicate and order (``select_images_torch``).

Only point-to-point traffic between adjacent boxes (``batch_isend_irecv`` = grouped ncclSend/ncclRecv on RCCL: every pair
talks over its own xGMI link; no ring, no collective over all ranks).  Host syncs: two per graph build (one ``nonzero`` over
all neighbours at once -- periodic: one read of the selection's counts --, one read of the incoming counts), one per graph in
``split_graph`` (three edge counts), none per layer.
"""
from __future__ import annotations

import ctypes
import itertools
from dataclasses import dataclass

import numpy as np
import torch
import torch.distributed as dist

from .radius_graph import periodic_mask

# neighbour offsets; the index of the RECEIVER-side offset is the P2POp tag of a periodic entry's messages (gloo matches by
# tag, RCCL by order: the ops with one peer are posted in tag order, so both pair the entries of a peer correctly)
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


def select_images_torch(pos, lo, hi, periodic, r, entries):
    """Torch restatement of ``e3_halo_select_count`` / ``_fill`` (any device): -> (pos_wrapped [n,3] fp32, idx [total]
    int64, counts (list of int), ghost_pos [total,3] fp32).  ``entries``: ``[(lo3, hi3, shift3), ...]`` fp32 values."""
    mask = periodic_mask(periodic, r, lo, hi)
    if pos.dtype != torch.float32 or pos.dim() != 2 or pos.shape[1] != 3:
        raise TypeError(f"periodic halo positions must be [n,3] float32, got {tuple(pos.shape)} {pos.dtype}")
    dev = pos.device
    pw = _wrap_torch(pos, lo, hi, mask)
    ne = len(entries)
    if ne == 0 or pos.shape[0] == 0:
        return pw, torch.empty(0, dtype=torch.long, device=dev), [0] * ne, torch.empty((0, 3), dtype=torch.float32, device=dev)
    elo = torch.tensor([e[0] for e in entries], dtype=torch.float32, device=dev)
    ehi = torch.tensor([e[1] for e in entries], dtype=torch.float32, device=dev)
    esh = torch.tensor([e[2] for e in entries], dtype=torch.float32, device=dev)
    m = ((pw[None, :, :] >= elo[:, None, :]) & (pw[None, :, :] < ehi[:, None, :])).all(-1)   # [ne, n], entry-major
    ent, idx = m.nonzero(as_tuple=True)
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
    if pos.dtype != torch.float32 or pos.dim() != 2 or pos.shape[1] != 3:
        raise TypeError(f"periodic halo positions must be [n,3] float32, got {tuple(pos.shape)} {pos.dtype}")
    lib = _lib.load()
    pos = pos.contiguous()
    dev, n, ne = pos.device, pos.shape[0], len(entries)
    arr = (_lib.HaloEntry * max(ne, 1))()
    for i, (elo, ehi, esh) in enumerate(entries):
        for a in range(3):
            arr[i].lo[a], arr[i].hi[a], arr[i].shift[a] = elo[a], ehi[a], esh[a]
    args = (_lib.Float3(*lo), _lib.Float3(*hi), mask, float(r), arr, ne)
    pw = torch.empty((n, 3), dtype=torch.float32, device=dev)
    counts = torch.zeros(max(ne, 1), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        wbytes = int(lib.e3_halo_select_workspace_bytes(n, ne))
        if wbytes < 0:
            raise RuntimeError(f"e3_halo_select_workspace_bytes: unsupported size (n = {n}, {ne} entries)")
        ws = torch.empty(max(wbytes, 16), dtype=torch.uint8, device=dev)
        _lib.check(lib.e3_halo_select_count(pos.data_ptr(), n, *args, pw.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                            wbytes, stream), "e3_halo_select_count")
        cnt = [int(v) for v in counts[:ne].tolist()] if ne else []                  # the one host read of the selection
        total = sum(cnt)
        idx = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        ghost = torch.empty((max(total, 1), 3), dtype=torch.float32, device=dev)
        _lib.check(lib.e3_halo_select_fill(pw.data_ptr(), n, *args, total, idx.data_ptr(), ghost.data_ptr(), ws.data_ptr(),
                                           wbytes, stream), "e3_halo_select_fill")
    return pw, idx[:total].long(), cnt, ghost[:total]


@dataclass
class SplitGraph:
    """Edge lists of a sharded graph, all sorted by dst (CSR order) in the graph's local (Morton) numbering."""
    graph: object                 # RadiusGraph with the edges into ghost rows removed (rowptr / src / dst consistent)
    interior: tuple               # (src int32 [Ei], dst int32 [Ei]): owned src
    boundary: tuple               # (src int32 [Eb], dst int32 [Eb]): ghost src
    dropped: int                  # edges into ghost rows that were removed


class GridHalo:
    """Ghost-cell halo of a ``dims = (px, py, pz)`` grid of equal boxes covering ``[lo, hi)``; rank = (ix py + iy) pz + iz.

    ``periodic`` (bool or 3 bools, validated by ``radius_graph.periodic_mask``): those axes wrap at ``[lo, hi)`` and the halo
    is built from ghost images (module docstring).  ``images`` lists the entries ``(peer, d, t)``; in periodic mode
    ``send_counts`` / ``recv_counts`` are per entry, ``neighbours`` stays the sorted distinct peers other than this rank.
    Positions must then be fp32; ``setup`` returns the owned ones wrapped.  Works without a process group at world 1
    (dims (1, 1, 1) with periodic axes: a pure self-halo)."""

    def __init__(self, dims, lo, hi, group=None, periodic=False):
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.dims = tuple(int(d) for d in dims)
        if self.dims[0] * self.dims[1] * self.dims[2] != self.world:
            raise ValueError(f"grid {self.dims} needs {self.dims[0] * self.dims[1] * self.dims[2]} ranks, the group has {self.world}")
        self.lo = [float(v) for v in lo]
        self.hi = [float(v) for v in hi]
        self.n_owned = 0
        self.bytes_last_exchange = 0
        self.neighbours = []       # adjacent ranks, ascending
        self.periodic = periodic_mask(periodic, 0.0, self.lo, self.hi)   # axis bit mask; 0 = open box (the original path)
        self._axes = tuple(bool((self.periodic >> a) & 1) for a in range(3))
        self.images = []           # entries (peer, d, t)
        self._set_boxes()

    # -- geometry -------------------------------------------------------------------------------------
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

    def _set_boxes(self):
        me = self.coords(self.rank)
        nb = set()
        for d in itertools.product((-1, 0, 1), repeat=3):
            c = [me[a] + d[a] for a in range(3)]
            if d != (0, 0, 0) and all(0 <= c[a] < self.dims[a] for a in range(3)):
                nb.add((c[0] * self.dims[1] + c[1]) * self.dims[2] + c[2])
        self.neighbours = sorted(nb)
        self.images = image_entries(self.dims, self.lo, self.hi, self._axes, self.rank)
        if self.periodic:
            ent = self.images
            self.neighbours = sorted({q for q, _, _ in ent if q != self.rank})
            at = {d: e for e, (_, d, _) in enumerate(ent)}
            # self entry e receives what this rank sends for its entry (me, -d)
            self._self_pairs = [(e, at[tuple(-v for v in d)]) for e, (q, d, _) in enumerate(ent) if q == self.rank]
            remote = [e for e, (q, _, _) in enumerate(ent) if q != self.rank]
            self._remote = remote
            # per peer, in tag order (the receiver-side offset: -d for what I send, d for what I receive)
            self._send_ops = sorted((ent[e][0], OFFSETS.index(tuple(-v for v in ent[e][1])), e) for e in remote)
            self._recv_ops = sorted((ent[e][0], OFFSETS.index(ent[e][1]), e) for e in remote)

    def _selection(self, r):
        """fp32 selection bounds and shift of every entry, sender side: the owned particles in ``[blo + t - r, bhi + t + r)``
        of the peer's box go to it, at ``p - t``."""
        out = []
        for q, _, t in self.images:
            blo, bhi = self.box(q)
            out.append(([_f32(blo[a] + t[a] - r) for a in range(3)], [_f32(bhi[a] + t[a] + r) for a in range(3)],
                        [-t[a] if t[a] else 0.0 for a in range(3)]))
        return out

    # -- p2p helpers ----------------------------------------------------------------------------------
    def _post_images(self, sends, recvs):
        """Periodic mode: grouped send / recv of the remote entries (``sends[e]`` / ``recvs[e]`` by entry index), per peer
        in tag order; empty messages are skipped on both ends."""
        ops = []
        for q, tag, e in self._send_ops:
            if sends[e].numel():
                ops.append(dist.P2POp(dist.isend, sends[e], q, self.group, tag=tag))
        for q, tag, e in self._recv_ops:
            if recvs[e].numel():
                ops.append(dist.P2POp(dist.irecv, recvs[e], q, self.group, tag=tag))
        return dist.batch_isend_irecv(ops) if ops else []

    def _start_images(self, sends, recvs):
        """Periodic mode: serve the self entries by local copies, post the others -> (kind, works, (host recvs, recvs))."""
        for e, m in self._self_pairs:
            recvs[e].copy_(sends[m])
        if self._remote and self._staged(sends[self._remote[0]]):
            hs = {e: sends[e].cpu() for e in self._remote}
            hr = {e: torch.empty(recvs[e].shape, dtype=recvs[e].dtype) for e in self._remote}
            return "staged", self._post_images(hs, hr), ([hr[e] for e in self._remote], [recvs[e] for e in self._remote])
        return "direct", (self._post_images(sends, recvs) if self._remote else []), ([], [])

    def _sendrecv_images(self, sends, recvs):
        kind, works, (hr, rr) = self._start_images(sends, recvs)
        for w in works:
            w.wait()
        for d, s in zip(rr, hr):
            d.copy_(s)

    def _staged(self, t):
        """gloo has no device transport: device tensors are staged through host memory (rehearsal mode only)."""
        return t.is_cuda and dist.get_backend(self.group) == "gloo"

    def _post(self, sends, recvs):
        """Grouped send / recv with every neighbour (empty messages are skipped on both ends: the sizes were agreed on in
        ``setup``)."""
        ops = []
        for q, s, r in zip(self.neighbours, sends, recvs):
            if s.numel():
                ops.append(dist.P2POp(dist.isend, s, q, self.group))
            if r.numel():
                ops.append(dist.P2POp(dist.irecv, r, q, self.group))
        return dist.batch_isend_irecv(ops) if ops else []

    def _sendrecv(self, sends, recvs):
        if sends and self._staged(sends[0]):
            hs, hr = [t.cpu() for t in sends], [t.cpu() for t in recvs]
            for w in self._post(hs, hr):
                w.wait()
            for d, s in zip(recvs, hr):
                d.copy_(s)
            return
        for w in self._post(sends, recvs):
            w.wait()

    # -- once per graph build -------------------------------------------------------------------------
    def setup(self, pos: torch.Tensor, feats: torch.Tensor, r: float):
        """pos [n,3], feats [n,F] of the owned particles -> (local_pos, local_feats) with the ghosts of every adjacent box
        appended in neighbour order.  Positions and features travel in their own dtypes.
        Periodic mode: ``[wrapped owned | ghost images]``, the images in entry order (``images``)."""
        if self.periodic:
            return self._setup_images(pos, feats, r)
        dev = pos.device
        n = pos.shape[0]
        self.n_owned = n
        nn = len(self.neighbours)
        w = min((self.hi[a] - self.lo[a]) / self.dims[a] for a in range(3) if self.dims[a] > 1) if nn else float("inf")
        if nn and r > w:
            raise ValueError(f"cutoff {r} exceeds the box width {w}: ghosts would come from beyond the adjacent boxes")
        if nn:
            # my particles within r (per axis: a superset of the r-ball) of each adjacent box -- one mask, ONE nonzero
            blo = torch.tensor([self.box(q)[0] for q in self.neighbours], dtype=pos.dtype, device=dev)   # [nn, 3]
            bhi = torch.tensor([self.box(q)[1] for q in self.neighbours], dtype=pos.dtype, device=dev)
            m = ((pos[None, :, :] >= blo[:, None, :] - r) & (pos[None, :, :] < bhi[:, None, :] + r)).all(-1)   # [nn, n]
            nbr, idx = m.nonzero(as_tuple=True)                     # sorted by neighbour, then particle  (host sync #1)
            cnt_out = torch.bincount(nbr, minlength=nn)
        else:
            idx = torch.empty(0, dtype=torch.long, device=dev)
            cnt_out = torch.zeros(0, dtype=torch.int64, device=dev)
        cnt_in = torch.zeros_like(cnt_out)
        self._sendrecv([cnt_out[i:i + 1] for i in range(nn)], [cnt_in[i:i + 1] for i in range(nn)])
        both = torch.stack([cnt_out, cnt_in]).tolist() if nn else [[], []]                               # host sync #2
        self.send_counts, self.recv_counts = [int(v) for v in both[0]], [int(v) for v in both[1]]
        self.sel = idx                                   # original indices of the particles sent, grouped by neighbour
        self._send_idx = idx
        out = []
        ng = sum(self.recv_counts)
        for t in (pos, feats):
            sends = list(t[idx].contiguous().split(self.send_counts)) if nn else []
            ghosts = torch.empty((ng, t.shape[1]), dtype=t.dtype, device=dev)
            self._sendrecv(sends, list(ghosts.split(self.recv_counts)) if nn else [])
            out.append(torch.cat([t, ghosts], 0))
        self.n_ghost = ng
        self._recv_idx = torch.arange(n, n + ng, device=dev)
        return out[0], out[1]

    def _setup_images(self, pos, feats, r):
        check_cutoff(self.dims, self.lo, self.hi, self._axes, r)        # ValueError before any transfer
        dev = pos.device
        n = pos.shape[0]
        self.n_owned = n
        ne = len(self.images)
        pw, idx, cnt_out, gpos = select_images(pos, self.lo, self.hi, self._axes, r, self._selection(r))  # host sync #1
        cnt_in = [0] * ne
        for e, m in self._self_pairs:
            cnt_in[e] = cnt_out[m]
        if self._remote:
            cdev = torch.device("cpu") if dist.get_backend(self.group) == "gloo" else dev
            co = torch.tensor(cnt_out, dtype=torch.int64, device=cdev)
            ci = torch.zeros(ne, dtype=torch.int64, device=cdev)
            works = self._post_images(list(co.split(1)), list(ci.split(1)))
            for w in works:
                w.wait()
            got = ci.tolist()                                                                   # host sync #2
            for e in self._remote:
                cnt_in[e] = int(got[e])
        self.send_counts, self.recv_counts = cnt_out, cnt_in
        self.sel = idx                         # original indices of the particles sent, grouped by entry
        self._send_idx = idx
        ng = sum(cnt_in)
        out = []
        for t, send in ((pw, gpos), (feats, None)):
            if send is None:
                send = t[idx]
            ghosts = torch.empty((ng, t.shape[1]), dtype=t.dtype, device=dev)
            self._sendrecv_images(list(send.split(cnt_out)), list(ghosts.split(cnt_in)))
            out.append(torch.cat([t, ghosts], 0))
        self.n_ghost = ng
        self._recv_idx = torch.arange(n, n + ng, device=dev)
        return out[0], out[1]

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
        return self

    def ghost_fraction(self) -> float:
        return self.n_ghost / max(1, self.n_owned)

    def split_graph(self, g) -> SplitGraph:
        """Drop the edges into ghost rows and split the rest by the ownership of their src (see the module docstring).
        ``g``: the RadiusGraph of the local cloud (after ``renumber(g.perm)``)."""
        from .radius_graph import RadiusGraph
        src, dst = g.src, g.dst
        N, E = g.rowptr.numel() - 1, int(src.numel())
        if src.is_cuda:
            # one classification + compaction on the device (csrc/e3_shard.hip); ONE host read for the three counts
            from . import _lib
            lib = _lib.load()
            dev = src.device
            ghost8 = self.is_ghost.to(torch.uint8)
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
        keep = ~self.is_ghost[dst.long()]
        src_k, dst_k = src[keep], dst[keep]
        deg = (g.rowptr[1:] - g.rowptr[:-1]).clone()
        deg[self.is_ghost] = 0
        rowptr = torch.zeros_like(g.rowptr)
        rowptr[1:] = torch.cumsum(deg, 0)
        g2 = RadiusGraph(g.perm, g.pos4, rowptr, src_k.contiguous(), int(src_k.numel()), g.grid)
        object.__setattr__(g2, "_dst", dst_k.contiguous())
        ghost_src = self.is_ghost[src_k.long()]
        interior = (src_k[~ghost_src].contiguous(), dst_k[~ghost_src].contiguous())
        boundary = (src_k[ghost_src].contiguous(), dst_k[ghost_src].contiguous())
        return SplitGraph(g2, interior, boundary, int(src.numel() - src_k.numel()))

    # -- once per layer -------------------------------------------------------------------------------
    def start(self, h: torch.Tensor):
        """Post this layer's ghost refresh (boundary rows of ``h`` to the neighbours) and return a token for ``finish``.
        Kernels launched between the two calls overlap the transfer as long as they do not read ghost rows."""
        D = h.shape[1]
        recv = torch.empty((self.n_ghost, D), dtype=h.dtype, device=h.device)
        send = h[self._send_idx].contiguous()
        sends, recvs = list(send.split(self.send_counts)), list(recv.split(self.recv_counts))
        if self.periodic:
            # self entries: local copies (not counted as exchanged bytes); the rest over torch.distributed
            self.bytes_last_exchange = sum(self.send_counts[e] for e in self._remote) * D * h.element_size()
            kind, works, (hr, rr) = self._start_images(sends, recvs)
            return (kind, works, recv, (send, hr, rr))
        self.bytes_last_exchange = send.numel() * h.element_size()
        if self._staged(h):
            hs, hr = [t.cpu() for t in sends], [t.cpu() for t in recvs]
            return ("staged", self._post(hs, hr), recv, (hs, hr, recvs))
        return ("direct", self._post(sends, recvs), recv, (send,))

    def finish(self, h: torch.Tensor, token) -> torch.Tensor:
        """Wait for the transfer and write the ghost rows of ``h`` in place (one indexed copy, no clone of ``h``).
        Inference only: a tensor autograd has saved for backward must not be overwritten."""
        if torch.is_grad_enabled() and h.requires_grad:
            raise RuntimeError("the halo refresh writes ghost rows in place: not differentiable (run under torch.no_grad())")
        kind, works, recv, keep = token
        for w in works:
            w.wait()
        if kind == "staged":
            for d, s in zip(keep[2], keep[1]):
                d.copy_(s)
        if recv.shape[0]:
            h.index_copy_(0, self._recv_idx, recv)
        return h

    def exchange(self, h: torch.Tensor) -> torch.Tensor:
        """Blocking form: overwrite the ghost rows of ``h`` (local numbering) with the owners' current values, in place."""
        return self.finish(h, self.start(h))

    def ghost_rows(self) -> torch.Tensor:
        """Local (graph-order) ids of the ghost rows."""
        return self._recv_idx


class SlabHalo(GridHalo):
    """Slabs along x: rank k owns ``x in [slab_lo, slab_hi)`` (given at ``setup``), unbounded in y and z."""

    def __init__(self, group=None):
        world = dist.get_world_size(group) if dist.is_initialized() else 1
        super().__init__((world, 1, 1), (0.0, -1e30, -1e30), (float(world), 1e30, 1e30), group)
        self.left = self.rank - 1 if self.rank > 0 else None
        self.right = self.rank + 1 if self.rank < self.world - 1 else None

    def setup(self, pos, feats, slab_lo: float, slab_hi: float, r: float):
        w = float(slab_hi) - float(slab_lo)
        self.lo[0] = float(slab_lo) - self.rank * w
        self.hi[0] = self.lo[0] + self.world * w
        out = super().setup(pos, feats, r)
        by = dict(zip(self.neighbours, self.recv_counts))
        self.n_ghost_left = by.get(self.left, 0) if self.left is not None else 0
        self.n_ghost_right = by.get(self.right, 0) if self.right is not None else 0
        return out

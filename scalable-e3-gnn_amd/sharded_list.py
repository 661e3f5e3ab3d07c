"""Verlet neighbour list of a sharded cloud (host side of ``e3_nl_update_split`` in include/e3gnn.h).

``neighbor_list.NeighborList`` across ranks: the halo is set up and the local graph over ``[owned | ghosts]`` is built ONCE at
``r + skin`` and kept, split included.  Every ``update(pos, x)`` measures how far the owned particles have moved since the
build (minimum image), agrees with the other ranks on one word -- the largest displacement anywhere -- and, while nobody has
moved ``skin / 2``, sends the current positions along the halo's stored entries (``Halo.update_positions``: no selection, no
count exchange) and cuts the stored edge list down to the pairs within ``r`` and into its interior / boundary parts in one
pass on the device (``e3_nl_update_split``), with one host read of the three counts.  Otherwise every rank rebuilds first.

Ownership is frozen between two builds, and a halo ``r + skin`` wide is complete only for particles inside their owner's
region: a build checks ``halo.owner_of(pos) == rank`` for every owned particle and raises ``OwnershipChanged`` on EVERY rank
when any rank has a stray.  ``redistribute(pos, x, *rows)``, called before the model on every step, is the way through a
crossing: it takes the same shared decision, and when a rebuild is due it moves the strays to their new owners first
(``Halo.migrate``), so the build that follows finds none; while the list holds it hands its decision to the ``update`` of the
same positions and costs nothing more.  ``update`` without it behaves as before.

The rounding budget behind ``skin / 2`` and ``MAX_COORD_OVER_SKIN``: DESIGN.md §4.4b.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass

import torch
import torch.distributed as dist

from . import _lib
from .neighbor_list import MAX_COORD_OVER_SKIN, verlet_threshold
from .radius_graph import RadiusGraph, radius_graph
from .sharding import SplitGraph, all_reduce_sum

_STALE = 0xffffffff   # the all-ones word: a NaN pattern, above every threshold


class OwnershipChanged(RuntimeError):
    """An owned particle has left its owner's region (raised by every rank of the halo's group at once): redistribute the
    particles by ``halo.owner_of`` and call again -- ``ShardedNeighborList.redistribute`` before every ``update`` does."""


@dataclass
class ShardedCloud:
    """The local cloud of one step in graph order, ``[owned | ghosts]`` renumbered by the stored graph's ``perm``."""
    split: SplitGraph        # the graph at r: ``split.graph`` and its interior / boundary lists
    x: torch.Tensor          # [n_local, F] features
    pos: torch.Tensor        # [n_local, 3] local coordinates (``split.graph.pos4[:, :3]``)


def _norm2(d):
    """fl(fl(fl(x x) + fl(y y)) + fl(z z)), one torch op per rounding: the builder's sum order."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    return (x * x + y * y) + z * z


def _max_bits(d2):
    """Largest of the fp32 patterns of ``d2`` with the sign cleared, as an int64 0-d tensor (0 for an empty one): non-negative
    floats order as their bits and a NaN pattern orders above +inf."""
    if d2.numel() == 0:
        return torch.zeros((), dtype=torch.int64, device=d2.device)
    return (d2.contiguous().view(torch.int32).long() & 0x7fffffff).max()


def _as_float(bits: int) -> float:
    return struct.unpack("<f", struct.pack("<I", bits & 0xffffffff))[0]


def nl_update_split_torch(pos, perm, ref_pos4, rowptr, src, is_ghost, r):
    """Torch restatement of ``e3_nl_update_split`` (any device; the CPU twin of the entry): the same lists in the same
    order, every fp32 operation an op of its own.  -> (pos4 [N,4], rowptr_out [N+1] int32, src, dst [E_kept] int32,
    (src, dst) interior, (src, dst) boundary, stats [4] int64 = {bits of max d2, E_kept, E_interior, E_boundary})."""
    N = perm.numel()
    dev = pos.device
    perm_l, src_l = perm.long(), src.long()
    cur = pos[perm_l].float()
    pos4 = torch.zeros((N, 4), dtype=torch.float32, device=dev)
    pos4[:, :3] = cur
    ghost = is_ghost.bool()
    deg = (rowptr[1:] - rowptr[:-1]).long()
    dst_l = torch.repeat_interleave(torch.arange(N, device=dev), deg)
    bits = _max_bits(_norm2(cur - ref_pos4[:, :3]))
    r32 = torch.tensor(float(r), dtype=torch.float32)
    keep = (_norm2(cur[src_l] - cur[dst_l]) <= float(r32 * r32)) & ~ghost[dst_l]
    s, d = src_l[keep], dst_l[keep]
    rowptr_out = torch.zeros(N + 1, dtype=torch.int32, device=dev)
    rowptr_out[1:] = torch.cumsum(torch.bincount(d, minlength=N), 0)
    gs = ghost[s]
    s, d = s.to(torch.int32), d.to(torch.int32)
    inner, outer = (s[~gs].contiguous(), d[~gs].contiguous()), (s[gs].contiguous(), d[gs].contiguous())
    stats = torch.stack([bits, *[torch.tensor(v, device=dev) for v in (s.numel(), inner[0].numel(), outer[0].numel())]])
    return pos4, rowptr_out, s, d, inner, outer, stats


class ShardedNeighborList:
    """``nl = ShardedNeighborList(r, skin, halo)`` (a ``GridHalo``, open or periodic, or a ``MortonHalo``);
    ``cloud = nl.update(pos, x)`` -- a collective: every rank of ``halo.group`` calls it -- is the local cloud at radius
    ``r`` for the owned positions ``pos`` [n,3] fp32 and features ``x`` [n,F] (``ShardedCloud``).

    ``builds`` / ``updates`` count the builds and the ``update`` calls; ``rebuilt`` tells whether the last update built (the
    same on every rank).  The list owns the halo's index state while it holds: a ``halo.setup`` by anyone else is noticed
    (``halo.generation``) and forces a rebuild.  ``graph_builder(lpos, R, lo, hi) -> RadiusGraph``: the builder of the
    local graph, ``radius_graph`` (ROCm tensors); a CPU rehearsal passes a host builder."""

    def __init__(self, r: float, skin: float, halo, graph_builder=radius_graph):
        self.r, self.skin = float(r), float(skin)
        if not (self.r > 0.0 and self.r < float("inf")):
            raise ValueError(f"r must be positive and finite, got {r}")
        if not (self.skin > 0.0 and self.skin < float("inf")):
            raise ValueError(f"skin must be positive, got {skin}: a list without a skin rebuilds on every step")
        if not (hasattr(halo, "local_bounds") and hasattr(halo, "owner_of")):
            raise TypeError("ShardedNeighborList needs a GridHalo or a MortonHalo")
        self.halo = halo
        self.graph_builder = graph_builder
        self.threshold = verlet_threshold(self.skin)
        self.builds = self.updates = 0
        self.migrations = self.migrated = 0     # redistributions that moved something; ``halo.migrated`` of the last one
        self.rebuilt = False
        self._g = None
        self._ws = self._stats = None
        self._held = None                       # ``redistribute``'s decision, for the ``update`` of the same positions

    @property
    def stored(self):
        """The stored ``SplitGraph`` at ``r + skin`` (None before the first build and after ``invalidate``)."""
        return self._g

    def invalidate(self):
        """Drop the stored graph: the next update rebuilds (on every rank: the decision is shared)."""
        self._g = None
        self._held = None

    # ---- the shared decision ------------------------------------------------------------------------------------------
    def _all_reduce(self, t, op):
        halo = self.halo
        if not dist.is_initialized() or halo.world == 1:
            return t
        buf = t.cpu() if t.is_cuda and dist.get_backend(halo.group) == "gloo" else t.clone()
        dist.all_reduce(buf, op=op, group=halo.group)
        return buf

    def _decide(self, pos):
        """-> (whether every rank's list holds, this rank's displacement | None).  The local word is the bits of max d2 of
        the owned particles (all ones when this rank has no list to hold); ONE all-reduce MAX, before any exchange."""
        halo, g = self.halo, self._g
        disp = None
        if (g is None or halo.generation != self._generation or pos.shape[0] != halo.n_owned or
                pos.device != g.graph.perm.device):
            word = torch.full((1,), _STALE, dtype=torch.int64, device=pos.device)
        else:
            disp = halo.displacement(pos)
            word = _max_bits(_norm2(disp)).reshape(1)
        bits = int(self._all_reduce(word, dist.ReduceOp.MAX).item())
        return _as_float(bits) < self.threshold, disp

    # ---- build --------------------------------------------------------------------------------------------------------
    def _build(self, pos, x):
        halo, R = self.halo, self.r + self.skin
        lo, hi = halo.local_bounds(R)
        # both refusals are collective: a rank that raised alone would leave its peers waiting in the next exchange
        strays = (halo.owner_of(pos) != halo.rank).sum().reshape(1)
        limit = MAX_COORD_OVER_SKIN * self.skin
        bad = torch.zeros_like(strays)
        if pos.shape[0]:
            bad = (~(pos.abs().max() <= limit)).long().reshape(1)
        if not max(abs(float(v)) for v in list(lo) + list(hi)) <= limit:
            bad = torch.ones_like(strays)
        n_stray, n_bad = (int(v) for v in all_reduce_sum(torch.cat([strays, bad]), halo.group).tolist())
        if n_stray:
            raise OwnershipChanged(f"ShardedNeighborList: {n_stray} particle(s) are no longer inside their owner's region: "
                                   "redistribute the particles by halo.owner_of and call again")
        if n_bad:
            raise ValueError(f"ShardedNeighborList: on {n_bad} rank(s) the coordinates or the local bounds exceed "
                             f"{MAX_COORD_OVER_SKIN} skin (skin = {self.skin}; or a position is not finite): the fp32 rounding "
                             "of the displacements is not covered; shift the origin or enlarge the skin")
        lpos, _ = halo.setup(pos, x, R)
        g = self.graph_builder(lpos, R, lo, hi)
        halo.renumber(g.perm)
        self._g = halo.split_graph(g)               # the kept graph: the edges into ghost rows are gone for good
        self._ghost8 = halo.is_ghost.to(torch.uint8)
        self._generation = halo.generation
        self.builds += 1
        if pos.is_cuda:
            wbytes = int(_lib.load().e3_nl_update_split_workspace_bytes(lpos.shape[0]))
            if wbytes < 0:
                raise RuntimeError("e3_nl_update_split_workspace_bytes: invalid arguments")
            if self._ws is None or self._ws.numel() < wbytes or self._ws.device != pos.device:
                self._ws = torch.empty(max(wbytes, 16), dtype=torch.uint8, device=pos.device)
                self._stats = torch.zeros(4, dtype=torch.int32, device=pos.device)

    # ---- prune --------------------------------------------------------------------------------------------------------
    def _prune(self, pos, x, disp):
        halo, g = self.halo, self._g.graph
        lpos, lx = halo.update_positions(pos, x, disp=disp)
        lpos = lpos.contiguous()
        N, E, dev = lpos.shape[0], g.num_edges, lpos.device
        if not lpos.is_cuda:
            pos4, rowptr, src, dst, inner, outer, stats = nl_update_split_torch(lpos, g.perm, g.pos4, g.rowptr, g.src,
                                                                               self._ghost8, self.r)
            ek = int(src.numel())
        else:
            lib = _lib.load()
            with torch.cuda.device(dev):
                pos4 = torch.empty((N, 4), dtype=torch.float32, device=dev)
                rowptr = torch.empty(N + 1, dtype=torch.int32, device=dev)
                outs = [torch.empty(max(E, 1), dtype=torch.int32, device=dev) for _ in range(6)]
                _lib.check(lib.e3_nl_update_split(
                    lpos.data_ptr(), g.perm.data_ptr(), g.pos4.data_ptr(), g.rowptr.data_ptr(), g.src.data_ptr(),
                    self._ghost8.data_ptr(), N, E, self.r, pos4.data_ptr(), rowptr.data_ptr(), *[o.data_ptr() for o in outs],
                    self._stats.data_ptr(), self._ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                    "e3_nl_update_split")
                _, ek, ei, eb = self._stats.tolist()      # the one host read of the prune
            src, dst = outs[0][:ek], outs[1][:ek]
            inner, outer = (outs[2][:ei], outs[3][:ei]), (outs[4][:eb], outs[5][:eb])
        out = RadiusGraph(g.perm, pos4, rowptr, src, ek, g.grid)
        object.__setattr__(out, "_dst", dst)
        perm = g.perm.long()
        return ShardedCloud(SplitGraph(out, inner, outer, E - ek), lx[perm], pos4[:, :3])

    # ---- redistribute -------------------------------------------------------------------------------------------------
    def _key(self, pos):
        """What "the same positions" means between ``redistribute`` and the ``update`` that follows: the same storage,
        shape and version counter, and a halo nobody has set up or migrated in between."""
        return (pos.data_ptr(), tuple(pos.shape), pos.stride(), pos._version, pos.device, self.halo.generation)

    def redistribute(self, pos: torch.Tensor, x: torch.Tensor, *rows: torch.Tensor):
        """Call before the model on every step -- a collective --: ``(pos, x, *rows)`` of the particles this rank owns,
        before -> after.  While the list holds (the shared decision of ``update``) the inputs themselves come back and the
        decision is kept for the ``update`` of the same ``pos`` tensor, which then skips its own: a holding step costs one
        all-reduce, with or without this call.  When a rebuild is due, ``halo.migrate(pos, x, *rows)`` moves every particle
        that has left its owner's region to its new rank (order of the result: ``Halo.migrate``) and the list is
        invalidated: the ``update`` that follows builds, and its stray check passes.  ``rows``: whatever else the caller
        keeps per particle (velocities, ids; ``sharding.pack_rows``).  ``migrations`` counts the calls that moved
        something, ``migrated`` is ``halo.migrated`` of the last one."""
        if pos.dtype != torch.float32 or pos.dim() != 2 or pos.shape[1] != 3:
            raise RuntimeError(f"pos must be [n,3] float32, got {tuple(pos.shape)} {pos.dtype}")
        if x.shape[0] != pos.shape[0]:
            raise ValueError(f"x has {x.shape[0]} rows for {pos.shape[0]} positions")
        self._held = None
        holds, disp = self._decide(pos)
        if holds:
            self._held = (self._key(pos), disp)
            return (pos, x, *rows)
        out = self.halo.migrate(pos, x, *rows)
        self.migrated = self.halo.migrated
        self.migrations += 1 if self.migrated else 0
        self.invalidate()
        return out

    def update(self, pos: torch.Tensor, x: torch.Tensor) -> ShardedCloud:
        """pos [n,3] fp32, x [n,F]: the particles this rank owns, in the same order on every call between two builds
        (periodic coordinates may be unwrapped or re-wrapped).  Rebuilds -- on every rank -- when any rank has no stored
        list, has seen ``n``, the device or the halo's ``generation`` change, or has a particle that moved ``skin / 2``."""
        if pos.dtype != torch.float32 or pos.dim() != 2 or pos.shape[1] != 3:
            raise RuntimeError(f"pos must be [n,3] float32, got {tuple(pos.shape)} {pos.dtype}")
        if x.shape[0] != pos.shape[0]:
            raise ValueError(f"x has {x.shape[0]} rows for {pos.shape[0]} positions")
        self.updates += 1
        self.rebuilt = False
        held, self._held = self._held, None
        if held is not None and held[0] == self._key(pos):
            holds, disp = True, held[1]          # ``redistribute`` has just decided for these positions, on every rank
        else:
            holds, disp = self._decide(pos)
        if not holds:
            self._build(pos, x)
            self.rebuilt = True
            holds, disp = self._decide(pos)
            if not holds:
                self._g = None
                raise RuntimeError("ShardedNeighborList: a displacement of the freshly built list is not below skin / 2: a "
                                   "position is not finite")
        return self._prune(pos, x, disp)

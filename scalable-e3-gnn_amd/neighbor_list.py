"""Verlet neighbour list (host side of ``e3_nl_update*`` in include/e3gnn.h).

The graph is built once at ``r + skin`` by the ordinary builder and kept.  Every ``update(pos)`` gathers the current
positions into the stored node order, measures how far each particle has moved since the build (minimum image, so
re-wrapped coordinates do not count as motion) and cuts the stored edge list down to the pairs within ``r`` -- all on the
device, with one host read of two words.  While no particle has moved ``skin / 2`` the result is the radius graph at ``r``
for the current positions: an ordinary ``RadiusGraph`` for every model and every path; otherwise the list is rebuilt first.

Why ``skin / 2`` is enough, and what the ``2^-10`` of the threshold pays for: DESIGN.md §4.4b.  The argument needs the
coordinates (and the box or cell extents) to stay below ``MAX_COORD_OVER_SKIN * skin``; a build checks that.
"""
from __future__ import annotations

import ctypes
import struct

import torch

from . import _lib
from .radius_graph import (RadiusGraph, _check_pos, cell_check_cutoff, cell_params, periodic_mask, radius_graph)

# the roundings of the displacement, of the pruned edge vector and of the builder's own edge vector stay below
# 64 * 2^-24 X for coordinates of magnitude <= X; the threshold leaves skin * 2^-10 for them: X <= 2^8 skin
MAX_COORD_OVER_SKIN = 256.0


def _f32(v: float) -> float:
    return ctypes.c_float(v).value


def verlet_threshold(skin: float) -> float:
    """thr = fl32(h h), h = fl32(0.5 skin (1 - 2^-10)) of the fp32 skin: the list is valid while max_i d2_i < thr."""
    h = _f32(0.5 * _f32(skin) * (1.0 - 2.0 ** -10))  # both factors are fp32 numbers: one rounding
    return _f32(h * h)


class NeighborList:
    """``nl = NeighborList(r, skin, lo, hi, periodic)`` / ``NeighborList(r, skin, cell=, origin=)`` /
    ``NeighborList(r, skin, batch=batch)``; ``g = nl.update(pos)`` is the ``RadiusGraph`` at radius ``r`` of ``pos``.

    ``builds`` / ``updates`` count the builder runs and the ``update`` calls; ``rebuilt`` tells whether the last update
    ran the builder.  With ``batch=`` (molecule id of every atom) the stored graph is ``batched_radius_graph``'s, open, and
    ``mol_of_node`` holds the molecule of every node in the graph's order."""

    def __init__(self, r: float, skin: float, lo=None, hi=None, periodic=False, cell=None, origin=None, batch=None):
        self.r, self.skin = float(r), float(skin)
        if not (self.r > 0.0 and self.r < float("inf")):
            raise ValueError(f"r must be positive and finite, got {r}")
        if not (self.skin > 0.0 and self.skin < float("inf")):
            raise ValueError(f"skin must be positive, got {skin}: a list without a skin rebuilds on every step, which is "
                             "what radius_graph does")
        self.batch = batch
        self.threshold = verlet_threshold(self.skin)
        self.builds = self.updates = 0
        self.rebuilt = False
        self.mol_of_node = None
        self._g = None
        self._ws = self._stats = None
        self._set_box(lo, hi, periodic, cell, origin)

    # ---- box -----------------------------------------------------------------------------------------------------------
    def _set_box(self, lo, hi, periodic, cell, origin):
        R = self.r + self.skin
        extent = 0.0
        mask = 7  # a cell is periodic along its three lattice vectors
        if cell is not None:
            if lo is not None or hi is not None or not (periodic is False or periodic is None):
                raise ValueError("cell= describes the whole periodic cell: it cannot be combined with lo / hi / periodic")
            if self.batch is not None:
                raise ValueError("batch= lays the molecules out in an open box: it cannot be combined with cell=")
            c9, o3, hgt, _ = cell_params(cell, origin)
            cell_check_cutoff(hgt, R)
            extent = max(abs(o3[c]) + sum(abs(c9[3 * a + c]) for a in range(3)) for c in range(3))
        else:
            if origin is not None:
                raise ValueError("origin= is the corner of a cell=; it needs cell=")
            mask = periodic_mask(periodic, R, lo, hi)
            if self.batch is not None and (mask or lo is not None or hi is not None):
                raise ValueError("batch= lays the molecules out in an open box of its own: it cannot be combined with "
                                 "lo / hi / periodic")
            if (lo is None) != (hi is None):
                raise ValueError("lo and hi come together")
            if lo is not None:
                if len(lo) != 3 or len(hi) != 3:
                    raise ValueError("lo and hi must have 3 entries")
                extent = max(abs(float(v)) for v in list(lo) + list(hi))
        self._box = dict(lo=lo, hi=hi, periodic=periodic, cell=cell, origin=origin)
        self._extent = extent
        self._mask = mask
        self._g = None

    def set_box(self, lo=None, hi=None, cell=None, origin=None):
        """Replace the box (``lo`` / ``hi``, the periodic axes stay) or the cell (``cell`` / ``origin``) and invalidate:
        the next update rebuilds (variable-cell relaxations).  A list keeps its kind: one made with ``cell=`` takes a new
        ``cell=``, one made with ``lo`` / ``hi`` a new ``lo`` / ``hi`` -- ``ValueError`` otherwise, and the list is left as
        it was."""
        if self._box["cell"] is not None:
            if cell is None or lo is not None or hi is not None:
                raise ValueError("this list was made with cell=: set_box takes a new cell= (and origin=), not lo / hi")
            periodic = False
        else:
            if cell is not None or origin is not None:
                raise ValueError("this list was made with lo / hi: set_box takes a new lo / hi, not cell= / origin=")
            periodic = self._box["periodic"]
        self._set_box(lo, hi, periodic, cell, origin)

    @property
    def fully_periodic(self) -> bool:
        """Whether the list's box is periodic on all three axes (a cell always is): what a stress needs."""
        return self._mask == 7

    @property
    def stored(self):
        """The stored graph at ``r + skin`` (None before the first build and after ``invalidate`` / ``set_box``)."""
        return self._g

    def invalidate(self):
        """Drop the stored graph: the next update rebuilds."""
        self._g = None

    # ---- build ---------------------------------------------------------------------------------------------------------
    def _build(self, pos):
        R = self.r + self.skin
        b = self._box
        extent = self._extent
        if self.batch is not None:
            from .batched import batched_radius_graph
            g, self.mol_of_node = batched_radius_graph(pos, self.batch, R)
            # the builder ran on the lattice copy of the molecules: its coordinates reach the far corner of the grid, which
            # is below (n_a + 1) cells of width 1.0001 R (1000 R where the grid is clamped: batched_radius_graph's limit)
            extent = max((n + 1) * 1.0001 * R if n < 256 else 1000.0 * R for n in g.grid[0])
        elif b["cell"] is not None:
            g = radius_graph(pos, R, cell=b["cell"], origin=b["origin"])
        else:
            g = radius_graph(pos, R, b["lo"], b["hi"], b["periodic"])
        N = pos.shape[0]
        if N:
            X = max(float(pos.abs().max().item()), extent)
            if not X <= MAX_COORD_OVER_SKIN * self.skin:
                raise ValueError(f"NeighborList: coordinates of magnitude {X} against skin = {self.skin}: the fp32 rounding "
                                 f"of the displacements is only covered up to {MAX_COORD_OVER_SKIN} skin (or a position is "
                                 "not finite); shift the origin, enlarge the skin or use radius_graph")
        self._g = g
        self.builds += 1
        lib = _lib.load()
        wbytes = lib.e3_nl_workspace_bytes(N)
        if wbytes < 0:
            raise RuntimeError("e3_nl_workspace_bytes: invalid arguments")
        if self._ws is None or self._ws.numel() < wbytes or self._ws.device != pos.device:
            self._ws = torch.empty(max(int(wbytes), 16), dtype=torch.uint8, device=pos.device)
            self._stats = torch.zeros(2, dtype=torch.int32, device=pos.device)

    # ---- prune ---------------------------------------------------------------------------------------------------------
    def _prune(self, pos):
        """The stored graph cut down to r at ``pos`` -> (RadiusGraph, max_i d2_i as a float; nan for a non-finite one)."""
        g = self._g
        N, E, dev = pos.shape[0], g.num_edges, pos.device
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            pos4 = torch.empty((N, 4), dtype=torch.float32, device=dev)
            rowptr = torch.empty(N + 1, dtype=torch.int32, device=dev)
            src = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
            dst = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
            head = (pos.data_ptr(), g.perm.data_ptr(), g.pos4.data_ptr(), g.rowptr.data_ptr(), g.src.data_ptr(), N, E, self.r)
            tail = (pos4.data_ptr(), rowptr.data_ptr(), src.data_ptr(), dst.data_ptr(), self._stats.data_ptr(),
                    self._ws.data_ptr(), stream)
            name, pbc = g.entry("e3_nl_update")
            _lib.call(name, *head, *pbc, *tail)
            bits, kept = self._stats.tolist()  # the one host read of an update
        maxd2 = struct.unpack("<f", struct.pack("<I", bits & 0xffffffff))[0]
        out = RadiusGraph(g.perm, pos4, rowptr, src[:kept], kept, g.grid, g.box, g.cell, g.origin, g.volume)
        object.__setattr__(out, "_dst", dst[:kept])
        return out, maxd2

    def update(self, pos: torch.Tensor) -> RadiusGraph:
        """pos [N,3] fp32 on a ROCm device (caller order; periodic coordinates may be unwrapped) -> the RadiusGraph at
        radius ``r`` for these positions, in the stored graph's node order (``perm`` is the stored one while the list
        holds).  Rebuilds when there is no stored graph, when ``N`` or the device changed, or when a particle has moved
        ``skin / 2`` since the build."""
        pos = _check_pos(pos)
        self.updates += 1
        self.rebuilt = False
        g = self._g
        if g is None or g.perm.numel() != pos.shape[0] or g.perm.device != pos.device:
            self._build(pos)
            self.rebuilt = True
        while True:
            out, maxd2 = self._prune(pos)
            if maxd2 < self.threshold:
                return out
            if self.rebuilt:
                raise RuntimeError("NeighborList: a displacement of the freshly built list is not below skin / 2: a "
                                   "position is not finite")
            self._build(pos)
            self.rebuilt = True

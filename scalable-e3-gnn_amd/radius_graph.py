"""Radius graph on the GPU (host side of ``e3_rg_*`` in include/e3gnn.h).

Builder-defined stage (no reference code in the mount): particles are renumbered by
a stable Morton sort, edges ``(src=j -> dst=i)`` exist iff ``i != j`` and ``|x_i-x_j|^2 <= r^2`` in
explicitly rounded fp32, and the result is CSR-by-dst with ascending ``src``.

Periodic boxes (``periodic=``, per axis): coordinates are wrapped into ``[lo, hi)`` and the edge test takes the minimum
image (definitions in include/e3gnn.h, ``e3_rg_sort_count_pbc``); the graph then carries ``box`` and every edge stage
downstream (geometry, message kernels, forces) uses the minimum-image edge vector.

General (triclinic) cells (``cell=``, rows = lattice vectors, periodic on all three): coordinates are wrapped into the cell
and the grid runs over the fractional coordinates scaled by the perpendicular heights (``e3_rg_sort_count_cell``); the
graph then carries ``cell`` / ``origin`` / ``volume`` instead of ``box`` and every edge stage selects its ``*_cell`` entry.

Capped rows (``max_neighbors=k``, any of the three periodicities): the count pass is followed by ``e3_rg_cap_rowptr`` and
``e3_rg_fill_nearest*`` instead of ``e3_rg_fill*``; every node keeps its k nearest neighbours inside ``r`` and the graph is
directed (include/e3gnn.h, "Capped rows").
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import torch

from . import _lib


class RgParams(ctypes.Structure):
    _fields_ = [("lo", ctypes.c_float * 3), ("hi", ctypes.c_float * 3), ("r", ctypes.c_float),
                ("n", ctypes.c_int32 * 3), ("inv", ctypes.c_float * 3), ("bits", ctypes.c_int32)]


@dataclass
class RadiusGraph:
    perm: torch.Tensor      # [N] int32   new id -> original id
    pos4: torch.Tensor      # [N,4] fp32  positions in new order (x,y,z,0)
    rowptr: torch.Tensor    # [N+1] int32 CSR by dst
    src: torch.Tensor       # [E] int32   ascending inside each row
    num_edges: int
    grid: tuple
    box: tuple | None = None  # (L_x, L_y, L_z), 0.0 on an open axis; None = open box (and on a cell graph)
    cell: tuple | None = None    # 9 fp32-exact floats, row-major, rows = lattice vectors; None = no general cell
    origin: tuple | None = None  # 3 fp32-exact floats: the corner of the cell (None without a cell)
    volume: float | None = None  # |det cell| (fp32-exact; None without a cell)
    max_neighbors: int | None = None  # the cap k of a capped graph (rows = the k nearest inside r); None = every pair
    truncated: int = 0                # rows cut by the cap (0 uncapped)
    full_edges: int | None = None     # the uncapped edge count (None = num_edges: the graph is uncapped)

    def __post_init__(self):
        if self.full_edges is None:
            self.full_edges = self.num_edges

    @property
    def cell_arg(self):
        """The ``cell`` as the ``float[9]`` argument of the ``*_cell`` entries (None without a cell)."""
        return None if self.cell is None else _lib.Float9(*self.cell)

    @property
    def box_arg(self):
        """The ``box`` as the ``float[3]`` argument of the ``*_pbc`` entries (None for an open box)."""
        return None if self.box is None else _lib.Float3(*self.box)

    @property
    def periodic(self) -> bool:
        """Whether edge vectors are minimum images (a box with a periodic axis, or a cell)."""
        return self.cell is not None or self.box is not None

    def entry(self, name: str, strained: bool = False):
        """The edge-stage entry of this graph's periodicity -> (``name`` + ``""`` | ``"_pbc"`` | ``"_cell"``, the host
        arguments that entry takes for it: none, the box, or the cell).  The strained entries come in two forms only:
        the un-suffixed one takes the box or NULL, ``_cell`` the cell."""
        if self.cell is not None:
            return name + "_cell", (self.cell_arg,)
        if strained:
            return name, (self.box_arg,)
        if self.box is not None:
            return name + "_pbc", (self.box_arg,)
        return name, ()

    @property
    def dst(self) -> torch.Tensor:
        """[E] int32 destination of every edge (expanded from rowptr once, then cached)."""
        d = getattr(self, "_dst", None)
        if d is None:
            n = self.rowptr.numel() - 1
            deg = (self.rowptr[1:] - self.rowptr[:-1]).long()
            d = torch.repeat_interleave(torch.arange(n, device=self.src.device, dtype=torch.int32), deg,
                                        output_size=self.num_edges)
            object.__setattr__(self, "_dst", d)
        return d


def grid_params(lo, hi, r) -> RgParams:
    p = RgParams()
    for a in range(3):
        p.lo[a], p.hi[a] = float(lo[a]), float(hi[a])
    p.r = float(r)
    _lib.check(_lib.load().e3_rg_grid(ctypes.byref(p)), "e3_rg_grid")
    return p


def periodic_mask(periodic, r, lo, hi) -> int:
    """Axis bit mask of ``periodic`` (bool or 3 bools), checked against the box: ``ValueError`` for a wrong-length mask, a
    missing ``lo`` / ``hi`` or ``2 r >= L`` on a periodic axis (L = hi - lo in fp32)."""
    if isinstance(periodic, (bool, int)) or periodic is None:
        axes = [bool(periodic)] * 3
    else:
        axes = [bool(a) for a in periodic]
        if len(axes) != 3:
            raise ValueError(f"periodic must be a bool or 3 bools, got {len(axes)}")
    mask = sum(1 << a for a in range(3) if axes[a])
    if mask == 0:
        return 0
    if lo is None or hi is None:
        raise ValueError("a periodic radius graph needs lo and hi: the box cannot be inferred from the points")
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError("lo and hi must have 3 entries")
    r32 = ctypes.c_float(r).value
    for a in range(3):
        if axes[a]:
            L = ctypes.c_float(ctypes.c_float(hi[a]).value - ctypes.c_float(lo[a]).value).value
            if not L > 0.0 or not 2.0 * r32 < L:
                raise ValueError(f"periodic axis {a}: need 0 < 2 r < L = hi - lo, got r = {r}, L = {L}")
    return mask


def cell_from_lengths_angles(a, b, c, alpha, beta, gamma):
    """The cell (3 rows = lattice vectors, lower-triangular) of lengths ``a, b, c`` and angles ``alpha`` (between b and
    c), ``beta`` (a, c), ``gamma`` (a, b) in degrees: a_0 along x, a_1 in the xy plane, a_2 with a positive z.
    ``ValueError`` when the angles do not span a volume."""
    import math
    try:
        a, b, c, alpha, beta, gamma = (float(v) for v in (a, b, c, alpha, beta, gamma))
    except (TypeError, ValueError):
        raise ValueError(f"lengths and angles must be numbers, got {a, b, c} and {alpha, beta, gamma}") from None
    # a residue of cos() below 5e-16 is cut off, which makes the cosines of 60, 90 and 120 degrees exactly 0 and +-1/2;
    # every other angle moves by at most that much
    ca, cb, cg = (round(math.cos(math.radians(v)), 15) for v in (alpha, beta, gamma))
    sg = math.sqrt(max(0.0, 1.0 - cg * cg))
    if not (min(a, b, c) > 0.0) or not sg > 0.0:
        raise ValueError(f"lengths must be positive and gamma inside (0, 180), got {a, b, c} and gamma = {gamma}")
    cx = cb
    cy = (ca - cb * cg) / sg
    cz2 = 1.0 - cx * cx - cy * cy
    if not cz2 > 0.0:
        raise ValueError(f"angles {alpha, beta, gamma} do not span a cell (the three vectors would be coplanar)")
    return [[a, 0.0, 0.0], [b * cg, b * sg, 0.0], [c * cx, c * cy, c * math.sqrt(cz2)]]


def cell_params(cell, origin=None):
    """``cell`` (3x3 nested sequence or CPU tensor; rows = lattice vectors) and ``origin`` as fp32-exact floats, with what
    the library derives from them -> (cell9, origin3, heights3, volume).  ``ValueError`` for a wrong shape or a cell that is
    singular or not finite."""
    if isinstance(cell, torch.Tensor):
        if cell.is_cuda:
            raise ValueError("cell must be a nested sequence or a CPU tensor (it is a host argument of the kernels)")
        cell = cell.detach().tolist()
    rows = [list(row) if hasattr(row, "__len__") else None for row in cell] if hasattr(cell, "__len__") else None
    if rows is None or len(rows) != 3 or any(row is None or len(row) != 3 for row in rows):
        raise ValueError("cell must be 3 x 3: one lattice vector per row")
    if isinstance(origin, torch.Tensor):
        origin = origin.detach().cpu().tolist()
    origin = [0.0, 0.0, 0.0] if origin is None else list(origin)
    if len(origin) != 3:
        raise ValueError("origin must have 3 entries")
    c9 = _lib.Float9(*[float(v) for row in rows for v in row])
    o3 = _lib.Float3(*[float(v) for v in origin])
    ginv, hgt, vol = _lib.Float9(), _lib.Float3(), ctypes.c_float()
    if _lib.load().e3_cell_derive(c9, ginv, hgt, ctypes.byref(vol)) != _lib.E3_OK or \
            not all(abs(v) < 3.0e38 for v in o3):
        raise ValueError(f"cell {[list(row) for row in rows]} is singular or not finite (or the origin is not finite)")
    return tuple(c9), tuple(o3), tuple(hgt), vol.value


def cell_check_cutoff(heights, r):
    """``ValueError`` unless ``0 < 2 r < min height`` in fp32 (the unique-image condition of the ``*_cell`` entries)."""
    r32 = ctypes.c_float(r).value
    if not r32 > 0.0 or not all(ctypes.c_float(2.0 * r32).value < h for h in heights):
        raise ValueError(f"cell: need 0 < 2 r < the smallest perpendicular height, got r = {r}, heights = "
                         f"{tuple(heights)}")


def _check_pos(pos):
    if not pos.is_cuda:
        raise RuntimeError("radius_graph runs on ROCm tensors only; there is no CPU path")
    if pos.dtype != torch.float32 or pos.dim() != 2 or pos.shape[1] != 3:
        raise RuntimeError(f"pos must be [N,3] float32, got {tuple(pos.shape)} {pos.dtype}")
    return pos.contiguous()


def _edge_count(rowptr, N) -> int:
    """E = rowptr[N], read together with the smallest degree: the count / scan run in int32 (indices are int32 end to end),
    so a graph with >= 2^31 edges wraps the running sum, which shows as a negative or decreasing rowptr."""
    if N > 0:
        E, mindeg = torch.stack([rowptr[-1], (rowptr[1:] - rowptr[:-1]).min()]).tolist()
    else:
        E, mindeg = int(rowptr[-1].item()), 0
    if E < 0 or mindeg < 0:
        raise RuntimeError("radius_graph: the edge count does not fit int32 (>= 2^31 edges); shard the cloud "
                           "(sharding.SlabHalo) or reduce the cutoff")
    return int(E)


MAX_NEIGHBORS_LIMIT = 64  # one candidate per lane of the wave that selects a capped row (e3_rg_fill_nearest)


def check_max_neighbors(max_neighbors):
    """``None`` or an int in [1, 64] (``bool`` is not an int here); ``ValueError`` otherwise."""
    if max_neighbors is None:
        return None
    if isinstance(max_neighbors, bool) or not isinstance(max_neighbors, int) or \
            not 1 <= max_neighbors <= MAX_NEIGHBORS_LIMIT:
        raise ValueError(f"max_neighbors must be None or an int in [1, {MAX_NEIGHBORS_LIMIT}], got {max_neighbors!r}")
    return max_neighbors


def _capped_counts(rowptr, stats, N):
    """One host read of a capped build -> (E, rows cut, full edge count).  The int32 guard of ``_edge_count`` applies to the
    capped count: a capped degree is in [0, k], so a wrapped running sum shows as a negative E or a decreasing rowptr."""
    mindeg = (rowptr[1:] - rowptr[:-1]).min() if N > 0 else rowptr[-1] * 0
    E, mindeg, cut, full = torch.cat([torch.stack([rowptr[-1], mindeg]).long(), stats]).tolist()
    if E < 0 or mindeg < 0:
        raise RuntimeError("radius_graph: the capped edge count does not fit int32 (>= 2^31 edges); shard the cloud "
                           "(sharding.SlabHalo) or lower max_neighbors")
    return int(E), int(cut), int(full)


def radius_graph(pos: torch.Tensor, r: float, lo=None, hi=None, periodic=False, cell=None, origin=None,
                 max_neighbors=None) -> RadiusGraph:
    """pos [N,3] fp32 on a ROCm device.  ``lo``/``hi``: bounding box (computed from pos when omitted).

    ``max_neighbors`` (None or an int k in [1, 64]): cap every node at its k nearest neighbours inside ``r``.  A row with at
    most k neighbours is unchanged; a longer row keeps the k sources with the smallest ``(d2, id)`` -- the fp32 ``d2`` of the
    edge test, ties to the lower new id -- still in ascending id (include/e3gnn.h, "Capped rows").  The capped graph is
    DIRECTED: ``j -> i`` can exist without ``i -> j``.  The graph records ``max_neighbors``, ``truncated`` (rows cut) and
    ``full_edges`` (the uncapped count, which may exceed int32: only the capped count has to fit).  ``ValueError`` for
    anything else; None is the uncapped call, launch for launch.

    ``periodic``: bool or 3 bools; periodic axes wrap at ``[lo, hi)`` (then ``lo`` / ``hi`` are required and
    ``2 r < hi - lo``).  Positions may lie outside the box on those axes; ``pos4`` holds them wrapped.

    ``cell`` (3x3 nested sequence or CPU tensor, rows = lattice vectors, the ASE convention) with ``origin`` (default
    (0,0,0)): a general cell, periodic on all three directions; needs ``2 r <`` every perpendicular height and excludes
    ``lo`` / ``hi`` / ``periodic`` (``ValueError``).  The graph carries ``cell`` / ``origin`` / ``volume``; ``box`` stays
    None."""
    k = check_max_neighbors(max_neighbors)
    if cell is not None:
        if lo is not None or hi is not None or not (periodic is False or periodic is None):
            raise ValueError("cell= describes the whole periodic cell: it cannot be combined with lo / hi / periodic")
        c9, o3, hgt, vol = cell_params(cell, origin)
        cell_check_cutoff(hgt, r)
        pos = _check_pos(pos)
        p = grid_params([0.0, 0.0, 0.0], hgt, r)  # the open grid of q = s * heights in [0, h)
        suffix, extra = "_cell", (_lib.Float9(*c9), _lib.Float3(*o3))
        fields = dict(cell=c9, origin=o3, volume=vol)
    else:
        if origin is not None:
            raise ValueError("origin= is the corner of a cell=; it needs cell=")
        mask = periodic_mask(periodic, r, lo, hi)
        pos = _check_pos(pos)
        if lo is None or hi is None:
            lo = pos.min(0).values.tolist() if pos.shape[0] else [0.0, 0.0, 0.0]
            hi = pos.max(0).values.tolist() if pos.shape[0] else [1.0, 1.0, 1.0]
            hi = [h if h > l else l + 1.0 for l, h in zip(lo, hi)]
        p = grid_params(lo, hi, r)
        suffix, extra, fields = "", (), {}
        if mask:
            suffix, extra = "_pbc", (mask,)
            fields = dict(box=tuple(ctypes.c_float(p.hi[a] - p.lo[a]).value if (mask >> a) & 1 else 0.0 for a in range(3)))
    N, dev = pos.shape[0], pos.device
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        wbytes = lib.e3_rg_workspace_bytes(N, ctypes.byref(p))
        if wbytes < 0:
            raise RuntimeError("e3_rg_workspace_bytes: invalid arguments")
        ws = torch.empty(max(int(wbytes), 16), dtype=torch.uint8, device=dev)
        perm = torch.empty(N, dtype=torch.int32, device=dev)
        pos4 = torch.empty((N, 4), dtype=torch.float32, device=dev)
        rowptr = torch.empty(N + 1, dtype=torch.int32, device=dev)
        _lib.call("e3_rg_sort_count" + suffix, pos.data_ptr(), N, ctypes.byref(p), *extra, perm.data_ptr(), pos4.data_ptr(),
                  rowptr.data_ptr(), ws.data_ptr(), wbytes, stream)
        if k is None:
            E = _edge_count(rowptr, N)
            src = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
            _lib.call("e3_rg_fill" + suffix, N, ctypes.byref(p), *extra, pos4.data_ptr(), rowptr.data_ptr(), src.data_ptr(),
                      ws.data_ptr(), wbytes, stream)
        else:
            # the capped row pointer replaces the full one in place: the full degrees stay in the workspace for the fill
            cbytes = lib.e3_rg_cap_workspace_bytes(N)
            cws = torch.empty(max(int(cbytes), 16), dtype=torch.uint8, device=dev)
            stats = torch.empty(2, dtype=torch.int64, device=dev)
            _lib.call("e3_rg_cap_rowptr", rowptr.data_ptr(), N, k, rowptr.data_ptr(), stats.data_ptr(), cws.data_ptr(),
                      cbytes, stream)
            E, cut, full = _capped_counts(rowptr, stats, N)
            src = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
            _lib.call("e3_rg_fill_nearest" + suffix, N, ctypes.byref(p), *extra, pos4.data_ptr(), rowptr.data_ptr(), k,
                      src.data_ptr(), ws.data_ptr(), wbytes, stream)
            fields.update(max_neighbors=k, truncated=cut, full_edges=full)
    return RadiusGraph(perm, pos4, rowptr, src[:E], E, (tuple(p.n), p.bits), **fields)

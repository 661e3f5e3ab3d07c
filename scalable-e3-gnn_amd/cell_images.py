"""Periodic cells below twice the cutoff: explicit image rows under an OPEN graph (host side of ``e3_cell_images_*`` and
``e3_image_rows_*`` in include/e3gnn.h).

``radius_graph(cell=)`` and every ``*_cell`` kernel take the unique minimum image of an edge, which exists only while
``2 r <`` every perpendicular height of the cell.  Below that bound a pair interacts through several images -- in a one-atom
cell every neighbour is an image of the atom itself.  ``CellImages`` takes the route of the sharded path: the
cloud is extended by the lattice images that can reach the cell, ``[owned (wrapped) | images]``, the graph over it is built
open, the edges INTO image rows are dropped and the image rows of the node features are refreshed from their owners before
every layer.  Every open-graph kernel then serves the small cell as it is; the cost is extra rows, not extra edges.

``CellImages`` offers the part of the ``sharding.Halo`` interface that ``SEGNN`` and the energy models use (``refresh``,
``exchange``, ``start`` / ``finish``, ``ghost_rows``, ``owned_new``, ``overflow``, ``anchor``, ``split_graph``), without a
process group: a refresh is one row copy on the device (``e3_image_rows_expand``), its transpose one ordered row sum
(``e3_image_rows_reduce``).  ``BatchedCellImages`` is the same for a batch of structures, each with its own cell, in one
selection.  Not covered: a Verlet list over image rows, the ``lo`` / ``hi`` box form, a cell with an open direction, the
sharded path, more than ``MAX_SHELLS`` image shells on an axis."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import torch

from . import _lib
from .radius_graph import cell_params, radius_graph

MAX_SHELLS = 7   # E3_CELL_IMAGE_MAX_SHELLS: image shells per axis, m_a = ceil(rho / height_a)


@dataclass
class ImageRowMap:
    """The index state of ``ops.image_rows_expand`` / ``ops.image_rows_reduce`` for ``M`` rows in one numbering."""
    source: torch.Tensor               # [M] int32: i on an owned row, the owner's row on an image row
    ptr: torch.Tensor                  # [M + 1] int32 \ the image rows grouped by their owner (CSR),
    rows: torch.Tensor                 # [G] int32     / ascending inside a row
    shift: torch.Tensor | None = None  # [M, 3] int32 lattice shift of every row (zero on owned rows)
    cell: tuple | None = None          # 9 fp32-exact floats, rows = lattice vectors (with ``shift``)

    @staticmethod
    def build(source: torch.Tensor, shift: torch.Tensor | None = None, cell=None) -> "ImageRowMap":
        source = source.to(torch.int32).contiguous()
        M, dev = source.numel(), source.device
        src = source.long()
        img = torch.nonzero(src != torch.arange(M, device=dev)).flatten()        # ascending
        order = torch.sort(src[img], stable=True).indices                          # by owner, ascending row inside one
        ptr = torch.zeros(M + 1, dtype=torch.int32, device=dev)
        ptr[1:] = torch.cumsum(torch.bincount(src[img], minlength=M), 0)
        shift = None if shift is None else shift.to(torch.int32).contiguous()
        return ImageRowMap(source, ptr, img[order].to(torch.int32), shift, None if cell is None else tuple(cell))


def _translation(rmap, dtype, device):
    """n_i cell of every row as a [M, 3] tensor (the torch restatement's translation)"""
    cell = torch.tensor(rmap.cell, dtype=torch.float64).view(3, 3).to(device=device, dtype=dtype)
    return rmap.shift.to(dtype) @ cell


def image_rows_expand_torch(x, rmap, translate=False):
    """Torch restatement of ``e3_image_rows_expand`` (any device, any dtype): ``x[source]`` (+ ``shift @ cell``)."""
    out = x[rmap.source.long()]
    return out + _translation(rmap, x.dtype, x.device) if translate else out


def image_rows_reduce_torch(g, rmap):
    """Torch restatement of ``e3_image_rows_reduce`` (any device): every row of ``g`` added to row ``source`` of zeros."""
    return torch.zeros_like(g).index_add_(0, rmap.source.long(), g)


def _rows(t):
    """rows the kernels can address with one leading dimension: unit column stride and, above one row, a pitch of at least D
    (a row-broadcast tensor -- strides (0, 1), what the backward of ``.sum(0)`` hands over -- is materialised)"""
    return t if t.stride(-1) == 1 and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1]) else t.contiguous()


def _check_translate(x, rmap):
    if rmap.shift is None or rmap.cell is None:
        raise ValueError("translate=True needs a map built with shift= and cell=")
    if x.shape[1] != 3 or (x.is_cuda and x.dtype != torch.float32):
        raise ValueError(f"translate=True moves positions: [M,3] fp32 rows, got {tuple(x.shape)} {x.dtype}")


def image_rows_expand_raw(x, rmap, translate=False, out=None):
    """``out[i] = x[source[i]]`` (``translate``: ``+ shift[i] cell``, [M,3] fp32) -> a new contiguous [M, D] tensor, or
    ``out=x`` for the in-place form that writes the image rows only.  ROCm tensors: ``e3_image_rows_expand`` (fp32, bf16,
    fp64; row-strided views are read in place); CPU tensors: ``image_rows_expand_torch``."""
    if x.dim() != 2 or x.shape[0] != rmap.source.numel():
        raise ValueError(f"rows must be [M, D] with M = {rmap.source.numel()}, got {tuple(x.shape)}")
    if translate:
        _check_translate(x, rmap)
    if not x.is_cuda:
        res = image_rows_expand_torch(x, rmap, translate)
        return res if out is None else out.copy_(res)
    if out is None:
        x = _rows(x)
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    elif out is not x or _rows(x) is not x:
        raise ValueError("the in-place form takes out=x, rows with unit column stride and a pitch of at least D")
    M, D = x.shape
    with torch.cuda.device(x.device):
        _lib.call("e3_image_rows_expand", x.data_ptr(), max(x.stride(0), D), rmap.source.data_ptr(),
                  rmap.shift.data_ptr() if translate else None, _lib.Float9(*rmap.cell) if translate else None, M, D,
                  _lib.dtype_code(x.dtype), out.data_ptr(), max(out.stride(0), D),
                  torch.cuda.current_stream(x.device).cuda_stream)
    return out


def image_rows_reduce_raw(g, rmap):
    """``out[i] = g[i] + sum of g[j] over the image rows j of owned row i``, 0 on image rows -> a new contiguous [M, D]
    tensor.  ROCm tensors: ``e3_image_rows_reduce`` (fp32 / fp64, ascending j, no atomics); CPU: the torch restatement."""
    if g.dim() != 2 or g.shape[0] != rmap.source.numel():
        raise ValueError(f"rows must be [M, D] with M = {rmap.source.numel()}, got {tuple(g.shape)}")
    if not g.is_cuda:
        return image_rows_reduce_torch(g, rmap)
    g = _rows(g)
    M, D = g.shape
    out = torch.empty((M, D), dtype=g.dtype, device=g.device)
    G = rmap.rows.numel()
    with torch.cuda.device(g.device):
        _lib.call("e3_image_rows_reduce", g.data_ptr(), max(g.stride(0), D), rmap.source.data_ptr(), rmap.ptr.data_ptr(),
                  rmap.rows.data_ptr() if G else None, G, M, D, _lib.dtype_code(g.dtype), out.data_ptr(), D,
                  torch.cuda.current_stream(g.device).cuda_stream)
    return out


def image_shells(cell9, origin3, r):
    """-> (shells (m_0, m_1, m_2), rho) of ``e3_cell_images_plan``; ``ValueError`` for an r that is not finite and positive
    (or a cell / origin that is not finite) and above ``MAX_SHELLS`` shells on an axis."""
    m, rho = _lib.Int3(), ctypes.c_float()
    st = _lib.load().e3_cell_images_plan(_lib.Float9(*cell9), _lib.Float3(*origin3), float(r), m, ctypes.byref(rho))
    if st != _lib.E3_OK:
        raise ValueError(f"cell images: need a finite r > 0 and a finite cell and origin, got r = {r}, cell = {tuple(cell9)}, "
                         f"origin = {tuple(origin3)}")
    if max(m) > MAX_SHELLS:
        raise ValueError(f"cell images: r = {r} needs {tuple(m)} image shells, more than {MAX_SHELLS} image shells on an axis "
                         "(the limit); the cell is too small for this cutoff -- build a supercell")
    return tuple(m), rho.value


class ImageRows:
    """What ``CellImages`` and ``BatchedCellImages`` share: the index state of an extended cloud ``[owned | images]`` after its
    ``setup`` and the part of the ``sharding.Halo`` interface that ``SEGNN`` and the energy models use.  Nothing here knows a
    cell: a subclass' ``setup`` selects the images and calls ``_selected``."""

    anchor = None    # ``Halo.anchor`` keeps a refresh in every rank's backward; one process has no peer to keep waiting
    _map_cell = None  # the cell of ``ImageRowMap`` (translate=True), where one cell serves every row

    def __init__(self):
        self.n_owned = self.n_ghost = 0
        self.overflow = None
        self.map = None

    def _selected(self, N, owner, shift):
        """The state after a selection: ``owner`` [G] / ``shift`` [G,3] int32 of the images of N owned particles"""
        dev = owner.device
        self.n_owned, self.n_ghost, self.owner, self.shift = N, owner.numel(), owner, shift
        # the setup order [owned | images]: every ``renumber`` starts from it, so it can be repeated (as ``Halo.renumber``)
        self._source0 = torch.cat([torch.arange(N, device=dev), owner.long()])
        self._shift0 = torch.cat([torch.zeros((N, 3), dtype=torch.int32, device=dev), shift])
        self.renumber(torch.arange(N + owner.numel(), device=dev))

    def renumber(self, perm: torch.Tensor):
        """The graph builder renumbers the extended cloud (``perm[new] = old``, old = the order ``setup`` returned): the index
        state in the new numbering."""
        p = perm.long()
        inv = torch.empty_like(p)
        inv[p] = torch.arange(p.numel(), device=p.device)
        n = self.n_owned
        self.map = ImageRowMap.build(inv[self._source0[p]], self._shift0[p], self._map_cell)
        self.owned_new = inv[:n]              # ids of the owned particles, in the caller's order
        self._img_idx = inv[n:]               # ids of the image rows, (owner, shift) order
        self.is_ghost = torch.zeros(p.numel(), dtype=torch.bool, device=p.device)
        self.is_ghost[self._img_idx] = True
        return self

    def split_graph(self, g):
        """Drop the edges into image rows and split the rest by owned / image source (``e3_split_edges``) -> SplitGraph.
        ``g``: the open RadiusGraph of the extended cloud, after ``renumber(g.perm)``."""
        from .sharding import split_graph
        return split_graph(self.is_ghost, g)

    # -- once per layer -------------------------------------------------------------------------------
    def exchange(self, h: torch.Tensor) -> torch.Tensor:
        """Overwrite the image rows of ``h`` with their owners' rows, in place (inference: not differentiable)."""
        if torch.is_grad_enabled() and h.requires_grad:
            raise RuntimeError("the image refresh writes image rows in place: not differentiable (run under torch.no_grad(), "
                               "or use refresh)")
        return image_rows_expand_raw(h, self.map, out=h)

    def start(self, h: torch.Tensor):
        """``Halo.start``: there is no transfer to overlap, so the refresh happens here, at once."""
        self.exchange(h)
        return None

    def finish(self, h: torch.Tensor, token) -> torch.Tensor:
        return h

    def ghost_rows(self) -> torch.Tensor:
        """Graph-order ids of the image rows."""
        return self._img_idx

    def refresh(self, h: torch.Tensor) -> torch.Tensor:
        """Differentiable refresh, out of place: -> a new [M, D] tensor with the owners' rows in the image rows
        (``ops.image_rows_expand``; its backward is ``ops.image_rows_reduce`` and vice versa, to any order)."""
        from . import ops
        return ops.image_rows_expand(h, self.map)

    # -- owned <-> extended ---------------------------------------------------------------------------
    def extend(self, t: torch.Tensor, translate: bool = False) -> torch.Tensor:
        """``t`` [N, D] on the owned particles in the caller's order -> [M, D] on the extended cloud in the current
        numbering, every image row a copy of its owner's (``translate``: positions, plus the lattice shift).  Differentiable."""
        from . import ops
        full = torch.zeros((self.map.source.numel(), t.shape[1]), dtype=t.dtype, device=t.device)
        return ops.image_rows_expand(full.index_copy(0, self.owned_new, t), self.map, translate=translate)

    def reduce(self, t: torch.Tensor) -> torch.Tensor:
        """The transpose of ``extend``: ``t`` [M, D] on the extended cloud (e.g. dE/dpos_ext: an image's position is its
        owner's plus a constant) -> [N, D] in the caller's order, every particle's own row plus its images' rows, summed in
        a fixed order.  Differentiable."""
        from . import ops
        return ops.image_rows_reduce(t, self.map)[self.owned_new]


class CellImages(ImageRows):
    """The image rows of one periodic cell (``cell`` 3x3, rows = lattice vectors, with ``origin``; held as ``cell_params``
    derives them).  ``setup`` selects the images, ``renumber`` follows the graph builder's order, ``split_graph`` drops the
    edges into image rows; after that it serves ``SEGNN(..., halo=images, split=split)`` as a ``sharding.Halo`` does."""

    def __init__(self, cell, origin=None):
        super().__init__()
        self.cell, self.origin, self.heights, self.volume = cell_params(cell, origin)
        self._map_cell = self.cell

    def needs_images(self, r: float) -> bool:
        """Whether ``radius_graph(cell=)`` refuses ``r``: ``2 r >=`` a perpendicular height in fp32."""
        r32 = ctypes.c_float(r).value
        return not all(ctypes.c_float(2.0 * r32).value < h for h in self.heights)

    def setup(self, pos: torch.Tensor, feats: torch.Tensor, r: float):
        """pos [N,3] fp32 (may be unwrapped), feats [N, C] -> (pos_ext [N + G, 3], feats_ext [N + G, C]): the wrapped
        particles in caller order, then their G images ordered by (owner, shift); ``owner`` [G] / ``shift`` [G,3] int32 are
        kept.  Count pass, one scan, ONE host read (G), fill pass (``e3_cell_images_count`` / ``_fill``)."""
        self.shells, self.rho = image_shells(self.cell, self.origin, r)
        if not pos.is_cuda:
            raise RuntimeError("CellImages.setup runs on ROCm tensors only; there is no CPU path")
        if pos.dtype != torch.float32 or pos.dim() != 2 or pos.shape[1] != 3:
            raise RuntimeError(f"pos must be [N,3] float32, got {tuple(pos.shape)} {pos.dtype}")
        pos = pos.detach().contiguous()
        N, dev = pos.shape[0], pos.device
        lib = _lib.load()
        c9, o3 = _lib.Float9(*self.cell), _lib.Float3(*self.origin)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            wbytes = lib.e3_cell_images_workspace_bytes(N)
            if wbytes < 0:
                raise RuntimeError("e3_cell_images_workspace_bytes: invalid arguments")
            ws = torch.empty(max(int(wbytes), 16), dtype=torch.uint8, device=dev)
            pos_w = torch.empty((N, 3), dtype=torch.float32, device=dev)
            off = torch.empty(N + 1, dtype=torch.int32, device=dev)
            _lib.call("e3_cell_images_count", pos.data_ptr(), N, c9, o3, float(r), pos_w.data_ptr(), off.data_ptr(),
                      ws.data_ptr(), wbytes, stream)
            G = int(off[-1].item())
            owner = torch.empty(G, dtype=torch.int32, device=dev)
            shift = torch.empty((G, 3), dtype=torch.int32, device=dev)
            pos_ext = torch.empty((N + G, 3), dtype=torch.float32, device=dev)
            pos_ext[:N] = pos_w
            _lib.call("e3_cell_images_fill", pos_w.data_ptr(), N, c9, o3, float(r), off.data_ptr(), G, owner.data_ptr(),
                      shift.data_ptr(), pos_ext[N:].data_ptr() if G else None, stream)
        self._selected(N, owner, shift)
        return pos_ext, image_rows_expand_raw(_pad_rows(feats, N + G), self.map)


def _aligned_host(n_bytes):
    """a zeroed host buffer whose address is a multiple of 16 -> (the ctypes array that owns it, the address)"""
    raw = (ctypes.c_uint8 * (n_bytes + 16))()
    addr = ctypes.addressof(raw)
    return raw, addr + (-addr) % 16


class BatchedCellImages(ImageRows):
    """The image rows of a batch of periodic structures, each with its own cell: ``cells`` [B,3,3] (a nested sequence or a
    CPU tensor; rows = lattice vectors) and ``origins`` [B,3] (None: zeros), every structure derived by ``cell_params``;
    ``volumes`` holds the B volumes.  One selection serves the whole batch (``e3_cell_images_count_batch`` / ``_fill_batch``:
    the cell is looked up per particle in a table of B records), and the rest is ``CellImages``' -- except that no single cell
    translates every row, so ``extend(translate=True)`` is a ``ValueError``."""

    def __init__(self, cells, origins=None):
        super().__init__()
        if isinstance(cells, torch.Tensor):
            if cells.is_cuda:
                raise ValueError("cells must be a nested sequence or a CPU tensor (they are host arguments of the kernels)")
            cells = cells.detach().tolist()
        if isinstance(origins, torch.Tensor):
            origins = origins.detach().cpu().tolist()
        cells = list(cells)
        origins = [None] * len(cells) if origins is None else list(origins)
        if len(origins) != len(cells):
            raise ValueError(f"origins must hold one origin per cell: {len(cells)} cells, {len(origins)} origins")
        params = [cell_params(c, o) for c, o in zip(cells, origins)]
        self.n_structures = len(params)
        self.cells = [p[0] for p in params]
        self.origins = [p[1] for p in params]
        self.heights = [p[2] for p in params]
        self.volumes = [p[3] for p in params]

    def plan(self, r: float):
        """-> (shells [B] of 3-tuples, rho [B] floats) of ``e3_cell_images_plan_batch``, which are those of
        ``e3_cell_images_plan`` per structure; the host table of the device records is kept for ``setup``.  ``ValueError``
        for an r that is not finite and positive and for a structure above ``MAX_SHELLS`` shells on an axis."""
        B, lib = self.n_structures, _lib.load()
        rec = int(lib.e3_cell_images_record_bytes())
        cells = (ctypes.c_float * (9 * max(B, 1)))(*[v for c in self.cells for v in c])
        origins = (ctypes.c_float * (3 * max(B, 1)))(*[v for o in self.origins for v in o])
        shells, rho = (ctypes.c_int32 * (3 * max(B, 1)))(), (ctypes.c_float * max(B, 1))()
        self._table_owner, self._table_host = _aligned_host(rec * max(B, 1))
        self._table_bytes = rec * B
        st = lib.e3_cell_images_plan_batch(ctypes.addressof(cells), ctypes.addressof(origins), B, float(r),
                                           ctypes.addressof(shells), ctypes.addressof(rho), self._table_host)
        if st != _lib.E3_OK:
            raise ValueError(f"cell images: need a finite r > 0 and finite cells and origins, got r = {r}")
        self.shells = [tuple(shells[3 * b:3 * b + 3]) for b in range(B)]
        self.rho = [rho[b] for b in range(B)]
        for b, m in enumerate(self.shells):
            if max(m) > MAX_SHELLS:
                raise ValueError(f"cell images: structure {b}: r = {r} needs {m} image shells, more than {MAX_SHELLS} image "
                                 "shells on an axis (the limit); the cell is too small for this cutoff -- build a supercell")
        return self.shells, self.rho

    def setup(self, pos: torch.Tensor, feats: torch.Tensor, batch: torch.Tensor, r: float):
        """pos [N,3] fp32 (may be unwrapped), feats [N, C], batch [N] (any integer dtype, any order; ids in [0, B), a structure
        may have no atoms) -> (pos_ext [N + G, 3], feats_ext [N + G, C], batch_ext [N + G] int64): every particle wrapped
        into its own cell, in caller order, then the G images ordered by (owner, shift).  One read of the per-structure
        counts (which is also where an id outside [0, B) and a non-finite position are refused, before any launch of the
        selection), count pass, one scan, ONE read of G, fill pass."""
        B = self.n_structures
        self.plan(r)
        if pos.dtype != torch.float32 or pos.dim() != 2 or pos.shape[1] != 3:
            raise RuntimeError(f"pos must be [N,3] float32, got {tuple(pos.shape)} {pos.dtype}")
        if batch.dim() != 1 or batch.shape[0] != pos.shape[0] or batch.dtype.is_floating_point or batch.dtype == torch.bool:
            raise ValueError(f"batch must be [N] of an integer dtype with N = {pos.shape[0]}, got {tuple(batch.shape)} "
                             f"{batch.dtype}")
        pos = pos.detach().contiguous()
        N, dev = pos.shape[0], pos.device
        ids = batch.to(dev).long()
        outside = (ids < 0) | (ids >= B)
        tally = torch.cat([torch.bincount(torch.where(outside, B, ids), minlength=B + 1),
                           (~torch.isfinite(pos)).sum().view(1)]).tolist()
        if tally[B]:
            raise ValueError(f"batch holds {tally[B]} structure ids outside [0, {B}): cells= describes {B} structures")
        if tally[B + 1]:
            raise ValueError("pos holds non-finite coordinates")
        if not pos.is_cuda:
            raise RuntimeError("BatchedCellImages.setup runs on ROCm tensors only; there is no CPU path")
        structure = ids.to(torch.int32)
        counts = (ctypes.c_int64 * max(B, 1))(*tally[:B])
        lib = _lib.load()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            wbytes = lib.e3_cell_images_workspace_bytes(N)
            if wbytes < 0:
                raise RuntimeError("e3_cell_images_workspace_bytes: invalid arguments")
            ws = torch.empty(max(int(wbytes), 16), dtype=torch.uint8, device=dev)
            host = torch.frombuffer(self._table_owner, dtype=torch.uint8, count=max(self._table_bytes, 16),
                                    offset=self._table_host - ctypes.addressof(self._table_owner))
            table = host.to(dev)                                  # a fresh allocation: 256-byte aligned
            pos_w = torch.empty((N, 3), dtype=torch.float32, device=dev)
            off = torch.empty(N + 1, dtype=torch.int32, device=dev)
            _lib.call("e3_cell_images_count_batch", pos.data_ptr(), structure.data_ptr(), N, table.data_ptr(),
                      self._table_host, ctypes.addressof(counts), B, pos_w.data_ptr(), off.data_ptr(), ws.data_ptr(), wbytes,
                      stream)
            G = int(off[-1].item())
            owner = torch.empty(G, dtype=torch.int32, device=dev)
            shift = torch.empty((G, 3), dtype=torch.int32, device=dev)
            pos_ext = torch.empty((N + G, 3), dtype=torch.float32, device=dev)
            pos_ext[:N] = pos_w
            _lib.call("e3_cell_images_fill_batch", pos_w.data_ptr(), structure.data_ptr(), N, table.data_ptr(),
                      self._table_host, ctypes.addressof(counts), B, off.data_ptr(), G, owner.data_ptr(), shift.data_ptr(),
                      pos_ext[N:].data_ptr() if G else None, stream)
        self._selected(N, owner, shift)
        self.counts = tally[:B]
        return pos_ext, image_rows_expand_raw(_pad_rows(feats, N + G), self.map), torch.cat([ids, ids[owner.long()]])


def _pad_rows(t, M):
    """[N, C] -> [M, C], zero rows past N (the expand overwrites them)"""
    out = torch.zeros((M,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    out[:t.shape[0]] = t
    return out


def cell_image_graph(pos: torch.Tensor, x: torch.Tensor, r: float, cell, origin=None):
    """The extended cloud of a periodic cell of ANY size and its open graph -> ``(images, split, x_g, pos_g)``: a
    ``CellImages``, the ``SplitGraph`` without the edges into image rows, and features / positions of the extended cloud in
    the graph's order.  Use as ``net(x_g, split.graph, halo=images, split=split)``; rows ``images.owned_new`` of the result
    are the N particles in the caller's order.  ``ValueError`` above ``MAX_SHELLS`` image shells on an axis."""
    images = CellImages(cell, origin)
    pos_ext, x_ext = images.setup(pos, x, r)
    g = radius_graph(pos_ext, r)     # open, bounds from the cloud: image positions carry their lattice shift
    images.renumber(g.perm)
    split = images.split_graph(g)
    perm = g.perm.long()
    return images, split, x_ext[perm], pos_ext[perm]


def batched_cell_image_graph(pos: torch.Tensor, x: torch.Tensor, batch: torch.Tensor, r: float, cells, origins=None):
    """The extended cloud of a batch of periodic structures (``cells`` [B,3,3], ``batch`` [N] the structure of every particle)
    and its open graph -> ``(images, split, x_g, pos_g, structure_g)``: a ``BatchedCellImages``, the ``SplitGraph`` without the
    edges into image rows, features / positions of the extended cloud in the graph's order and ``structure_g`` [M] int64, the
    structure of every extended row in that order.  The graph is ``batched.batched_radius_graph`` over the extended cloud:
    intra-structure edges only, found on a lattice copy and returned with the extended positions themselves, so the edge
    vectors see no offset.  Use as ``cell_image_graph``'s result."""
    from .batched import batched_radius_graph
    images = BatchedCellImages(cells, origins)
    pos_ext, x_ext, batch_ext = images.setup(pos, x, batch, r)
    g, structure_g = batched_radius_graph(pos_ext, batch_ext, r)
    images.renumber(g.perm)
    split = images.split_graph(g)
    perm = g.perm.long()
    return images, split, x_ext[perm], pos_ext[perm], structure_g

"""Edge / node stages of the SEGNN forward (host side of ``e3_edge_geometry``, ``e3_gather_concat``,
``e3_gate``, ``e3_segment_sum`` and their ``*_backward`` in include/e3gnn.h).  Builder-defined,
fp32.  Every op is differentiable (torch.autograd.Function over the HIP backward kernels): with the tensor products'
own backward a whole SEGNN layer has parameter gradients and forces.  With grad mode on inside a backward
(``create_graph=True``) the same backward call runs as a second Function (``_*BackwardFn``) that has a backward of its own --
the linear stages by composition (gather <-> its backward, segment sum <-> its backward), the gate, the edge geometry and the
envelope on ``e3_gate_blocks_backward2``, ``e3_edge_geometry_jvp`` / ``e3_edge_geometry_hvp`` (and their ``_strained`` forms)
and ``e3_cutoff_envelope_backward2`` -- so a loss on the forces has parameter gradients and the energy has Hessian-vector
products in the positions and in a strain; those Functions are once differentiable.  ROCm tensors only; no CPU path.
The exception is the pair ``image_rows_expand`` / ``image_rows_reduce`` (image rows of a small periodic cell, cell_images.py): two
adjoint linear maps, each the other's backward, differentiable to any order, with a torch restatement for CPU tensors."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .radius_graph import RadiusGraph


def _check(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise RuntimeError(f"{name}: ROCm tensor required (no CPU path)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: float32 required, got {t.dtype}")


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _wants_grad(*ts) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


def _ptr(t):
    """the address of a tensor, None (NULL) for None"""
    return t.data_ptr() if t is not None else None


def _f32c(t):
    """a tensor as contiguous fp32, None for None"""
    return t.to(torch.float32).contiguous() if t is not None else None


def _geometry_head(pos4, g, N, *lmax):
    """the leading arguments of every edge geometry entry: (pos4, rowptr, src, N), and lmax where the entry takes it"""
    return (pos4.data_ptr(), g.rowptr.data_ptr(), g.src.data_ptr(), N, *lmax)


def _strain_tail(strain, structure):
    """the strain arguments of every ``*_strained`` entry, which follow its box or cell: (strain, structure | NULL, S)"""
    return strain.data_ptr(), _ptr(structure), strain.shape[0]


def _edge_geometry_raw(pos4, g, want_dist, want_node_attr, lmax, want_edge=True, strain=None, structure=None):
    N, E, dev = g.rowptr.numel() - 1, g.num_edges, pos4.device
    ny = (lmax + 1) ** 2
    Y = torch.empty((E, ny), dtype=torch.float32, device=dev) if want_edge else None
    d = torch.empty(E, dtype=torch.float32, device=dev) if (want_dist and want_edge) else None
    A = torch.empty((N, ny), dtype=torch.float32, device=dev) if want_node_attr else None
    if E == 0:  # nothing to launch on (an empty src has no address to hand to the library): every row is empty, A = [1, 0, ...]
        if A is not None:
            A.zero_()[:, 0] = 1.0
        return Y, d, A
    outs = (_ptr(Y), _ptr(d), _ptr(A), _stream(pos4))
    with torch.cuda.device(dev):
        if strain is not None:  # [S,3,3] contiguous fp32, structure [N] int32 | None (checked by _strain_args): the
            # minimum image of the box or cell first, then the strain
            name, pbc = g.entry("e3_edge_geometry_strained", strained=True)
            _lib.call(name, *_geometry_head(pos4, g, N, lmax), *pbc, *_strain_tail(strain, structure), *outs)
        else:  # periodic box / general cell: minimum-image edge vectors
            name, pbc = g.entry({1: "e3_edge_geometry", 2: "e3_edge_geometry_l2"}[lmax])
            _lib.call(name, *_geometry_head(pos4, g, N), *pbc, *outs)
    return Y, d, A


def _strain_args(strain, structure, g):
    """-> (strain as [S,3,3] contiguous fp32, structure as [N] contiguous int32 | None).  ValueError for a wrong shape,
    RuntimeError for a tensor that is not on a ROCm device (or a strain that is not fp32)."""
    N = g.rowptr.numel() - 1
    if tuple(strain.shape) == (3, 3):
        strain = strain.reshape(1, 3, 3)
    if strain.dim() != 3 or tuple(strain.shape[1:]) != (3, 3) or strain.shape[0] < 1:
        raise ValueError(f"strain must be [S,3,3] (S >= 1) or [3,3], got {tuple(strain.shape)}")
    if structure is not None:
        if structure.dim() != 1 or structure.shape[0] != N:
            raise ValueError(f"structure must be [N] = [{N}] (graph order), got {tuple(structure.shape)}")
        if structure.dtype.is_floating_point or structure.dtype.is_complex or structure.dtype == torch.bool:
            raise ValueError(f"structure must be an integer tensor, got {structure.dtype}")
    _check(strain, "strain")
    if structure is not None:
        if not structure.is_cuda:
            raise RuntimeError("structure: ROCm tensor required (no CPU path)")
        structure = structure.to(torch.int32).contiguous()
    return strain.contiguous(), structure


class _EdgeGeometryFn(torch.autograd.Function):
    """pos [N,3] (graph order) -> Y, d, A; backward = e3_edge_geometry_backward (dY/dpos, dd/dpos, dA/dpos).
    With a strain [S,3,3] (and structure [N] int32 | None) the strained entries run instead, and ONE backward launch
    (e3_edge_geometry_backward_strained) returns the gradients of both pos and strain."""

    @staticmethod
    def forward(ctx, pos, strain, g, lmax, structure, pos_hessian=True):
        pos4 = torch.zeros((pos.shape[0], 4), dtype=torch.float32, device=pos.device)
        pos4[:, :3] = pos
        Y, d, A = _edge_geometry_raw(pos4, g, True, True, lmax, strain=strain, structure=structure)
        ctx.g, ctx.lmax, ctx.structure = g, lmax, structure
        # the caller's pos itself (with its graph) is kept only where a second backward can use it
        ctx.pos_hessian = bool(pos_hessian)
        ctx.save_for_backward(pos4, strain, pos if (ctx.pos_hessian and ctx.needs_input_grad[0]) else None)
        return Y, d, A

    @staticmethod
    def backward(ctx, gY, gd, gA):
        pos4, strain, pos = ctx.saved_tensors
        g = ctx.g
        if torch.is_grad_enabled():  # create_graph: the backward itself is differentiated, in gY, gd, gA and -- unless the
            # caller declined (pos_hessian=False) -- in pos and strain: the saved inputs are the caller's tensors, with
            # their graph
            p = pos if pos is not None else pos4  # pos4: a constant, no position edge
            eps = strain if (strain is None or ctx.pos_hessian) else strain.detach()
            gpos, gstrain = _EdgeGeometryBackwardFn.apply(p, eps, pos4, gY, gd, gA, g, ctx.lmax, ctx.structure)
            return gpos, gstrain, None, None, None, None
        gpos, gstrain = _edge_geometry_backward_raw(pos4, strain, g, ctx.lmax, ctx.structure, gY, gd, gA)
        return gpos, gstrain, None, None, None, None


def _edge_geometry_backward_raw(pos4, strain, g, lmax, structure, gY, gd, gA):
    """-> (g_pos [N,3], g_strain | None): e3_edge_geometry_backward, or its strained form with a strain"""
    N = pos4.shape[0]
    gpos = torch.empty((N, 3), dtype=torch.float32, device=pos4.device)
    gY, gd, gA = (t.contiguous() if t is not None else None for t in (gY, gd, gA))  # no cast: autograd hands in fp32
    gstrain = None
    if g.num_edges == 0:  # no edge: the outputs do not depend on pos or strain
        return gpos.zero_(), (torch.zeros_like(strain) if strain is not None else None)
    with torch.cuda.device(pos4.device):
        head = _geometry_head(pos4, g, N, lmax)
        if strain is not None:
            gstrain = torch.empty_like(strain)
            ws = _strain_workspace(N, pos4.device)
            name, pbc = g.entry("e3_edge_geometry_backward_strained", strained=True)
            _lib.call(name, *head, *pbc, *_strain_tail(strain, structure), _ptr(gY), _ptr(gd), _ptr(gA), gpos.data_ptr(),
                      gstrain.data_ptr(), ws.data_ptr(), ws.numel(), _stream(pos4))
        else:
            name, pbc = g.entry("e3_edge_geometry_backward")
            _lib.call(name, *head, *pbc, _ptr(gY), _ptr(gd), _ptr(gA), gpos.data_ptr(), _stream(pos4))
    return gpos, gstrain


def _strain_workspace(N, device):
    """the workspace of the strained backward and of the strained Hessian (one 9-float partial per workgroup)"""
    return torch.empty(max(1, _lib.load().e3_edge_geometry_backward_strained_workspace_bytes(N)), dtype=torch.uint8,
                       device=device)


def _edge_geometry_jvp_raw(pos4, g, lmax, v, want_y=True, want_d=True, want_a=True, strain=None, structure=None,
                           xi=None):
    """Tangent of (Y, d, A) along the displacement field v [N,3] (e3_edge_geometry_jvp) -> dY | None, dd | None, dA | None.
    With a ``strain`` [S,3,3] (``structure`` int32 [N] | None): the tangent of the strained geometry along v and the strain
    tangent ``xi`` [S,3,3], either of them None = zero (e3_edge_geometry_jvp_strained)."""
    N, E, dev = pos4.shape[0], g.num_edges, pos4.device
    ny = (lmax + 1) ** 2
    if E == 0:  # nothing to launch on: no output depends on the positions
        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
        return (z(0, ny) if want_y else None), (z(0) if want_d else None), (z(N, ny) if want_a else None)
    dY = torch.empty((E, ny), dtype=torch.float32, device=dev) if want_y else None
    dd = torch.empty(E, dtype=torch.float32, device=dev) if want_d else None
    dA = torch.empty((N, ny), dtype=torch.float32, device=dev) if want_a else None
    v, xi = _f32c(v), _f32c(xi)
    with torch.cuda.device(dev):
        head = _geometry_head(pos4, g, N, lmax)
        if strain is not None:
            name, pbc = g.entry("e3_edge_geometry_jvp_strained", strained=True)
            _lib.call(name, *head, *pbc, *_strain_tail(strain, structure), _ptr(v), _ptr(xi), _ptr(dY), _ptr(dd), _ptr(dA),
                      _stream(pos4))
        else:
            name, pbc = g.entry("e3_edge_geometry_jvp")
            _lib.call(name, *head, *pbc, v.data_ptr(), _ptr(dY), _ptr(dd), _ptr(dA), _stream(pos4))
    return dY, dd, dA


def _edge_geometry_hvp_raw(pos4, g, lmax, gY, gd, gA, v):
    """h_pos [N,3] = d<v, g_pos>/dpos of the unstrained geometry backward at (gY, gd, gA), each of them a tensor or None
    (e3_edge_geometry_hvp): the Hessian of Y, d and A in the edge vector, applied to the displacement field v [N,3]."""
    N = pos4.shape[0]
    if g.num_edges == 0:  # no edge: g_pos does not depend on the positions
        return torch.zeros((N, 3), dtype=torch.float32, device=pos4.device)
    hpos = torch.empty((N, 3), dtype=torch.float32, device=pos4.device)
    gY, gd, gA = (t.contiguous() if t is not None else None for t in (gY, gd, gA))  # no cast, as in the backward
    v = _f32c(v)
    with torch.cuda.device(pos4.device):
        name, pbc = g.entry("e3_edge_geometry_hvp")
        _lib.call(name, *_geometry_head(pos4, g, N, lmax), *pbc, _ptr(gY), _ptr(gd), _ptr(gA), v.data_ptr(),
                  hpos.data_ptr(), _stream(pos4))
    return hpos


def _edge_geometry_hvp_strained_raw(pos4, strain, g, lmax, structure, gY, gd, gA, v, xi, want_pos=True, want_strain=True):
    """(h_pos [N,3] | None, h_strain [S,3,3] | None) = the derivative of <v, g_pos> + <xi, g_strain> of the strained geometry
    backward at (gY, gd, gA) in (pos, strain) (e3_edge_geometry_hvp_strained); ``v`` [N,3] or ``xi`` [S,3,3] may be None
    (zero), not both."""
    N, dev = pos4.shape[0], pos4.device
    hpos = torch.empty((N, 3), dtype=torch.float32, device=dev) if want_pos else None
    hstrain = torch.empty_like(strain) if want_strain else None
    if g.num_edges == 0:  # no edge: neither gradient depends on pos or strain
        return (hpos.zero_() if want_pos else None), (hstrain.zero_() if want_strain else None)
    gY, gd, gA, v, xi = (_f32c(t) for t in (gY, gd, gA, v, xi))
    with torch.cuda.device(dev):
        ws = _strain_workspace(N, dev)
        name, pbc = g.entry("e3_edge_geometry_hvp_strained", strained=True)
        _lib.call(name, *_geometry_head(pos4, g, N, lmax), *pbc, *_strain_tail(strain, structure), _ptr(gY), _ptr(gd),
                  _ptr(gA), _ptr(v), _ptr(xi), _ptr(hpos), _ptr(hstrain), ws.data_ptr(), ws.numel(), _stream(pos4))
    return hpos, hstrain


class _EdgeGeometryBackwardFn(torch.autograd.Function):
    """The backward of ``_EdgeGeometryFn``, unstrained (``strain`` None) or strained, as a differentiable op of (pos, strain,
    gY, gd, gA) -> (g_pos, g_strain | None).  It is linear in the three gradients, so its backward in them is the tangent of
    the forward along the cotangents (v, Xi) of (g_pos, g_strain) (``e3_edge_geometry_jvp`` / ``_jvp_strained``); in the
    positions and the strain it is the Hessian of Y, d and A in the edge vector applied to those cotangents
    (``e3_edge_geometry_hvp`` / ``_hvp_strained``), launched only when ``pos`` or ``strain`` requires grad -- a parameter
    gradient of a loss on energies, forces and stress never needs it, and that path (``pos_hessian=False``) hands in constants
    in their place.  Either cotangent may be absent (None: zeros).  ``pos4`` is the padded copy of ``pos`` the kernels read."""

    @staticmethod
    def forward(ctx, pos, strain, pos4, gY, gd, gA, g, lmax, structure):
        ctx.g, ctx.lmax, ctx.structure = g, lmax, structure
        ctx.set_materialize_grads(False)
        gY, gd, gA = gY.contiguous(), gd.contiguous(), gA.contiguous()  # autograd hands in zeros for an unused output
        ctx.hessian = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        if ctx.hessian:
            ctx.save_for_backward(pos4, strain, gY, gd, gA)
        else:
            ctx.save_for_backward(pos4, strain)
        return _edge_geometry_backward_raw(pos4, strain, g, lmax, structure, gY, gd, gA)

    @staticmethod
    @once_differentiable
    def backward(ctx, v, xi):
        pos4, strain, *grads = ctx.saved_tensors
        g, lmax, sid = ctx.g, ctx.lmax, ctx.structure
        if v is None and xi is None:
            return (None,) * 9
        want = ctx.needs_input_grad
        hpos = hstrain = None
        if strain is None:
            dY, dd, dA = _edge_geometry_jvp_raw(pos4, g, lmax, v, *want[3:6])
            if want[0]:
                hpos = _edge_geometry_hvp_raw(pos4, g, lmax, *grads, v)
        else:
            strain = strain.detach()
            dY, dd, dA = _edge_geometry_jvp_raw(pos4, g, lmax, v, *want[3:6], strain=strain, structure=sid, xi=xi)
            if ctx.hessian:
                hpos, hstrain = _edge_geometry_hvp_strained_raw(pos4, strain, g, lmax, sid, *grads, v, xi, want[0], want[1])
        return hpos, hstrain, None, dY, dd, dA, None, None, None


def edge_geometry(g: RadiusGraph, want_dist=True, want_node_attr=True, lmax: int = 1, pos: torch.Tensor | None = None,
                  want_edge=True, strain: torch.Tensor | None = None, structure: torch.Tensor | None = None,
                  pos_hessian: bool = True):
    """-> Y [E,(lmax+1)^2] | None, d [E] | None, A [N,(lmax+1)^2] | None.  ``want_edge=False``: only the node attribute
    (the fused message kernel computes the spherical harmonics of its edges itself).

    ``pos`` [N,3] (graph order, i.e. ``original_pos[g.perm]``): when given and it requires grad, the three outputs are
    differentiable w.r.t. it (forces = -dE/dpos); otherwise the graph's own ``pos4`` is used.  A periodic graph
    (``g.box``, or a general cell ``g.cell``) takes the minimum image of every edge vector, so ``pos`` may be the
    unwrapped coordinates (moved by whole periods / lattice vectors).

    Second derivatives: under ``create_graph=True`` the gradient w.r.t. ``pos`` is itself differentiable, once: w.r.t. the
    gradients of Y, d and A that produced it (``e3_edge_geometry_jvp``) -- what the parameter gradient of a loss on the forces
    needs -- and w.r.t. ``pos`` (``e3_edge_geometry_hvp``: the Hessian of Y, d, A in the edge vector), so d(forces)/d(pos)
    taken through it is the full second derivative on the edge set of ``g``.  ``pos_hessian=False`` declines the second of
    the two: the gradient is then treated as a function of the three gradients alone and ``pos`` receives only what flows
    through them -- for a caller that differentiates w.r.t. parameters only and has no use for a gradient in its position
    leaf (the force-loss step of the energy models).  With a ``strain`` the gradients w.r.t. ``pos`` and ``strain`` are
    differentiable in the same way, once, in all five of (gY, gd, gA, pos, strain): the tangent along the cotangents (v, Xi) of
    (g_pos, g_strain) is ``e3_edge_geometry_jvp_strained`` and the derivative in ``pos`` and ``strain`` is
    ``e3_edge_geometry_hvp_strained`` -- together the second derivative of an energy in the joint coordinates (pos, strain):
    force constants, the force-strain coupling and the Born elastic term.  ``pos_hessian=False`` then hands in constants for
    both ``pos`` and ``strain`` (the parameter gradient of a loss on the stress needs the tangent only).

    ``strain`` [S,3,3] (or [3,3]: one structure), fp32 on the device, and ``structure`` [N] integer structure id of every
    row (graph order; None = every row is structure 0): every edge vector r of structure s (the structure of its dst row)
    becomes r + strain[s] r before Y, d and A are formed (include/e3gnn.h, e3_edge_geometry_strained).  When ``pos`` or
    ``strain`` requires grad, the outputs are differentiable w.r.t. both (virial = -dE/dstrain at strain = 0, stress =
    dE/dstrain / V); a strain without grad still deforms the forward.  ``strain=None`` is the unstrained call."""
    _check(g.pos4, "pos4")
    if strain is None:
        if structure is not None:
            raise ValueError("structure= is the structure of each row for a strain=; it needs strain=")
        if pos is not None and _wants_grad(pos):
            _check(pos, "pos")
            return _EdgeGeometryFn.apply(pos, None, g, lmax, None, pos_hessian)
        pos4 = g.pos4
        if pos is not None:
            pos4 = torch.zeros_like(g.pos4)
            pos4[:, :3] = pos
        return _edge_geometry_raw(pos4, g, want_dist, want_node_attr, lmax, want_edge)
    eps, sid = _strain_args(strain, structure, g)
    if pos is not None:
        _check(pos, "pos")
    if _wants_grad(pos, strain):
        return _EdgeGeometryFn.apply(pos if pos is not None else g.pos4[:, :3], eps, g, lmax, sid, pos_hessian)
    pos4 = g.pos4
    if pos is not None:
        pos4 = torch.zeros_like(g.pos4)
        pos4[:, :3] = pos
    return _edge_geometry_raw(pos4, g, want_dist, want_node_attr, lmax, want_edge, strain=eps, structure=sid)


class _GatherConcatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, extra, g):
        ctx.g, ctx.has_extra = g, extra is not None
        ctx.D, ctx.nx = h.shape[1], (extra.shape[1] if extra is not None else 0)  # extra: [E, n_extra] (gather_concat)
        return _gather_concat_raw(h, g, extra)

    @staticmethod
    def backward(ctx, gm):
        g, D, nx = ctx.g, ctx.D, ctx.nx
        if torch.is_grad_enabled():  # create_graph: the (linear) backward is differentiated in gm
            gh, gx = _GatherConcatBackwardFn.apply(gm, g, D, nx)
            return gh, gx, None
        gh, gx = _gather_concat_backward_raw(gm, g, D, nx)
        return gh, gx, None


def _gather_concat_backward_raw(gm, g, D, nx):
    """gm [E, 2D+nx] -> (g_h [N,D], g_extra [E,nx] | None): e3_gather_concat_backward"""
    gm = gm.contiguous()
    N = g.rowptr.numel() - 1
    gh = torch.empty((N, D), dtype=torch.float32, device=gm.device)
    gx = torch.empty((g.num_edges, nx), dtype=torch.float32, device=gm.device) if nx else None
    if g.num_edges == 0:  # no edge: nothing reaches h (an empty tensor has no address to hand to the library)
        return gh.zero_(), gx
    with torch.cuda.device(gm.device):
        _lib.check(_lib.load().e3_gather_concat_backward(gm.data_ptr(), gm.stride(0), D, g.rowptr.data_ptr(),
                                                         g.src.data_ptr(), N, nx, gh.data_ptr(), gh.stride(0),
                                                         gx.data_ptr() if gx is not None else None, _stream(gm)),
                   "e3_gather_concat_backward")
    return gh, gx  # gx [E, nx]: the shape _GatherConcatFn was given


class _GatherConcatBackwardFn(torch.autograd.Function):
    """gm -> (g_h, g_extra | None), linear: its backward is the forward gather on the cotangents,
    cot(gm) = [c_gh[dst] | c_gh[src] | c_gx]."""

    @staticmethod
    def forward(ctx, gm, g, D, nx):
        ctx.g, ctx.nx = g, nx
        return _gather_concat_backward_raw(gm, g, D, nx)

    @staticmethod
    @once_differentiable
    def backward(ctx, c_gh, c_gx):
        return _gather_concat_raw(c_gh.contiguous(), ctx.g, c_gx if ctx.nx else None), None, None, None


def _extra_columns(extra, E):
    """extra [E] or [E, ...] -> [E, n_extra]; E = 0 has no -1 to infer: the width is that of the trailing dimensions"""
    if E == 0:
        nx = 1
        for s in extra.shape[1:]:
            nx *= s
        return extra.reshape(0, nx)
    return extra.reshape(E, -1)


def _gather_concat_raw(h, g, extra):
    if h.stride(-1) != 1:
        h = h.contiguous()
    N, D = h.shape
    E = g.num_edges
    nx = 0
    if extra is not None:
        extra = _extra_columns(extra, E).contiguous()
        nx = extra.shape[1]
    out = torch.empty((E, 2 * D + nx), dtype=torch.float32, device=h.device)
    if E == 0:  # nothing to launch on: the empty result has no address to hand to the library
        return out
    with torch.cuda.device(h.device):
        _lib.check(_lib.load().e3_gather_concat(h.data_ptr(), h.stride(0), D, g.rowptr.data_ptr(), g.src.data_ptr(), N,
                                                extra.data_ptr() if nx else None, nx, out.data_ptr(), out.stride(0),
                                                _stream(h)), "e3_gather_concat")
    return out


def gather_concat(h: torch.Tensor, g: RadiusGraph, extra: torch.Tensor | None = None) -> torch.Tensor:
    """[E, 2D+n_extra] = [h[dst] | h[src] | extra]  (differentiable w.r.t. h and extra)"""
    _check(h, "h")
    if extra is not None:
        _check(extra, "extra")
    if _wants_grad(h, extra):
        ex2 = _extra_columns(extra, g.num_edges) if extra is not None else None
        return _GatherConcatFn.apply(h, ex2, g)
    return _gather_concat_raw(h, g, extra)


class _GateBlocksFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ns, blocks):
        ctx.ns, ctx.blocks = ns, blocks
        ctx.save_for_backward(x)
        return _gate_blocks_raw(x, ns, blocks)

    @staticmethod
    def backward(ctx, go):
        (x,) = ctx.saved_tensors
        if torch.is_grad_enabled():  # create_graph: the backward is differentiated in x and go
            return _GateBlocksBackwardFn.apply(x, go, ctx.ns, ctx.blocks), None, None
        return _gate_blocks_backward_raw(x, go, ctx.ns, ctx.blocks), None, None


def _gate_blocks_backward_raw(x, go, ns, blocks):
    import ctypes
    go = go.contiguous()
    gi = torch.empty_like(x)
    ls = (ctypes.c_int32 * len(blocks))(*[l for l, _ in blocks])
    ms = (ctypes.c_int32 * len(blocks))(*[m for _, m in blocks])
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().e3_gate_blocks_backward(x.data_ptr(), x.stride(0), go.data_ptr(), go.stride(0),
                                                       gi.data_ptr(), gi.stride(0), x.shape[0], ns, len(blocks),
                                                       ls, ms, _stream(x)), "e3_gate_blocks_backward")
    return gi


def _gate_blocks_backward2_raw(x, go, c, ns, blocks, want_go=True, want_x=True):
    """-> (cot(go) | None, cot(x) | None) for the cotangent ``c`` of the gate backward's g_in, in one launch
    (e3_gate_blocks_backward2).  Row strides may exceed the widths (``x``, ``go``, ``c``: last dimension contiguous)."""
    import ctypes
    B = x.shape[0]
    wide = sum(m * (2 * l + 1) for l, m in blocks)
    ng = sum(m for _, m in blocks)
    cgo = torch.empty((B, ns + wide), dtype=torch.float32, device=x.device) if want_go else None
    cx = torch.empty((B, ns + ng + wide), dtype=torch.float32, device=x.device) if want_x else None
    ls = (ctypes.c_int32 * len(blocks))(*[l for l, _ in blocks])
    ms = (ctypes.c_int32 * len(blocks))(*[m for _, m in blocks])
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().e3_gate_blocks_backward2(
            x.data_ptr(), x.stride(0), go.data_ptr(), go.stride(0), c.data_ptr(), c.stride(0),
            cgo.data_ptr() if want_go else None, cgo.stride(0) if want_go else 0,
            cx.data_ptr() if want_x else None, cx.stride(0) if want_x else 0, B, ns, len(blocks), ls, ms, _stream(x)),
            "e3_gate_blocks_backward2")
    return cgo, cx


class _GateBlocksBackwardFn(torch.autograd.Function):
    """(x, go) -> g_in = e3_gate_blocks_backward; its backward is e3_gate_blocks_backward2 (silu'', sigmoid'')."""

    @staticmethod
    def forward(ctx, x, go, ns, blocks):
        ctx.ns, ctx.blocks = ns, blocks
        go = go.contiguous()
        ctx.save_for_backward(x, go)
        return _gate_blocks_backward_raw(x, go, ns, blocks)

    @staticmethod
    @once_differentiable
    def backward(ctx, c):
        x, go = ctx.saved_tensors
        if c.stride(-1) != 1:
            c = c.contiguous()
        cgo, cx = _gate_blocks_backward2_raw(x, go, c, ctx.ns, ctx.blocks, ctx.needs_input_grad[1], ctx.needs_input_grad[0])
        return cx, cgo, None, None


def gate(x: torch.Tensor, ns: int, nv: int) -> torch.Tensor:
    """[B, ns + nv + 3nv] (scalars | gates | vectors) -> [B, ns + 3nv] = [silu(s) | sigmoid(g) v]  (differentiable)"""
    _check(x, "x")
    if x.stride(-1) != 1:
        x = x.contiguous()
    B = x.shape[0]
    assert x.shape[1] == ns + 4 * nv, (x.shape, ns, nv)
    if _wants_grad(x):
        return _GateBlocksFn.apply(x, ns, ((1, nv),))
    out = torch.empty((B, ns + 3 * nv), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().e3_gate(x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), B, ns, nv,
                                       _stream(x)), "e3_gate")
    return out


class _SegmentSumFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, msg, g):
        ctx.g = g
        return _segment_sum_raw(msg, g)

    @staticmethod
    def backward(ctx, ga):
        if torch.is_grad_enabled():  # create_graph: the (linear) backward is differentiated in ga
            return _SegmentSumBackwardFn.apply(ga, ctx.g), None
        return _segment_sum_backward_raw(ga, ctx.g), None


def _segment_sum_backward_raw(ga, g):
    ga = ga.contiguous()
    N, D = ga.shape
    gm = torch.empty((g.num_edges, D), dtype=torch.float32, device=ga.device)
    if g.num_edges == 0:
        return gm
    with torch.cuda.device(ga.device):
        _lib.check(_lib.load().e3_segment_sum_backward(ga.data_ptr(), ga.stride(0), g.rowptr.data_ptr(), N, D,
                                                       gm.data_ptr(), max(gm.stride(0), D), _stream(ga)),
                   "e3_segment_sum_backward")
    return gm


class _SegmentSumBackwardFn(torch.autograd.Function):
    """ga -> g_msg[e] = ga[dst(e)], linear: its backward is the segment sum of the cotangent."""

    @staticmethod
    def forward(ctx, ga, g):
        ctx.g = g
        return _segment_sum_backward_raw(ga, g)

    @staticmethod
    @once_differentiable
    def backward(ctx, c_gm):
        return _segment_sum_raw(c_gm, ctx.g), None


def _segment_sum_raw(msg, g):
    if msg.stride(-1) != 1:
        msg = msg.contiguous()
    N = g.rowptr.numel() - 1
    D = msg.shape[1]
    if g.num_edges == 0:  # nothing to launch on: every row is empty
        return torch.zeros((N, D), dtype=msg.dtype, device=msg.device)
    agg = torch.empty((N, D), dtype=msg.dtype, device=msg.device)
    fn = "e3_segment_sum" if msg.dtype == torch.float32 else "e3_segment_sum_bf16"
    with torch.cuda.device(msg.device):
        _lib.check(getattr(_lib.load(), fn)(msg.data_ptr(), msg.stride(0), g.rowptr.data_ptr(), N, D,
                                            agg.data_ptr(), agg.stride(0), _stream(msg)), fn)
    return agg


def _segment_sum_weighted_raw(msg, w, g):
    N, D = g.rowptr.numel() - 1, msg.shape[1]
    agg = torch.empty((N, D), dtype=torch.float32, device=msg.device)
    with torch.cuda.device(msg.device):
        _lib.check(_lib.load().e3_segment_sum_weighted(msg.data_ptr(), msg.stride(0), w.data_ptr(), g.rowptr.data_ptr(), N,
                                                       D, agg.data_ptr(), agg.stride(0), _stream(msg)),
                   "e3_segment_sum_weighted")
    return agg


class _SegmentSumWeightedFn(torch.autograd.Function):
    """agg = sum_e w_e msg_e per CSR row; backward = e3_segment_sum_weighted_backward (g_msg, and g_w when w needs it)."""

    @staticmethod
    def forward(ctx, msg, w, g):
        ctx.g = g
        ctx.save_for_backward(msg, w)
        return _segment_sum_weighted_raw(msg, w, g)

    @staticmethod
    def backward(ctx, ga):
        msg, w = ctx.saved_tensors
        if torch.is_grad_enabled():  # create_graph: the (bilinear) backward is differentiated in ga, msg and w
            gm, gw = _SegmentSumWeightedBackwardFn.apply(ga, msg, w, ctx.g, ctx.needs_input_grad[1])
            return gm, gw, None
        gm, gw = _segment_sum_weighted_backward_raw(ga, msg, w, ctx.g, ctx.needs_input_grad[1])
        return gm, gw, None


def _segment_sum_weighted_backward_raw(ga, msg, w, g, need_w):
    """-> (g_msg[e] = w[e] ga[dst(e)], g_w[e] = <msg[e], ga[dst(e)]> | None): e3_segment_sum_weighted_backward"""
    ga = ga.contiguous()
    N, D = ga.shape
    gm = torch.empty((g.num_edges, D), dtype=torch.float32, device=ga.device)
    gw = torch.empty(g.num_edges, dtype=torch.float32, device=ga.device) if need_w else None
    with torch.cuda.device(ga.device):
        _lib.check(_lib.load().e3_segment_sum_weighted_backward(
            ga.data_ptr(), ga.stride(0), msg.data_ptr(), msg.stride(0), w.data_ptr(), g.rowptr.data_ptr(), N, D,
            gm.data_ptr(), max(gm.stride(0), D), gw.data_ptr() if gw is not None else None, _stream(ga)),
            "e3_segment_sum_weighted_backward")
    return gm, gw


class _SegmentSumWeightedBackwardFn(torch.autograd.Function):
    """(ga, msg, w) -> (g_msg, g_w | None), bilinear.  For the cotangents (c_gm, c_gw):
    cot(ga) = sum_e w_e c_gm_e + sum_e c_gw_e msg_e (two weighted sums), and (cot(msg), cot(w)) = (c_gw_e ga[dst],
    <c_gm_e, ga[dst]>) is ONE e3_segment_sum_weighted_backward call with msg := c_gm and w := c_gw."""

    @staticmethod
    def forward(ctx, ga, msg, w, g, need_w):
        ctx.g, ctx.need_w = g, need_w
        ga = ga.contiguous()
        ctx.save_for_backward(ga, msg, w)
        return _segment_sum_weighted_backward_raw(ga, msg, w, g, need_w)

    @staticmethod
    @once_differentiable
    def backward(ctx, c_gm, c_gw):
        ga, msg, w = ctx.saved_tensors
        g = ctx.g
        c_gm = c_gm.contiguous()
        cot_ga = _segment_sum_weighted_raw(c_gm, w, g)
        if ctx.need_w:
            c_gw = c_gw.contiguous()
            cot_ga = cot_ga + _segment_sum_weighted_raw(msg, c_gw, g)
            cot_msg, cot_w = _segment_sum_weighted_backward_raw(ga, c_gm, c_gw, g, True)
        else:  # no g_w was formed (w does not require grad): g_msg = w ga[dst] does not depend on msg
            cot_msg, cot_w = None, None
        return cot_ga, cot_msg, cot_w, None, None


def segment_sum(msg: torch.Tensor, g: RadiusGraph, weight: torch.Tensor | None = None) -> torch.Tensor:
    """agg[i] = sum of msg rows of CSR row i (fixed order, reproducible); fp32 (differentiable), or bf16 storage with fp32
    accumulation.  ``weight`` [E] fp32 (an edge envelope, ``cutoff_envelope``): agg[i] = sum_e weight_e msg_e, in the same
    fixed order (bit-equal to the unweighted sum at weight = 1), differentiable w.r.t. ``msg`` and ``weight``; fp32 only."""
    if not msg.is_cuda:
        raise RuntimeError("msg: ROCm tensor required (no CPU path)")
    if msg.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"segment_sum: float32 / bfloat16 required, got {msg.dtype}")
    if weight is not None:
        if msg.dtype != torch.float32:
            raise RuntimeError("segment_sum(weight=): the envelope is fp32; bf16 storage has no weighted sum")
        _check(weight, "weight")
        if weight.dim() != 1 or weight.shape[0] != g.num_edges or msg.dim() != 2 or msg.shape[0] != g.num_edges:
            raise ValueError(f"segment_sum(weight=): msg [E, D] and weight [E] with E = {g.num_edges} required, got "
                             f"{tuple(msg.shape)} and {tuple(weight.shape)}")
        if g.num_edges == 0:  # nothing to launch on: every row is empty
            return torch.zeros((g.rowptr.numel() - 1, msg.shape[1]), dtype=torch.float32, device=msg.device)
        if msg.stride(-1) != 1:
            msg = msg.contiguous()
        weight = weight.contiguous()
        if _wants_grad(msg, weight):
            return _SegmentSumWeightedFn.apply(msg, weight, g)
        return _segment_sum_weighted_raw(msg, weight, g)
    if msg.dtype == torch.float32 and _wants_grad(msg):
        return _SegmentSumFn.apply(msg, g)
    return _segment_sum_raw(msg, g)


ENVELOPE_P_RANGE = (2, 16)


def _envelope_args(r_c, p):
    """-> (float r_c, int p); ValueError for p outside [2, 16] or an r_c that is not a finite positive number."""
    import math
    if isinstance(p, bool) or int(p) != p or not ENVELOPE_P_RANGE[0] <= int(p) <= ENVELOPE_P_RANGE[1]:
        raise ValueError(f"envelope exponent p must be an integer in [{ENVELOPE_P_RANGE[0]}, {ENVELOPE_P_RANGE[1]}], got {p!r}")
    r_c = float(r_c)
    if not (math.isfinite(r_c) and r_c > 0.0):
        raise ValueError(f"envelope cutoff must be finite and > 0, got {r_c}")
    return r_c, int(p)


class _CutoffEnvelopeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, d, r_c, p):
        ctx.r_c, ctx.p = r_c, p
        ctx.save_for_backward(d)
        return _cutoff_envelope_raw(d, r_c, p)

    @staticmethod
    def backward(ctx, gw):
        (d,) = ctx.saved_tensors
        if torch.is_grad_enabled():  # create_graph: the backward is differentiated in d and gw
            return _CutoffEnvelopeBackwardFn.apply(d, gw, ctx.r_c, ctx.p), None, None
        return _cutoff_envelope_backward_raw(d, gw, ctx.r_c, ctx.p), None, None


def _cutoff_envelope_backward_raw(d, gw, r_c, p):
    gw = gw.contiguous()
    gd = torch.empty_like(d)
    with torch.cuda.device(d.device):
        _lib.check(_lib.load().e3_cutoff_envelope_backward(d.data_ptr(), gw.data_ptr(), d.numel(), r_c, p,
                                                           gd.data_ptr(), _stream(d)), "e3_cutoff_envelope_backward")
    return gd


class _CutoffEnvelopeBackwardFn(torch.autograd.Function):
    """(d, gw) -> g_d = gw u'(d); its backward is e3_cutoff_envelope_backward2: cot(gw) = c u'(d), cot(d) = c gw u''(d)."""

    @staticmethod
    def forward(ctx, d, gw, r_c, p):
        ctx.r_c, ctx.p = r_c, p
        gw = gw.contiguous()
        ctx.save_for_backward(d, gw)
        return _cutoff_envelope_backward_raw(d, gw, r_c, p)

    @staticmethod
    @once_differentiable
    def backward(ctx, c):
        d, gw = ctx.saved_tensors
        c = c.contiguous()
        need_d, need_gw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        cot_gw = torch.empty_like(d) if need_gw else None
        cot_d = torch.empty_like(d) if need_d else None
        with torch.cuda.device(d.device):
            _lib.check(_lib.load().e3_cutoff_envelope_backward2(
                d.data_ptr(), gw.data_ptr(), c.data_ptr(), d.numel(), ctx.r_c, ctx.p,
                cot_gw.data_ptr() if need_gw else None, cot_d.data_ptr() if need_d else None, _stream(d)),
                "e3_cutoff_envelope_backward2")
        return cot_d, cot_gw, None, None


def _cutoff_envelope_raw(d, r_c, p):
    w = torch.empty_like(d)
    with torch.cuda.device(d.device):
        _lib.check(_lib.load().e3_cutoff_envelope(d.data_ptr(), d.numel(), r_c, p, w.data_ptr(), _stream(d)),
                   "e3_cutoff_envelope")
    return w


def cutoff_envelope(d: torch.Tensor, r_c: float, p: int = 6) -> torch.Tensor:
    """Edge weights w [E] = u_p(d / r_c): the polynomial envelope of include/e3gnn.h (e3_cutoff_envelope), 1 at d = 0 and
    exactly 0 for every d >= r_c, with two vanishing derivatives at r_c.  Differentiable w.r.t. ``d``."""
    r_c, p = _envelope_args(r_c, p)
    _check(d, "d")
    if d.dim() != 1:
        raise ValueError(f"cutoff_envelope: d must be [E], got {tuple(d.shape)}")
    d = d.contiguous()
    if _wants_grad(d):
        return _CutoffEnvelopeFn.apply(d, r_c, p)
    return _cutoff_envelope_raw(d, r_c, p)


def enveloped_node_attr(Y: torch.Tensor, w: torch.Tensor, g: RadiusGraph) -> torch.Tensor:
    """Node attribute of an enveloped model, A [N, (lmax+1)^2] = [1, S_1.. / (1 + S_0)] with S = sum_e w_e Y_e per row
    (Y_e[0] = 1, so S_0 = sum_e w_e): a smooth, bounded stand-in for the mean of Y -- an edge at the cutoff has no share in
    it, an isolated node has [1, 0, ...].  Differentiable w.r.t. ``Y`` and ``w``."""
    S = segment_sum(Y, g, weight=w)
    return torch.cat([torch.ones_like(S[:, :1]), S[:, 1:] / (1.0 + S[:, :1])], 1)


def _gate_blocks_raw(x, ns, blocks):
    import ctypes
    B = x.shape[0]
    wide = sum(m * (2 * l + 1) for l, m in blocks)
    out = torch.empty((B, ns + wide), dtype=torch.float32, device=x.device)
    ls = (ctypes.c_int32 * len(blocks))(*[l for l, _ in blocks])
    ms = (ctypes.c_int32 * len(blocks))(*[m for _, m in blocks])
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().e3_gate_blocks(x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), B, ns,
                                              len(blocks), ls, ms, _stream(x)), "e3_gate_blocks")
    return out


def gate_blocks(x: torch.Tensor, ns: int, blocks) -> torch.Tensor:
    """x = [ns scalars | one gate per gated channel | gated blocks]; blocks = [(l, mul), ...]
    -> [silu(scalars) | sigmoid(gate) * block]  (differentiable)"""
    _check(x, "x")
    if x.stride(-1) != 1:
        x = x.contiguous()
    blocks = tuple((int(l), int(m)) for l, m in blocks)
    ng = sum(m for _, m in blocks)
    wide = sum(m * (2 * l + 1) for l, m in blocks)
    assert x.shape[1] == ns + ng + wide, (x.shape, ns, blocks)
    if _wants_grad(x):
        return _GateBlocksFn.apply(x, ns, blocks)
    return _gate_blocks_raw(x, ns, blocks)


def pow2_scale(tensors, target_log2: int = 10) -> torch.Tensor:
    """Device-resident operand scale ``[s, 1/s, scratch, scratch]`` (fp32) of up to 4 fp32 tensors: ``s`` is the power of
    two that puts their joint max |x| at ``2^target_log2`` (``e3_pow2_scale``; no host sync).  The fp16-split MFMA
    kernels take it as ``in_scale``."""
    import ctypes
    from .tensor_product import TPSegment
    ts = []
    for t in tensors:
        _check(t, "pow2_scale")
        if t.dim() == 1:
            t = t.unsqueeze(1)
        if t.stride(-1) != 1:
            t = t.contiguous()
        ts.append(t)
    assert 1 <= len(ts) <= 4
    dev = ts[0].device
    out = torch.empty(4, dtype=torch.float32, device=dev)
    segs = (TPSegment * len(ts))()
    rows = (ctypes.c_int64 * len(ts))()
    for i, t in enumerate(ts):
        segs[i].base, segs[i].ld, segs[i].ncols = t.data_ptr(), t.stride(0), t.shape[1]
        rows[i] = t.shape[0]
    with torch.cuda.device(dev):
        _lib.check(_lib.load().e3_pow2_scale(ctypes.byref(segs), rows, len(ts), target_log2, out.data_ptr(),
                                             _stream(out)), "e3_pow2_scale")
    return out


def join_pow2_scales(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """The operand scale of the union of two tensor sets from their scales (same target): the smaller ``s``, the larger
    ``1/s`` -- lets a caller that already knows the scale of one operand (``h``: returned by ``add_pow2_scale``) scan
    only the other one.  Device side, no host sync."""
    return torch.stack([torch.minimum(a[0], b[0]), torch.maximum(a[1], b[1]), torch.maximum(a[2], b[2]), a[3]])


def add_pow2_scale(h: torch.Tensor, u: torch.Tensor, target_log2: int = 10):
    """``h + u`` and the operand scale of the sum in one pass (``e3_add_pow2_scale``) -> (sum, scale)."""
    _check(h, "h")
    _check(u, "u")
    assert h.shape == u.shape
    h, u = h.contiguous(), u.contiguous()
    out = torch.empty_like(h)
    sc = torch.empty(4, dtype=torch.float32, device=h.device)
    if h.numel() % 4 or (h.data_ptr() | u.data_ptr() | out.data_ptr()) % 16:
        torch.add(h, u, out=out)
        return out, pow2_scale([out], target_log2)
    with torch.cuda.device(h.device):
        _lib.check(_lib.load().e3_add_pow2_scale(h.data_ptr(), u.data_ptr(), out.data_ptr(), h.numel(), target_log2,
                                                 sc.data_ptr(), _stream(h)), "e3_add_pow2_scale")
    return out, sc


class _ImageRowsExpandFn(torch.autograd.Function):
    """rows -> rows[source] (+ a constant translation): linear in the rows, its backward is the row reduce."""

    @staticmethod
    def forward(ctx, x, rmap, translate):
        from .cell_images import image_rows_expand_raw
        ctx.rmap = rmap
        return image_rows_expand_raw(x, rmap, translate)

    @staticmethod
    def backward(ctx, g):
        return _ImageRowsReduceFn.apply(g, ctx.rmap), None, None


class _ImageRowsReduceFn(torch.autograd.Function):
    """the transpose of the expand: linear, its backward is the expand (without the translation, a constant)."""

    @staticmethod
    def forward(ctx, g, rmap):
        from .cell_images import image_rows_reduce_raw
        ctx.rmap = rmap
        return image_rows_reduce_raw(g, rmap)

    @staticmethod
    def backward(ctx, c):
        return _ImageRowsExpandFn.apply(c, ctx.rmap, False), None


def image_rows_expand(x: torch.Tensor, rmap, translate: bool = False) -> torch.Tensor:
    """x [M, D] -> out[i] = x[rmap.source[i]]: every image row a copy of its owner's row, owned rows unchanged
    (``e3_image_rows_expand``; fp32, bf16 or fp64 on a ROCm device, a torch restatement on the CPU).  ``rmap``: a
    ``cell_images.ImageRowMap``.  ``translate=True`` (x [M,3] fp32 positions) adds the lattice shift ``rmap.shift[i] @ cell``.
    Differentiable to any order: the backward is ``image_rows_reduce`` and that one's backward is this op, both applied as
    Functions."""
    return _ImageRowsExpandFn.apply(x, rmap, translate)


def image_rows_reduce(g: torch.Tensor, rmap) -> torch.Tensor:
    """g [M, D] -> out[i] = g[i] + the rows of the images of owned row i, zero on image rows: the transpose of
    ``image_rows_expand`` (``e3_image_rows_reduce``: fp32 / fp64, summed in ascending row order without atomics, so bit-equal
    from run to run; a torch restatement on the CPU).  Differentiable to any order."""
    return _ImageRowsReduceFn.apply(g, rmap)

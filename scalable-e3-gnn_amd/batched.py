"""Small-graph / many-batch path (BASELINE.json configs[3]: QM9-style batched molecules, energy head).

No reference code exists for this stage in the mount (SURVEY.md §8 row a-N5): the contract here is builder-defined.
A batch of molecules is ONE radius graph: the molecules are laid out on a 3-D lattice whose spacing exceeds the largest
molecule by two cutoff radii, so the cell-list builder (`e3_rg_*`) finds exactly the intra-molecular pairs in one pass,
with the same kernels as the single-cloud path.  The neighbour search runs on the lattice copy; the graph that is
returned carries the ORIGINAL coordinates, so edge vectors / spherical harmonics see no shift rounding.  The energy
head is the per-molecule sum of a scalar (`1x0e`) node readout.  The force head is -dE/dpos by reverse-mode autograd
through the whole message pass: every stage has a HIP backward (tensor products: `e3_l1tp_backward` / `e3_tp_backward`;
edge geometry, gather/concat, gates, segment-sum: `e3_*_backward`, csrc/e3_edge_geometry_bwd.hip and csrc/e3_edge_bwd.hip).  With ``create_graph=True`` the
forces keep their graph: every stage's backward has a backward of its own (the multilinear stages by composition of the
same entries; `e3_edge_geometry_jvp`, `e3_gate_blocks_backward2`, `e3_cutoff_envelope_backward2`), so a loss on energies
AND forces has parameter gradients.  The derivative of the forces w.r.t. the positions needs one kernel
more, the Hessian of Y, d, A in the edge vector (`e3_edge_geometry_hvp`): a parameter gradient never needs it and the
force-loss step does not launch it; `hessian_vector_product` / `hessian` of the two models below do.  The strained forms of
both kernels (`e3_edge_geometry_jvp_strained` / `_hvp_strained`) give the second derivative in the joint coordinates
(pos, strain): `PeriodicEnergyModel.strain_hessian_vector_product` / `elastic_tensor` (Born term and force-strain coupling).
Virials and stress are the derivative w.r.t. a zero strain per structure, reduced inside the same geometry backward
(`e3_edge_geometry_backward_strained`); `PeriodicEnergyModel` is the periodic-box counterpart of `BatchedEnergyModel`, and
`BatchedPeriodicEnergyModel` their combination: a batch of periodic structures, each with its own cell, over image rows.
"""
from __future__ import annotations

import dataclasses
import math

import torch
from torch import nn

from .radius_graph import RadiusGraph, check_max_neighbors, radius_graph
from .segnn import SEGNN


def batched_radius_graph(pos: torch.Tensor, batch: torch.Tensor, r: float, max_neighbors=None):
    """pos [N,3] fp32 on a ROCm device, batch [N] integer molecule id of every atom (any order, ids 0..n_mol-1).
    -> (RadiusGraph over all atoms with intra-molecular edges only, mol_of_node [N] int64 in the graph's node order)

    ``max_neighbors`` (None or an int in [1, 64]): the cap of ``radius_graph(max_neighbors=)`` -- every atom keeps its k
    nearest neighbours inside ``r``; the distances are those of the lattice copy the search runs on, and the graph is
    then directed."""
    check_max_neighbors(max_neighbors)
    if not pos.is_cuda:
        raise RuntimeError("batched_radius_graph runs on ROCm tensors only; there is no CPU path")
    batch = batch.long()
    N = pos.shape[0]
    n_mol = int(batch.max().item()) + 1 if N else 0
    if N == 0:
        g = radius_graph(pos, r, [0.0] * 3, [1.0] * 3, max_neighbors=max_neighbors)
        return g, batch
    idx = batch[:, None].expand(-1, 3)
    pmin = torch.full((n_mol, 3), float("inf"), device=pos.device).scatter_reduce(0, idx, pos, "amin")
    pmax = torch.full((n_mol, 3), float("-inf"), device=pos.device).scatter_reduce(0, idx, pos, "amax")
    extent = float((pmax - pmin).max().item())
    cell = extent + 2.0 * float(r)
    side = max(1, math.ceil(n_mol ** (1.0 / 3.0) - 1e-9))
    lattice = torch.stack([batch % side, (batch // side) % side, batch // (side * side)], 1).to(pos.dtype)
    shifted = (pos - pmin[batch]) + lattice * cell + float(r)
    nz = (n_mol + side * side - 1) // (side * side)
    hi = [side * cell + float(r), side * cell + float(r), nz * cell + float(r)]
    if max(hi) / float(r) > 1000:
        raise RuntimeError("batch too large for one lattice pass (cell grid > 1000 cells per axis): split the batch")
    g = radius_graph(shifted.contiguous(), r, [0.0, 0.0, 0.0], hi, max_neighbors=max_neighbors)
    perm = g.perm.long()
    pos4 = torch.zeros((N, 4), dtype=torch.float32, device=pos.device)
    pos4[:, :3] = pos[perm]
    return dataclasses.replace(g, pos4=pos4), batch[perm]


def _skin_radius(net, r: float, skin: float) -> float:
    """The graph radius r + skin of a forward.  A skin needs the envelope (ValueError without one): only an enveloped model
    gives an edge beyond r no share in the energy."""
    if skin != 0.0 and net.envelope is None:
        raise ValueError("skin= needs a model built with envelope=: without the envelope the edges between r and r + skin "
                         "would change the energy")
    if not skin >= 0.0:
        raise ValueError(f"skin must be >= 0, got {skin}")
    return r if skin == 0.0 else float(r) + float(skin)


def _cutoff_kw(net, r: float) -> dict:
    """cutoff= of the net's forward: the envelope's radius r of an enveloped model, nothing otherwise."""
    return {} if net.envelope is None else {"cutoff": float(r)}


def _neighbors_graph(neighbors, pos, r, skin, defaults: dict):
    """The graph of a forward with ``neighbors=`` (a ``neighbor_list.NeighborList``): ``neighbors.update(pos)``.  The list
    owns the radius, the skin and the box, so ``r`` must be the list's and every argument of ``defaults`` (name -> (value,
    default)) must be left alone -- ``ValueError`` naming the argument otherwise."""
    if float(r) != neighbors.r:
        raise ValueError(f"r = {r} is not the radius of neighbors= ({neighbors.r})")
    if skin != 0.0:
        raise ValueError("skin= must stay 0 with neighbors=: the list has a skin of its own and returns the graph at r")
    for name, (value, default) in defaults.items():
        if value is not default:
            raise ValueError(f"{name}= must be left at its default with neighbors=: the list holds the box it was made with")
    return neighbors.update(pos)


_NO_SECOND_ORDER_STRAIN = ("create_graph=True with virial= / stress=: the tangent kernel of the strained edge geometry exists at "
                           "ops.edge_geometry(strain=), but the stress loss is not wired at model level, so the virial and the "
                           "stress cannot be trained on here")


def _check_create_graph(net, x, forces: bool, strained: bool):
    """The preconditions of ``create_graph=True`` (second derivatives: a loss on the forces)."""
    if strained:
        raise NotImplementedError(_NO_SECOND_ORDER_STRAIN)
    if x.dtype == torch.bfloat16:
        raise NotImplementedError("create_graph=True with bf16 storage: bf16 runs the fused inference kernels only and has no "
                                  "differentiable chain")
    if not forces:
        raise ValueError("create_graph=True keeps the graph of the forces: it needs forces=True")
    if not any(p.requires_grad for p in net.parameters()):
        raise ValueError("create_graph=True needs at least one parameter that requires grad: the graph of the forces leads "
                         "to the parameters only (the derivative of the forces w.r.t. the positions is "
                         "hessian_vector_product)")


def _energy_and_gradients(net, x_g, g, pos_g, seg, n_seg, forces, n_strain, structure, cutoff_kw=None, halo=None,
                          split=None, create_graph=False):
    """Energy of ``net``'s scalar node readout summed per segment (``seg`` [N] graph order, ``n_seg`` segments; ``seg``
    None: the 0-d total), and from ONE backward pass through the differentiable chain dE/dpos_g [N,3] (``forces``) and
    dE/deps [n_strain,3,3] at a zero per-structure strain (``n_strain`` > 0; ``structure`` [N] graph order, None = one
    structure).  -> (energy, dE/dpos_g | None, dE/deps | None); the energy keeps its graph in training mode.
    ``create_graph``: the backward pass is itself recorded, so dE/dpos_g carries a graph that leads to the parameters (a
    loss on the forces can be differentiated once more), and the energy keeps its graph in eval mode too.

    ``halo`` / ``split`` (sharded path; ``g`` = ``split.graph``): the readout is summed over THIS rank's owned rows, the
    ghost rows are refreshed by ``halo.refresh`` in every layer, and ``halo.anchor`` is among the differentiated inputs, so
    the backward of every refresh runs on every rank; dE/dpos_g then covers the local cloud, ghost rows included.  A
    ``cell_images.CellImages`` serves as ``halo`` in one process (image rows of a small cell; its ``anchor`` is None)."""
    from . import ops
    with torch.enable_grad():
        p = pos_g.detach().float().requires_grad_(forces)
        eps = torch.zeros((n_strain, 3, 3), dtype=torch.float32, device=p.device, requires_grad=True) if n_strain else None
        # differentiable Y, d, A.  pos_hessian=False: under create_graph the graph of the forces is wanted for the parameters
        # only, so the geometry backward gets no position edge (no Hessian launch, no unused .grad on the leaf p)
        geometry = ops.edge_geometry(g, lmax=net.lmax, pos=p, strain=eps, structure=structure, pos_hessian=False)
        e_node = net(x_g, g, geometry=geometry, halo=halo, split=split, **(cutoff_kw or {}))
        if halo is not None:
            e_node = e_node[halo.owned_new]
        if seg is None:
            energy = e_node[:, 0].sum()
        else:
            energy = torch.zeros(n_seg, dtype=e_node.dtype, device=e_node.device).index_add(0, seg, e_node[:, 0])
        # halo.anchor: the leaf that keeps every rank's refresh in the backward (None for the image rows of one process)
        anchor = None if halo is None else halo.anchor
        leaves = ([p] if forces else []) + ([eps] if eps is not None else []) + ([] if anchor is None else [anchor])
        if create_graph:
            grads = list(torch.autograd.grad(energy.sum(), leaves, create_graph=True))
        else:
            grads = list(torch.autograd.grad(energy.sum(), leaves, retain_graph=net.training))
    gpos = grads.pop(0) if forces else None
    geps = grads.pop(0) if eps is not None else None
    return (energy if (net.training or create_graph) else energy.detach()), gpos, geps


HESSIAN_MAX_ATOMS = 256   # hessian(): 3 N second backwards and a dense [N,3,N,3] result -- molecules and small cells


def _hessian_vector_products(net, x_g, g, pos_g, v_g, cutoff_kw, xi=None, strained=False, halo=None, split=None):
    """H v for every v of ``v_g`` [K,N,3] (graph order) -> [K,N,3], H = d2(sum of the scalar node readout)/dpos_g^2 on the
    edge set of ``g``.  One forward, one first backward with ``create_graph=True`` -- the geometry with its position edge
    (``ops.edge_geometry(pos_hessian=True)``) -- and one second backward per vector on the retained graph.  Only the
    position leaf is differentiated: the parameters may be frozen and none of them gets a ``.grad``.

    ``strained`` (or an ``xi`` [K,3,3]): the same in the joint coordinates (pos_g, eps) at a zero strain eps of the whole graph
    -> (h_pos [K,N,3], h_strain [K,3,3]) = the Hessian applied to (v, xi), either of which may be None (zero), not both.

    ``halo`` / ``split`` (a ``cell_images.CellImages`` and its split graph, ``g`` = ``split.graph``): N counts the rows of the
    extended cloud, the readout is summed over the owned rows and every layer refreshes the image rows differentiably; the
    caller extends ``v`` to the image rows and reduces the product (H = E^T H_ext E)."""
    from . import ops
    if x_g.dtype == torch.bfloat16:
        raise NotImplementedError("hessian_vector_product with bf16 storage: bf16 runs the fused inference kernels only and "
                                  "has no differentiable chain")
    strained = strained or xi is not None
    v_g = v_g.to(torch.float32) if v_g is not None else None
    xi = xi.to(torch.float32) if xi is not None else None
    K = len(v_g) if v_g is not None else len(xi)
    # the parameters are constants of H v: frozen for the length of the call, so that no backward forms a weight gradient
    # or a weight cotangent that nobody reads (the Functions decide from requires_grad at forward time)
    trainable = [q for q in net.parameters() if q.requires_grad]
    for q in trainable:
        q.requires_grad_(False)
    try:
        with torch.enable_grad():
            p = pos_g.detach().float().requires_grad_(True)
            eps = torch.zeros((1, 3, 3), dtype=torch.float32, device=p.device, requires_grad=True) if strained else None
            leaves = [p] + ([eps] if strained else [])
            geometry = ops.edge_geometry(g, lmax=net.lmax, pos=p, strain=eps)
            e_node = net(x_g, g, geometry=geometry, halo=halo, split=split, **(cutoff_kw or {}))
            if halo is not None:
                e_node = e_node[halo.owned_new]
            first = torch.autograd.grad(e_node[:, 0].sum(), leaves, create_graph=True)
        out = []
        for k in range(K):
            pairs = [(f, c[k]) for f, c in zip(first, (v_g, xi[:, None] if xi is not None else None)) if c is not None]
            out.append(torch.autograd.grad([f for f, _ in pairs], leaves, [c for _, c in pairs], retain_graph=k + 1 < K))
    finally:
        for q in trainable:
            q.requires_grad_(True)
    if not strained:
        return torch.stack([o[0] for o in out]) if out else torch.zeros_like(v_g)
    if not out:
        return torch.zeros((0, *pos_g.shape), device=p.device), torch.zeros((0, 3, 3), device=p.device)
    return torch.stack([o[0] for o in out]), torch.stack([o[1][0] for o in out])


def _check_vectors(v, pos):
    """v [N,3] or [K,N,3] for pos [N,3] -> v as [K,N,3]; ValueError otherwise"""
    if v is None:
        raise ValueError("hessian_vector_product needs v= ([N,3] or [K,N,3])")
    if tuple(v.shape[-2:]) != tuple(pos.shape) or v.dim() not in (2, 3):
        raise ValueError(f"v must be [N,3] or [K,N,3] with N = {pos.shape[0]}, got {tuple(v.shape)}")
    return v.reshape(-1, *pos.shape)


def _check_strain_vectors(v, strain_v, pos):
    """v [N,3] | [K,N,3] | None and strain_v [3,3] | [K,3,3] | None -> (v [K,N,3] | None, strain_v [K,3,3] | None, whether the
    caller's tensors carry no K); ValueError when both are None, a shape is wrong or the K's differ"""
    if v is None and strain_v is None:
        raise ValueError("strain_hessian_vector_product needs v= ([N,3] or [K,N,3]) or strain_v= ([3,3] or [K,3,3])")
    if strain_v is not None and (tuple(strain_v.shape[-2:]) != (3, 3) or strain_v.dim() not in (2, 3)):
        raise ValueError(f"strain_v must be [3,3] or [K,3,3], got {tuple(strain_v.shape)}")
    vs = _check_vectors(v, pos) if v is not None else None
    xs = strain_v.reshape(-1, 3, 3) if strain_v is not None else None
    if vs is not None and xs is not None and (len(vs) != len(xs) or (v.dim() == 2) != (strain_v.dim() == 2)):
        raise ValueError(f"v {tuple(v.shape)} and strain_v {tuple(strain_v.shape)} must hold the same number K of vectors")
    single = (v if v is not None else strain_v).dim() == 2
    return vs, xs, single


VOIGT = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))


def voigt(born: torch.Tensor) -> torch.Tensor:
    """born [3,3,3,3] -> [6,6]: ``C[I,J] = sum_abcd born[a,b,c,d] S_I[a,b] S_J[c,d]`` with the symmetric strain basis
    ``S_I = (e_a e_b^T + e_b e_a^T) / 2`` of the Voigt pair I = (a, b) in the order xx, yy, zz, yz, xz, xy -- the second
    derivative in the Voigt strains with engineering shears (eps_ab = eps_ba = gamma / 2), i.e. the average of the four
    index permutations of a shear entry."""
    if tuple(born.shape) != (3, 3, 3, 3):
        raise ValueError(f"born must be [3,3,3,3], got {tuple(born.shape)}")
    basis = torch.zeros((6, 3, 3), dtype=born.dtype, device=born.device)
    for i, (a, b) in enumerate(VOIGT):
        basis[i, a, b] += 0.5
        basis[i, b, a] += 0.5
    return torch.einsum("iab,abcd,jcd->ij", basis, born, basis)


def _dense_hessian(hvp, pos, chunk: int = 96):
    """[N,3,N,3] from ``hvp(v [K,N,3]) -> [K,N,3]`` on the 3 N unit vectors, ``chunk`` at a time"""
    N = pos.shape[0]
    if N > HESSIAN_MAX_ATOMS:
        raise ValueError(f"hessian() is meant for molecules and small cells: N = {N} > {HESSIAN_MAX_ATOMS} atoms "
                         "(HESSIAN_MAX_ATOMS); use hessian_vector_product")
    eye = torch.eye(3 * N, dtype=torch.float32, device=pos.device).view(3 * N, N, 3)
    cols = [hvp(eye[k:k + chunk]) for k in range(0, 3 * N, chunk)]
    H = torch.cat(cols) if cols else eye
    return H.view(N, 3, N, 3).permute(2, 3, 0, 1).contiguous()   # H[i, a, j, b] = (H e_jb)[i, a]


class BatchedEnergyModel(nn.Module):
    """SEGNN with a scalar node readout summed per molecule: energies [n_mol].  ``envelope`` (the exponent p, e.g. 6;
    ``SEGNN(envelope=)``): every pair is weighted by a smooth cutoff envelope of radius ``r``, so the energy is a smooth
    function of the positions and forces / virials are its derivatives also where a pair crosses the cutoff."""

    def __init__(self, in_irreps="1x0e+1x1o", hidden: int = 32, num_layers: int = 4, lmax: int = 2,
                 envelope: int | None = None):
        super().__init__()
        self.net = SEGNN(in_irreps, hidden, "1x0e", num_layers, lmax=lmax, envelope=envelope)

    def _graph(self, pos, batch, r, skin, neighbors):
        """The graph of a forward -> (RadiusGraph, molecule of every node in graph order)"""
        if neighbors is not None:
            if neighbors.batch is None:
                raise ValueError("neighbors= of a batched model must be a NeighborList made with batch=")
            g = _neighbors_graph(neighbors, pos, r, skin, {})
            if neighbors.rebuilt and not (neighbors.batch.shape == batch.shape and
                                          torch.equal(neighbors.batch.to(batch.device).long(), batch.long())):
                raise ValueError("batch= is not the tensor neighbors= was made with")
            return g, neighbors.mol_of_node
        return batched_radius_graph(pos, batch, _skin_radius(self.net, r, skin))

    def forward(self, x: torch.Tensor, pos: torch.Tensor, batch: torch.Tensor, r: float, forces: bool = False,
                virial: bool = False, skin: float = 0.0, neighbors=None, create_graph: bool = False):
        """-> energies [n_mol]; with ``forces=True``: (energies, forces [N,3] = -dE/dpos in the caller's atom order);
        with ``virial=True`` the per-molecule virials W [n_mol,3,3] = -dE/deps (zero strain per molecule, not
        symmetrised) come last: (energies, forces, W) or (energies, W).

        ``skin`` (enveloped models only): the graph is built at ``r + skin`` while the envelope's radius stays ``r``; the
        outputs are those of ``skin = 0`` up to rounding.

        ``neighbors`` (a ``NeighborList(r, skin, batch=batch)``): the graph is ``neighbors.update(pos)`` -- built at the
        list's ``r + skin`` once, pruned to ``r`` on the device while no atom has moved half the skin -- for any model,
        enveloped or not; ``skin`` stays 0 and ``batch`` must be the tensor the list was made with (compared when the
        list rebuilds).

        ``create_graph=True`` (needs ``forces=True`` and a parameter that requires grad; fp32): energies and forces both
        carry a graph, in ``train()`` and ``eval()`` mode, so ``loss(energies, forces).backward()`` fills ``p.grad`` of
        every parameter -- training on forces.  The graph leads to the parameters only: the derivative of the forces
        w.r.t. the positions is ``hessian_vector_product``.  ``NotImplementedError`` with ``virial=True`` (the tangent kernel of the
        strained geometry exists, ``ops.edge_geometry(strain=)``, but a loss on the virial is not wired at model level) and for
        bf16 storage.  False (the default) is the first-order call, unchanged."""
        if create_graph:
            _check_create_graph(self.net, x, forces, virial)
        g, mol = self._graph(pos, batch, r, skin, neighbors)
        cut = _cutoff_kw(self.net, r)
        n_mol = int(batch.max().item()) + 1 if batch.numel() else 0
        perm = g.perm.long()
        if not forces and not virial:
            e_node = self.net(x[perm], g, **cut)
            return torch.zeros(n_mol, dtype=e_node.dtype, device=e_node.device).index_add_(0, mol, e_node[:, 0])
        energy, gpos, geps = _energy_and_gradients(self.net, x[perm], g, pos[perm], mol, n_mol, forces,
                                                   n_mol if virial else 0, mol if virial else None, cut,
                                                   create_graph=create_graph)
        out = [energy]
        if forces:
            f = torch.empty_like(gpos)
            f[perm] = -gpos
            out.append(f)
        if virial:
            out.append(-geps)
        return tuple(out)

    def hessian_vector_product(self, x: torch.Tensor, pos: torch.Tensor, batch: torch.Tensor, r: float, v: torch.Tensor,
                               skin: float = 0.0, neighbors=None) -> torch.Tensor:
        """H v, H = d2(sum of the energies)/dpos2 on the edge set of the current graph (block diagonal over the molecules);
        ``v`` [N,3] or [K,N,3] in the caller's atom order -> a detached tensor of the shape of ``v``.  ``r`` / ``skin`` /
        ``neighbors`` select the graph exactly as in ``forward``.  One forward and one first backward with
        ``create_graph=True``, then one second backward per vector (``e3_edge_geometry_hvp`` closes the chain, DESIGN.md
        §4.6).  Works on a frozen model in ``eval()``; no parameter gets a ``.grad``.  fp32: bf16 storage raises
        ``NotImplementedError``."""
        vs = _check_vectors(v, pos)
        g, _ = self._graph(pos, batch, r, skin, neighbors)
        perm = g.perm.long()
        hv = _hessian_vector_products(self.net, x[perm], g, pos[perm], vs[:, perm], _cutoff_kw(self.net, r))
        out = torch.empty_like(hv)
        out[:, perm] = hv
        return out.reshape(v.shape)

    def hessian(self, x: torch.Tensor, pos: torch.Tensor, batch: torch.Tensor, r: float, skin: float = 0.0,
                neighbors=None) -> torch.Tensor:
        """The dense H [N,3,N,3] (``H[i,a,j,b]`` = d2E/dpos[i,a] dpos[j,b]): ``hessian_vector_product`` on the 3 N unit vectors
        in chunks.  ``ValueError`` above ``HESSIAN_MAX_ATOMS`` = 256 atoms: it is meant for molecules and small cells."""
        return _dense_hessian(lambda vs: self.hessian_vector_product(x, pos, batch, r, vs, skin=skin, neighbors=neighbors), pos)


def _graph_volume(g) -> float:
    """V of a fully periodic graph: |det cell|, or L_x L_y L_z of a box"""
    return float(g.volume) if g.cell is not None else float(g.box[0]) * float(g.box[1]) * float(g.box[2])


_IMAGES_NEED_CELL = ("images= extends a general cell by its lattice images: it needs cell= (the lo / hi / periodic box form is not "
                     "covered; pass the box as a diagonal cell)")
_IMAGES_NO_LIST = ("images= with neighbors=: a Verlet list over image rows is not implemented (the list would have to follow the "
                   "image selection); call without neighbors=")


def _image_vectors(images, v):
    """v [K,N,3] on the owned particles (caller order) -> [K,M,3] on the extended cloud, image rows copies of their owners'
    (no translation: a direction has no lattice shift)"""
    K, N = v.shape[0], v.shape[1]
    M = images.n_owned + images.n_ghost
    if K == 0:
        return v.new_zeros((0, M, 3))
    return images.extend(v.permute(1, 0, 2).reshape(N, 3 * K)).view(M, K, 3).permute(1, 0, 2).contiguous()


def _reduce_vectors(images, h):
    """the transpose of ``_image_vectors``: h [K,M,3] -> [K,N,3] in the caller's order"""
    K, M = h.shape[0], h.shape[1]
    if K == 0:
        return h.new_zeros((0, images.n_owned, 3))
    return images.reduce(h.permute(1, 0, 2).reshape(M, 3 * K)).view(images.n_owned, K, 3).permute(1, 0, 2).contiguous()


class PeriodicEnergyModel(nn.Module):
    """SEGNN with a scalar node readout summed over a periodic (or partly periodic) orthorhombic box, or over a general
    (triclinic) cell: the energy, and on request forces, the virial and the stress of the box (conventions:
    include/e3gnn.h, e3_edge_geometry_strained).  The graph is built inside ``forward`` (``radius_graph(..., periodic=)``
    or ``radius_graph(..., cell=)``).  ``envelope`` (the exponent p, e.g. 6; ``SEGNN(envelope=)``): every pair is weighted
    by a smooth cutoff envelope of radius ``r``; the energy is then a smooth function of the positions and of the strain, and
    forces and stress are its derivatives also where a pair crosses the cutoff (what a relaxation or an MD run needs)."""

    def __init__(self, in_irreps="1x0e+1x1o", hidden: int = 32, num_layers: int = 4, lmax: int = 2,
                 envelope: int | None = None):
        super().__init__()
        self.net = SEGNN(in_irreps, hidden, "1x0e", num_layers, lmax=lmax, envelope=envelope)

    def forward(self, x: torch.Tensor, pos: torch.Tensor, r: float, lo=None, hi=None, periodic=True, forces: bool = False,
                virial: bool = False, stress: bool = False, cell=None, origin=None, skin: float = 0.0, neighbors=None,
                create_graph: bool = False, images=False):
        """x [N, in_dim], pos [N,3] (caller order; coordinates on periodic axes may be unwrapped).  -> the 0-d energy,
        then whichever of forces [N,3] (= -dE/dpos, caller order), virial W [3,3] (= -dE/deps at eps = 0, not
        symmetrised) and stress [3,3] (= (1/V) dE/deps = -W/V, V = L_x L_y L_z) were requested, in that order; the
        energy alone when none was.  ``stress=True`` needs all three axes periodic (ValueError otherwise).

        ``cell`` (3x3, rows = lattice vectors) with ``origin``: a general cell instead of ``lo`` / ``hi`` / ``periodic``
        (``radius_graph(cell=)``; always periodic on all three directions); the stress uses V = |det cell|.

        ``skin`` (enveloped models only): the graph is built at ``r + skin`` -- the periodic and cell cutoff checks apply
        to that radius -- while the envelope's radius stays ``r``; the outputs are those of ``skin = 0`` up to rounding.

        ``neighbors`` (a ``NeighborList`` holding the box or cell): the graph is ``neighbors.update(pos)`` -- built at the
        list's ``r + skin`` once, pruned to ``r`` on the device while no particle has moved half the skin -- for any
        model, enveloped or not; ``lo`` / ``hi`` / ``periodic`` / ``cell`` / ``origin`` / ``skin`` then stay at their
        defaults (ValueError otherwise) and ``stress=True`` needs a list periodic on all three axes.

        ``create_graph=True`` (needs ``forces=True`` and a parameter that requires grad; fp32): the energy and the forces
        both carry a graph, in ``train()`` and ``eval()`` mode, so ``loss(energy, forces).backward()`` fills ``p.grad`` of
        every parameter -- training on forces -- for an open box, a box and ``cell=``, with or without ``envelope=``,
        ``skin=`` and ``neighbors=``.  The graph leads to the parameters only: the derivative of the forces w.r.t. the
        positions is ``hessian_vector_product``.  ``NotImplementedError`` with ``virial=True`` / ``stress=True`` (the tangent kernel of
        the strained geometry exists, ``ops.edge_geometry(strain=)``, but a loss on the stress is not wired at model level) and
        for bf16 storage.  False (the default) is the first-order call, unchanged.

        ``images`` (with ``cell=``): False (the default) is the call above -- a cell with ``2 r >=`` a perpendicular height
        is a ``ValueError``.  True extends the cloud by the lattice images within ``r`` of the cell
        (``cell_images.CellImages``) and runs the OPEN graph over [particles | images], so a cell of any size works -- a
        primitive cell, a one-atom cell -- up to 7 image shells per axis (``ValueError`` beyond); forces come out on the N
        particles, an image's share added to its owner's in a fixed order; energy only under ``no_grad`` runs the fused
        inference kernels.  "auto" takes that path only when the cell needs it (``2 (r + skin) >=`` a height) and is the
        default call otherwise.  Everything above holds on the image path (``forces``, ``virial``, ``stress``, ``skin``,
        ``create_graph``) except ``neighbors=`` (``NotImplementedError``); without ``cell=`` it is a ``ValueError``."""
        if create_graph:
            _check_create_graph(self.net, x, forces, virial or stress)
        if self._use_images(images, r, lo, hi, periodic, cell, origin, skin, neighbors):
            return self._forward_images(x, pos, r, cell, origin, skin, forces, virial, stress, create_graph)
        g, cut = self._graph(pos, r, lo, hi, periodic, cell, origin, skin, neighbors, stress)
        perm = g.perm.long()
        if not (forces or virial or stress):
            return self.net(x[perm], g, **cut)[:, 0].sum()
        energy, gpos, geps = _energy_and_gradients(self.net, x[perm], g, pos[perm], None, 1, forces,
                                                   1 if (virial or stress) else 0, None, cut, create_graph=create_graph)
        out = [energy]
        if forces:
            f = torch.empty_like(gpos)
            f[perm] = -gpos
            out.append(f)
        if virial:
            out.append(-geps[0])
        if stress:
            out.append((geps[0].double() / _graph_volume(g)).float())
        return tuple(out)

    def _use_images(self, images, r, lo, hi, periodic, cell, origin, skin, neighbors) -> bool:
        """Whether a call takes the image path; the refusals of ``images=`` (before anything is built)"""
        if images is False:
            return False
        if images is not True and images != "auto":
            raise ValueError(f'images must be False, True or "auto", got {images!r}')
        if cell is None or lo is not None or hi is not None or periodic is not True:
            raise ValueError(_IMAGES_NEED_CELL)
        if neighbors is not None:
            raise NotImplementedError(_IMAGES_NO_LIST)
        if images is True:
            return True
        from .cell_images import CellImages
        return CellImages(cell, origin).needs_images(_skin_radius(self.net, r, skin))

    def _image_cloud(self, x, pos, r, cell, origin, skin):
        """-> (CellImages, SplitGraph, x and pos of the extended cloud in graph order, the cutoff= of the net's forward)"""
        from .cell_images import cell_image_graph
        cut = _cutoff_kw(self.net, r)
        return (*cell_image_graph(pos, x, _skin_radius(self.net, r, skin), cell, origin), cut)

    def _forward_images(self, x, pos, r, cell, origin, skin, forces, virial, stress, create_graph):
        """``forward`` over the image rows: the open graph of the extended cloud, the readout summed over the particles,
        dE/dpos of the extended cloud reduced to the particles (differentiable: ``create_graph`` keeps it in the graph)"""
        im, split, x_g, pos_g, cut = self._image_cloud(x, pos, r, cell, origin, skin)
        if not (forces or virial or stress):
            return self.net(x_g, split.graph, halo=im, split=split, **cut)[im.owned_new, 0].sum()
        energy, gpos, geps = _energy_and_gradients(self.net, x_g, split.graph, pos_g, None, 1, forces,
                                                   1 if (virial or stress) else 0, None, cut, halo=im, split=split,
                                                   create_graph=create_graph)
        out = [energy]
        if forces:
            out.append(-im.reduce(gpos))
        if virial:
            out.append(-geps[0])
        if stress:
            out.append((geps[0].double() / float(im.volume)).float())
        return tuple(out)

    def _graph(self, pos, r, lo, hi, periodic, cell, origin, skin, neighbors, stress=False):
        """The graph of a forward -> (RadiusGraph, the cutoff= of the net's forward)"""
        from .radius_graph import periodic_mask
        r_env, r = r, _skin_radius(self.net, r, skin)
        cut = _cutoff_kw(self.net, r_env)
        if neighbors is not None:
            if stress and not neighbors.fully_periodic:  # from the list's box: refused before the list is touched
                raise ValueError("stress is defined for a box periodic on all three axes; use virial=True for an open axis")
            g = _neighbors_graph(neighbors, pos, r, skin, {"lo": (lo, None), "hi": (hi, None), "periodic": (periodic, True),
                                                          "cell": (cell, None), "origin": (origin, None)})
        elif cell is not None:
            if lo is not None or hi is not None or periodic is not True:
                raise ValueError("cell= describes the whole periodic cell: it cannot be combined with lo / hi / periodic")
            g = radius_graph(pos, r, cell=cell, origin=origin)
        else:
            if stress and periodic_mask(periodic, r, lo, hi) != 7:
                raise ValueError("stress is defined for a box periodic on all three axes; use virial=True for an open axis")
            g = radius_graph(pos, r, lo, hi, periodic=periodic)
        return g, cut

    def hessian_vector_product(self, x: torch.Tensor, pos: torch.Tensor, r: float, lo=None, hi=None, periodic=True, cell=None,
                               origin=None, v: torch.Tensor | None = None, skin: float = 0.0, neighbors=None,
                               images=False) -> torch.Tensor:
        """H v, H = d2E/dpos2 on the edge set of the current graph (the lattice shift of every edge held fixed); ``v`` [N,3]
        or [K,N,3] in the caller's order -> a detached tensor of the shape of ``v``.  ``lo`` / ``hi`` / ``periodic`` /
        ``cell`` / ``origin`` / ``skin`` / ``neighbors`` select the graph exactly as in ``forward``: open box, box, cell,
        envelope, skin, Verlet list.  One forward and one first backward with ``create_graph=True``, then one second backward
        per vector (``e3_edge_geometry_hvp`` closes the chain) -- what vibrational frequencies, phonons at
        Gamma, dimer / Lanczos saddle searches and Newton-type relaxations consume.  Works on a frozen model in ``eval()``;
        no parameter gets a ``.grad``.  fp32: bf16 storage raises ``NotImplementedError``.  ``images``: as in ``forward``;
        on the image path ``v`` is copied to the image rows (a direction has no lattice shift) and the product is reduced
        back to the N particles, H = E^T H_ext E."""
        vs = _check_vectors(v, pos)
        if self._use_images(images, r, lo, hi, periodic, cell, origin, skin, neighbors):
            im, split, x_g, pos_g, cut = self._image_cloud(x, pos, r, cell, origin, skin)
            hv = _hessian_vector_products(self.net, x_g, split.graph, pos_g, _image_vectors(im, vs.float()), cut, halo=im,
                                          split=split)
            return _reduce_vectors(im, hv).reshape(v.shape)
        g, cut = self._graph(pos, r, lo, hi, periodic, cell, origin, skin, neighbors)
        perm = g.perm.long()
        hv = _hessian_vector_products(self.net, x[perm], g, pos[perm], vs[:, perm], cut)
        out = torch.empty_like(hv)
        out[:, perm] = hv
        return out.reshape(v.shape)

    def _strain_hvp(self, x, pos, r, lo, hi, periodic, cell, origin, v, strain_v, skin, neighbors, stress, images=False):
        """-> (h_pos [K,N,3] caller order, h_strain [K,3,3], whether the caller's vectors carry no K, the volume | None);
        ``stress``: refuse an open axis as ``forward(stress=True)`` does (the volume is returned then)"""
        vs, xs, single = _check_strain_vectors(v, strain_v, pos)
        if self._use_images(images, r, lo, hi, periodic, cell, origin, skin, neighbors):
            im, split, x_g, pos_g, cut = self._image_cloud(x, pos, r, cell, origin, skin)
            hp, hs = _hessian_vector_products(self.net, x_g, split.graph, pos_g,
                                              _image_vectors(im, vs.float()) if vs is not None else None, cut, xi=xs,
                                              strained=True, halo=im, split=split)
            return _reduce_vectors(im, hp), hs, single, float(im.volume)
        g, cut = self._graph(pos, r, lo, hi, periodic, cell, origin, skin, neighbors, stress)
        perm = g.perm.long()
        hp, hs = _hessian_vector_products(self.net, x[perm], g, pos[perm], vs[:, perm] if vs is not None else None, cut,
                                          xi=xs, strained=True)
        out = torch.empty_like(hp)
        out[:, perm] = hp
        return out, hs, single, (_graph_volume(g) if stress else None)

    def strain_hessian_vector_product(self, x: torch.Tensor, pos: torch.Tensor, r: float, lo=None, hi=None, periodic=True,
                                      cell=None, origin=None, v: torch.Tensor | None = None,
                                      strain_v: torch.Tensor | None = None, skin: float = 0.0, neighbors=None,
                                      images=False):
        """The Hessian of E in the joint coordinates (pos, eps) at eps = 0 -- eps the 3x3 strain of ``forward``'s virial, every
        edge vector r of the current graph becoming r + eps r -- applied to (v, Xi):
            h_pos = H v + Lambda Xi,   h_strain = Lambda^T v + B Xi,
        H = d2E/dpos2 (``hessian_vector_product``), Lambda = d2E/dpos deps (the force-strain coupling) and B = d2E/deps deps
        (the Born term, not divided by the volume).  ``v`` [N,3] or [K,N,3] (caller order), ``strain_v`` [3,3] or [K,3,3]; a
        None is zero; ``ValueError`` if both are None or their K differ.  -> (h_pos [N,3], h_strain [3,3]), or ([K,N,3],
        [K,3,3]) when the vectors carry a K; detached.  The graph arguments are those of ``forward``.  One forward, one first
        backward with ``create_graph=True``, one second backward per pair (``e3_edge_geometry_jvp_strained`` /
        ``e3_edge_geometry_hvp_strained`` close the chain).  Works on a frozen model in ``eval()``; no
        parameter gets a ``.grad``.  fp32: bf16 storage raises ``NotImplementedError``.  ``images``: as in ``forward`` and
        ``hessian_vector_product``; the strain is the global one of the open graph over the extended cloud, whose image
        positions carry their lattice shift, so every edge vector is the true one."""
        hp, hs, single, _ = self._strain_hvp(x, pos, r, lo, hi, periodic, cell, origin, v, strain_v, skin, neighbors, False,
                                             images)
        return (hp[0], hs[0]) if single else (hp, hs)

    def elastic_tensor(self, x: torch.Tensor, pos: torch.Tensor, r: float, lo=None, hi=None, periodic=True, cell=None,
                       origin=None, skin: float = 0.0, neighbors=None, images=False):
        """-> (born [3,3,3,3], coupling [N,3,3,3]) of the current graph (the graph arguments of ``forward``):
            born[a,b,c,d]     = (1/V) d2E/deps_ab deps_cd    the Born (clamped-ion) elastic tensor,
            coupling[i,k,a,b] = d2E/dpos_ik deps_ab          the force-strain coupling (internal-strain tensor), caller order,
        from ``strain_hessian_vector_product`` on the nine unit Xi: one forward, one first backward, nine second backwards.
        All three axes must be periodic, as for ``stress=True`` (the same ``ValueError``); V as in ``forward`` (L_x L_y L_z or
        |det cell|).  What it is NOT: it is the plain second derivative in the full 3x3 eps (nine independent components), not
        symmetrised -- ``voigt(born)`` contracts it with the symmetric strain basis -- and at a stressed state it differs from
        the stress-strain coefficients by terms in the stress.  The relaxed-ion constants are born - Lambda^T H^+ Lambda / V
        with ``hessian()``, left to the caller.  ``images``: as in ``forward`` (a small cell: V = |det cell|)."""
        unit = torch.eye(9, dtype=torch.float32, device=pos.device).view(9, 3, 3)
        hp, hs, _, V = self._strain_hvp(x, pos, r, lo, hi, periodic, cell, origin, None, unit, skin, neighbors, True, images)
        born = (hs.double() / V).float().view(3, 3, 3, 3).permute(2, 3, 0, 1).contiguous()   # hs[(c, d), a, b]
        coupling = hp.view(3, 3, pos.shape[0], 3).permute(2, 3, 0, 1).contiguous()             # hp[(a, b), i, k]
        return born, coupling

    def hessian(self, x: torch.Tensor, pos: torch.Tensor, r: float, lo=None, hi=None, periodic=True, cell=None, origin=None,
                skin: float = 0.0, neighbors=None, images=False) -> torch.Tensor:
        """The dense H [N,3,N,3] (``H[i,a,j,b]`` = d2E/dpos[i,a] dpos[j,b]): ``hessian_vector_product`` on the 3 N unit vectors
        in chunks.  ``ValueError`` above ``HESSIAN_MAX_ATOMS`` = 256 atoms: it is meant for molecules and small cells.
        ``images``: as in ``forward``; the limit counts the N particles, not their image rows."""
        return _dense_hessian(lambda vs: self.hessian_vector_product(x, pos, r, lo, hi, periodic, cell, origin, vs, skin=skin,
                                                                     neighbors=neighbors, images=images), pos)


class BatchedPeriodicEnergyModel(nn.Module):
    """SEGNN with a scalar node readout summed per structure over a BATCH of periodic structures, each with its own general
    cell: energies [B], and on request forces, per-structure virials and stresses, in one call (fitting a potential to a
    crystal dataset).  Every structure takes the image path of ``PeriodicEnergyModel(..., images=True)`` whatever its size:
    the cloud is extended by every structure's lattice images in one selection (``cell_images.BatchedCellImages``) and the
    open batched graph runs over it, so a cell may be smaller than the cutoff, up to 7 image shells per axis.  ``.net`` is the
    same ``SEGNN(..., "1x0e", ...)``: a state dict of the other energy models loads as it is.

    Not covered: ``neighbors=`` (a Verlet list over image rows), ``max_neighbors=``, ``hessian()``,
    ``strain_hessian_vector_product`` and ``elastic_tensor`` on a batch, a minimum-image fast path for the structures of a batch
    that are large enough for one, the sharded path, and bf16 storage with gradients (bf16 runs the fused inference call
    only)."""

    def __init__(self, in_irreps="1x0e+1x1o", hidden: int = 32, num_layers: int = 4, lmax: int = 2,
                 envelope: int | None = None):
        super().__init__()
        self.net = SEGNN(in_irreps, hidden, "1x0e", num_layers, lmax=lmax, envelope=envelope)

    def _image_cloud(self, x, pos, batch, r, cells, origins, skin):
        """-> (BatchedCellImages, SplitGraph, x, pos and structure of the extended cloud in graph order, the cutoff= of the
        net's forward)"""
        from .cell_images import batched_cell_image_graph
        cut = _cutoff_kw(self.net, r)
        return (*batched_cell_image_graph(pos, x, batch, _skin_radius(self.net, r, skin), cells, origins), cut)

    def forward(self, x: torch.Tensor, pos: torch.Tensor, batch: torch.Tensor, r: float, cells, origins=None,
                forces: bool = False, virial: bool = False, stress: bool = False, skin: float = 0.0,
                create_graph: bool = False):
        """x [N, in_dim], pos [N,3] (caller order, may be unwrapped), batch [N] the structure of every atom (any integer
        dtype, any order), cells [B,3,3] (rows = lattice vectors; a nested sequence or a CPU tensor) with origins [B,3]
        (None: zeros).  B comes from ``cells``: a structure without atoms is legal and has energy 0 and zero virial and
        stress.  -> energies [B], then whichever of forces [N,3] (= -dE/dpos, caller order), virials [B,3,3] (= -dE/deps_b
        at a zero strain per structure, not symmetrised) and stresses [B,3,3] (= (1/V_b) dE/deps_b, V_b = |det cell_b|) were
        requested, in that order; the energies alone when none was.  Energies only under ``no_grad`` run the fused inference
        kernels.

        ``skin``, ``create_graph``: as ``PeriodicEnergyModel.forward`` on its image path -- ``create_graph=True`` needs
        ``forces=True`` and a parameter that requires grad, and raises ``NotImplementedError`` with ``virial=True`` /
        ``stress=True`` and for bf16 storage.

        ``ValueError`` before any launch of the selection for a ``batch`` id outside [0, B), a structure above 7 image shells
        (the message names it), non-finite input; ``RuntimeError`` for CPU tensors."""
        if create_graph:
            _check_create_graph(self.net, x, forces, virial or stress)
        if pos.shape[0] == 0:
            return self._empty(x, pos, r, cells, origins, skin, forces, virial, stress)
        im, split, x_g, pos_g, structure_g, cut = self._image_cloud(x, pos, batch, r, cells, origins, skin)
        B = im.n_structures
        seg = batch.to(pos.device).long()
        if not (forces or virial or stress):
            e_node = self.net(x_g, split.graph, halo=im, split=split, **cut)[im.owned_new, 0]
            return torch.zeros(B, dtype=e_node.dtype, device=e_node.device).index_add_(0, seg, e_node)
        strained = virial or stress
        energy, gpos, geps = _energy_and_gradients(self.net, x_g, split.graph, pos_g, seg, B, forces, B if strained else 0,
                                                   structure_g if strained else None, cut, halo=im, split=split,
                                                   create_graph=create_graph)
        out = [energy]
        if forces:
            out.append(-im.reduce(gpos))
        if virial:
            out.append(-geps)
        if stress:
            V = torch.tensor(im.volumes, dtype=torch.float64, device=geps.device).view(B, 1, 1)
            out.append((geps.double() / V).float())
        return tuple(out)

    def _empty(self, x, pos, r, cells, origins, skin, forces, virial, stress):
        """``forward`` of a batch without atoms: the cells are checked as always, every output is zero, nothing is launched"""
        from .cell_images import BatchedCellImages
        if not pos.is_cuda:
            raise RuntimeError("BatchedCellImages.setup runs on ROCm tensors only; there is no CPU path")
        im = BatchedCellImages(cells, origins)
        im.plan(_skin_radius(self.net, r, skin))
        B = im.n_structures
        energy = torch.zeros(B, dtype=x.dtype, device=pos.device)
        if not (forces or virial or stress):
            return energy
        zeros = torch.zeros((B, 3, 3), dtype=torch.float32, device=pos.device)
        return (energy,) + ((torch.zeros_like(pos),) if forces else ()) + (zeros,) * (int(virial) + int(stress))

    def hessian_vector_product(self, x: torch.Tensor, pos: torch.Tensor, batch: torch.Tensor, r: float, cells, origins=None,
                               v: torch.Tensor | None = None, skin: float = 0.0) -> torch.Tensor:
        """H v, H = d2(sum of the energies)/dpos2 on the edge set of the current graph, block diagonal over the structures;
        ``v`` [N,3] or [K,N,3] in the caller's order -> a detached tensor of the shape of ``v``.  As
        ``PeriodicEnergyModel.hessian_vector_product`` on its image path: ``v`` is copied to the image rows (a direction has
        no lattice shift) and the product is reduced back to the N atoms, H = E^T H_ext E.  fp32: bf16 storage raises
        ``NotImplementedError``."""
        if pos.shape[0] == 0 and v is not None and v.dim() in (2, 3) and tuple(v.shape[-2:]) == (0, 3):
            return torch.zeros_like(v)                            # no atoms: nothing to reshape and nothing to launch
        vs = _check_vectors(v, pos)
        im, split, x_g, pos_g, _, cut = self._image_cloud(x, pos, batch, r, cells, origins, skin)
        hv = _hessian_vector_products(self.net, x_g, split.graph, pos_g, _image_vectors(im, vs.float()), cut, halo=im,
                                      split=split)
        return _reduce_vectors(im, hv).reshape(v.shape)


class ShardedEnergyModel(nn.Module):
    """``PeriodicEnergyModel``'s energy, forces, virial and stress for a cloud sharded over ranks by a ``sharding.GridHalo``
    (open or periodic) or ``MortonHalo``: every rank passes its OWNED particles and gets the total energy, the forces on
    its owned particles and the box's virial / stress.  ``.net`` is the same ``SEGNN(..., "1x0e", ...)``: a state dict of
    ``PeriodicEnergyModel`` loads as it is.  Gradients cross the ghost refresh of every layer by ``Halo.refresh``; an
    owned particle's force also collects what its ghost copies on other ranks (and its own periodic images) received
    (``Halo.reduce_ghosts``).  fp32, first order; the exchanges of the backward are not overlapped with compute.
    ``envelope`` (the exponent p, e.g. 6): the smooth cutoff envelope of ``PeriodicEnergyModel``; an enveloped model runs
    the per-product kernels with the blocking ghost refresh -- the overlap of the refresh with the interior edges belongs
    to the one-launch message kernel, which has no envelope."""

    def __init__(self, in_irreps="1x0e+1x1o", hidden: int = 32, num_layers: int = 4, lmax: int = 2,
                 envelope: int | None = None):
        super().__init__()
        self.net = SEGNN(in_irreps, hidden, "1x0e", num_layers, lmax=lmax, envelope=envelope)

    def forward(self, x: torch.Tensor, pos: torch.Tensor, r: float, halo, forces: bool = False, virial: bool = False,
                stress: bool = False, skin: float = 0.0, neighbors=None, create_graph: bool = False):
        """x [n, in_dim], pos [n,3] fp32: the particles this rank owns (``halo.owner_of``), caller order.  Every rank of
        the halo's group calls with the same flags.  -> the 0-d TOTAL energy (all-reduced), then whichever of forces
        [n,3] (= -dE_total/dpos of the owned particles, caller order), virial W [3,3] (= -dE_total/deps, all-reduced,
        not symmetrised) and stress [3,3] (= -W / V, V = the volume of the halo's box) were requested, in that order.
        ``stress=True`` needs a ``GridHalo`` periodic on all three axes (ValueError otherwise).

        With nothing requested under ``torch.no_grad()`` the fused inference path runs.  In training mode the energy
        returned is ``E_local + (E_total - E_local).detach()``: its value is the total, and ``loss.backward()`` on every
        rank -- each exactly once, the refreshes exchange gradients -- leaves each rank's share of dE_total/dtheta in
        ``.grad``; ``sharding.all_reduce_grads(model, halo.group)`` sums the shares.

        ``skin`` (enveloped models only): the halo is set up and the local graph built at ``r + skin`` -- the halo's
        cutoff checks apply to that radius -- while the envelope's radius stays ``r``; the outputs are those of
        ``skin = 0`` up to rounding.

        ``neighbors`` (a ``ShardedNeighborList(r, skin, halo)``): the local cloud is ``neighbors.update(pos, x)`` -- halo
        and graph built at the list's ``r + skin`` once, then positions sent along the stored entries and the stored
        edges pruned and split on the device while no particle on any rank has moved half the skin -- for any model,
        enveloped or not; ``r`` and ``halo`` must be the list's and ``skin`` stays 0 (ValueError otherwise).  May raise
        ``OwnershipChanged`` (on every rank) when the list has to rebuild.

        ``create_graph=True`` raises ``NotImplementedError``: the ghost refresh (``Halo.refresh``) is first order."""
        from .sharding import GridHalo, all_reduce_sum
        if create_graph:
            raise NotImplementedError("create_graph=True on the sharded path: the ghost refresh (Halo.refresh) is first order, "
                                      "its backward has no backward; train on forces with PeriodicEnergyModel")
        if stress and not (isinstance(halo, GridHalo) and halo.periodic == 7):
            raise ValueError("stress is defined for a GridHalo periodic on all three axes; use virial=True otherwise")
        cut = _cutoff_kw(self.net, r)
        if neighbors is not None:
            if float(r) != neighbors.r:
                raise ValueError(f"r = {r} is not the radius of neighbors= ({neighbors.r})")
            if halo is not neighbors.halo:
                raise ValueError("halo= is not the halo of neighbors=: the list holds the index state of the halo it was "
                                 "made with")
            if skin != 0.0:
                raise ValueError("skin= must stay 0 with neighbors=: the list has a skin of its own and returns the graph "
                                 "at r")
            cloud = neighbors.update(pos, x)
            split, x_g, pos_g = cloud.split, cloud.x, cloud.pos
        else:
            r = _skin_radius(self.net, r, skin)
            lpos, lx = halo.setup(pos, x, r)
            lo, hi = halo.local_bounds(r)
            g = radius_graph(lpos, r, lo, hi)            # open graph over [owned (wrapped) | ghosts and images]
            halo.renumber(g.perm)
            split = halo.split_graph(g)
            perm = g.perm.long()
            x_g, pos_g = lx[perm], lpos[perm]
        gpos = geps = None
        if not (forces or virial or stress):
            e_local = self.net(x_g, split.graph, halo=halo, split=split, **cut)[halo.owned_new, 0].sum()
        else:
            e_local, gpos, geps = _energy_and_gradients(self.net, x_g, split.graph, pos_g, None, 1, forces,
                                                        1 if (virial or stress) else 0, None, cut, halo=halo, split=split)
        parts = [e_local.detach().reshape(1)] + ([geps.reshape(9)] if geps is not None else [])
        total = all_reduce_sum(torch.cat(parts), halo.group)
        energy = total[0]
        if self.training and e_local.requires_grad:
            energy = e_local + (energy - e_local.detach())
        if not (forces or virial or stress):
            return energy
        out = [energy]
        if forces:
            out.append(-halo.reduce_ghosts(gpos))
        if virial:
            out.append(-total[1:].view(3, 3))
        if stress:
            V = math.prod(float(halo.hi[a]) - float(halo.lo[a]) for a in range(3))
            out.append((total[1:].view(3, 3).double() / V).float())
        return tuple(out)

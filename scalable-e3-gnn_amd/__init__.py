"""MI355X-native hot path of Scalable-E3-GNN (import name: ``scalable_e3_gnn_amd``).

The directory is called ``scalable-e3-gnn_amd`` (not a valid Python identifier); the repo-root
packages ``models`` / ``__graft_entry__`` / ``tests/conftest.py`` register it under the import name
``scalable_e3_gnn_amd`` via :func:`importlib` (see ``models/__init__.py``).

Public surface:
  * ``L1TensorProduct`` — drop-in for ``models.segnn.l1_tensor_prod.L1TensorProduct`` of the reference.
  * ``Irreps`` / ``Irrep`` / ``Instruction`` — e3nn-shaped bookkeeping (e3nn itself is optional).
  * ``NeighborList`` — Verlet list: a graph built at ``r + skin``, pruned to ``r`` on the device on every step.
  * ``ShardedEnergyModel`` — energy, forces, virial and stress of a cloud sharded over ranks (``sharding`` halos).
  * ``ShardedNeighborList`` / ``OwnershipChanged`` — the Verlet list of a sharded cloud: halo and local graph built at
    ``r + skin``, positions sent along the stored entries and the stored edges pruned and split on the device on every step;
    ``nl.redistribute(pos, x, *rows)`` before the model moves the particles that left their owner's region to their new rank
    when a rebuild is due (``Halo.migrate``), so a trajectory rebuilds through a crossing.
  * ``pack_rows`` / ``unpack_rows`` — the per-particle tensors of a caller as one int32 row table and back, bit for bit:
    what a migration moves (``sharding.Halo.migrate``, ``sharding.migrate_rows``).
  * ``CellImages`` / ``cell_image_graph`` — periodic cells below twice the cutoff: the cloud extended by explicit lattice image
    rows under an open graph (``PeriodicEnergyModel(...)(..., cell=, images=True | "auto")`` uses it).
  * ``BatchedPeriodicEnergyModel`` / ``BatchedCellImages`` / ``batched_cell_image_graph`` — a batch of periodic structures, each
    with its own cell, in one call: per-structure energies, forces, virials and stresses over one selection of image rows.
Everything computes through ``lib/libe3gnn_hip.so`` (C ABI: ``include/e3gnn.h``); there is no CPU path.
"""
from .irreps import Instruction, Irrep, Irreps, as_blocks  # noqa: F401
from .l1_tensor_prod import L1TensorProduct  # noqa: F401
from .neighbor_list import NeighborList  # noqa: F401
from .batched import BatchedPeriodicEnergyModel, ShardedEnergyModel  # noqa: F401
from .cell_images import BatchedCellImages, CellImages, batched_cell_image_graph, cell_image_graph  # noqa: F401
from .sharded_list import OwnershipChanged, ShardedNeighborList  # noqa: F401
from .sharding import pack_rows, unpack_rows  # noqa: F401

__all__ = ["L1TensorProduct", "Irreps", "Irrep", "Instruction", "as_blocks", "NeighborList", "ShardedEnergyModel",
           "ShardedNeighborList", "OwnershipChanged", "pack_rows", "unpack_rows", "CellImages", "cell_image_graph",
           "BatchedCellImages", "batched_cell_image_graph", "BatchedPeriodicEnergyModel"]

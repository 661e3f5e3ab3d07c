"""ctypes binding of ``libe3gnn_hip.so`` (C ABI declared in ``include/e3gnn.h``).

There is no fallback: if the shared library is missing or a call fails, a ``RuntimeError`` is raised.
``torch`` is imported first so that the HIP runtime already mapped by PyTorch-ROCm
(``libamdhip64.so``, same SONAME) is the one the library binds to — device pointers and streams then
belong to a single runtime.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_int, c_int32, c_int64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libe3gnn_hip.so")

E3_OK = 0
E3_F32, E3_F64, E3_BF16 = 0, 1, 2
CLS_NAMES = ("l0e", "l0o", "l1e", "l1o")

_lib = None

VoidP4 = c_void_p * 4
Float3 = ctypes.c_float * 3  # a host float[3] argument (periodic box lengths)
Float9 = ctypes.c_float * 9  # a host float[9] argument (a cell: rows = lattice vectors)
Int3 = c_int32 * 3           # a host int32[3] argument (cells per axis)


class HaloEntry(ctypes.Structure):
    """``e3_halo_entry`` of include/e3gnn.h: one ghost image's selection bounds and shift (fp32)."""
    _fields_ = [("lo", ctypes.c_float * 3), ("hi", ctypes.c_float * 3), ("shift", ctypes.c_float * 3)]


# name -> (restype, argtypes); mirrors include/e3gnn.h one to one
SIGNATURES = {
    "e3_abi_version": (c_int, []),
    "e3_status_string": (c_char_p, [c_int]),
    "e3_last_hip_error": (c_char_p, []),
    "e3_l1tp_plan_create": (c_int, [POINTER(c_int32), c_int, POINTER(c_int32), c_int, POINTER(c_void_p)]),
    "e3_l1tp_plan_destroy": (c_int, [c_void_p]),
    "e3_l1tp_in1_dim": (c_int, [c_void_p]),
    "e3_l1tp_out_dim": (c_int, [c_void_p]),
    "e3_l1tp_weight_shape": (c_int, [c_void_p, c_int, POINTER(c_int), POINTER(c_int)]),
    "e3_l1tp_norm_len": (c_int, [c_void_p, c_int]),
    "e3_l1tp_packed_bytes": (c_int64, [c_void_p, c_int]),
    "e3_l1tp_pack_weights": (c_int, [c_void_p, VoidP4, VoidP4, c_int, c_void_p, c_void_p]),
    "e3_l1tp_forward": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                c_int64, c_int, c_int, c_void_p]),
    "e3_l1tp_backward_workspace_bytes": (c_int64, [c_void_p, c_int64, c_int]),
    "e3_rg_grid": (c_int, [c_void_p]),
    "e3_rg_workspace_bytes": (c_int64, [c_int64, c_void_p]),
    "e3_rg_sort_count": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                 c_void_p]),
    "e3_rg_fill": (c_int, [c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "e3_edge_geometry": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "e3_gather_concat": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_int64, c_void_p, c_int, c_void_p,
                                 c_int64, c_void_p]),
    "e3_gate": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_int, c_void_p]),
    "e3_segment_sum": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p]),
    "e3_split_edges_workspace_bytes": (c_int64, [c_int64]),
    "e3_split_edges": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "e3_halo_select_workspace_bytes": (c_int64, [c_int64, c_int]),
    "e3_halo_select_count": (c_int, [c_void_p, c_int64, Float3, Float3, c_int32, ctypes.c_float, c_void_p, c_int, c_void_p,
                                     c_void_p, c_void_p, c_int64, c_void_p]),
    "e3_halo_select_fill": (c_int, [c_void_p, c_int64, Float3, Float3, c_int32, ctypes.c_float, c_void_p, c_int, c_int64,
                                    c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    # Morton-range halo (n_cells = int32[3], splitters = host int32[n_ranks + 1])
    "e3_morton_keys": (c_int, [c_void_p, c_int64, Float3, Float3, Int3, c_void_p, c_void_p]),
    "e3_morton_select_workspace_bytes": (c_int64, [c_int64, c_int]),
    "e3_morton_select_count": (c_int, [c_void_p, c_int64, Float3, Float3, Int3, ctypes.c_float, POINTER(c_int32), c_int,
                                       c_int, c_void_p, c_void_p, c_int64, c_void_p]),
    "e3_morton_select_fill": (c_int, [c_void_p, c_int64, Float3, Float3, Int3, ctypes.c_float, POINTER(c_int32), c_int,
                                      c_int, c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
    # migration between ranks (owner = device int32[n]; counts of the fill = host int32[n_ranks + 1])
    "e3_migrate_workspace_bytes": (c_int64, [c_int64, c_int]),
    "e3_migrate_count": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_int64, c_void_p]),
    "e3_migrate_fill": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_int, POINTER(c_int32), c_int64, c_int64,
                                c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "e3_tp_plan_create": (c_int, [POINTER(c_int32), c_int, c_int, POINTER(c_int32), c_int, POINTER(c_void_p)]),
    "e3_tp_plan_destroy": (c_int, [c_void_p]),
    "e3_tp_in1_dim": (c_int, [c_void_p]),
    "e3_tp_in2_dim": (c_int, [c_void_p]),
    "e3_tp_out_dim": (c_int, [c_void_p]),
    "e3_tp_weight_shape": (c_int, [c_void_p, c_int, POINTER(c_int), POINTER(c_int)]),
    "e3_tp_norm_len": (c_int, [c_void_p, c_int]),
    "e3_tp_packed_bytes": (c_int64, [c_void_p, c_int]),
    "e3_tp_pack_weights": (c_int, [c_void_p, c_void_p * 6, c_void_p * 6, c_int, c_void_p, c_void_p]),
    "e3_tp_forward": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64,
                              c_int, c_void_p, c_int, c_void_p]),
    "e3_tp_forward_fused": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64,
                                    c_int, c_int, c_void_p, c_void_p]),
    "e3_msg_plan_create": (c_int, [c_int, c_int, POINTER(c_void_p)]),
    "e3_msg_plan_destroy": (c_int, [c_void_p]),
    "e3_msg_packed_bytes": (c_int64, [c_void_p]),
    "e3_msg_premix_floats_per_node": (c_int64, [c_void_p]),
    "e3_msg_weight_shape": (c_int, [c_void_p, c_int, c_int, POINTER(c_int), POINTER(c_int)]),
    "e3_msg_supports": (c_int, [c_void_p, c_int]),
    "e3_msg_pack_weights": (c_int, [c_void_p, c_void_p * 3, c_void_p * 3, c_void_p * 3, c_void_p * 3, c_int, c_void_p,
                                    c_void_p]),
    "e3_msg_premix": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "e3_msg_premix_regions": (c_int, [c_void_p, c_int64, POINTER(c_int64), POINTER(c_int64), POINTER(c_int64)]),
    "e3_msg_refresh_rows": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int,
                                    c_void_p]),
    "e3_msg_forward": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p]),
    # owned sums: (..., dtype, tiles_per_block, workspace, workspace_bytes, out_scale4, target_log2[, box | cell], stream)
    "e3_msg_owned_workspace_bytes": (c_int64, [c_void_p, c_int64, c_int, c_int]),
    "e3_msg_forward_owned": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_int64, c_void_p,
                                     c_int, c_void_p]),
    "e3_msg_forward_owned_pbc": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_int64,
                                         c_void_p, c_int, Float3, c_void_p]),
    "e3_msg_forward_owned_cell": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_int64,
                                          c_void_p, c_int, Float9, c_void_p]),
    "e3_edge_geometry_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p]),
    # periodic boxes (box = float[3] of L per axis, 0 = open; periodic = axis bit mask)
    "e3_rg_sort_count_pbc": (c_int, [c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_int64, c_void_p]),
    "e3_rg_fill_pbc": (c_int, [c_int64, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "e3_edge_geometry_pbc": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, Float3, c_void_p, c_void_p, c_void_p,
                                     c_void_p]),
    "e3_edge_geometry_l2_pbc": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, Float3, c_void_p, c_void_p, c_void_p,
                                        c_void_p]),
    "e3_edge_geometry_backward_pbc": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, Float3, c_void_p, c_void_p,
                                              c_void_p, c_void_p, c_void_p]),
    "e3_msg_forward_pbc": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, Float3,
                                   c_void_p]),
    # general periodic cells (cell = float[9], rows = lattice vectors; origin = float[3])
    "e3_cell_derive": (c_int, [Float9, Float9, Float3, POINTER(ctypes.c_float)]),
    "e3_rg_sort_count_cell": (c_int, [c_void_p, c_int64, c_void_p, Float9, Float3, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_int64, c_void_p]),
    "e3_rg_fill_cell": (c_int, [c_int64, c_void_p, Float9, Float3, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                c_void_p]),
    # capped rows, the k nearest inside r (rowptr_full, N, k, rowptr_capped, stats[2] int64, workspace, bytes, stream), and
    # the fills of the three modes (..., sorted_pos4, rowptr_capped, k, src, workspace, bytes, stream)
    "e3_rg_cap_workspace_bytes": (c_int64, [c_int64]),
    "e3_rg_cap_rowptr": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "e3_rg_fill_nearest": (c_int, [c_int64, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int64, c_void_p]),
    "e3_rg_fill_nearest_pbc": (c_int, [c_int64, c_void_p, c_int32, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int64,
                                       c_void_p]),
    "e3_rg_fill_nearest_cell": (c_int, [c_int64, c_void_p, Float9, Float3, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                        c_int64, c_void_p]),
    "e3_edge_geometry_cell": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, Float9, c_void_p, c_void_p, c_void_p,
                                      c_void_p]),
    "e3_edge_geometry_l2_cell": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, Float9, c_void_p, c_void_p, c_void_p,
                                         c_void_p]),
    "e3_edge_geometry_backward_cell": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, Float9, c_void_p, c_void_p,
                                               c_void_p, c_void_p, c_void_p]),
    "e3_msg_forward_cell": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, Float9,
                                    c_void_p]),
    "e3_edge_geometry_strained_cell": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, Float9, c_void_p, c_void_p,
                                               c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "e3_edge_geometry_backward_strained_cell": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, Float9, c_void_p,
                                                        c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                        c_void_p, c_int64, c_void_p]),
    "e3_gather_concat_backward": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64,
                                          c_void_p, c_void_p]),
    "e3_gate_blocks_backward": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_int,
                                        POINTER(c_int32), POINTER(c_int32), c_void_p]),
    "e3_segment_sum_backward": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p]),
    "e3_pow2_scale": (c_int, [c_void_p, POINTER(c_int64), c_int, c_int, c_void_p, c_void_p]),
    "e3_add_pow2_scale": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "e3_tp_backward": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p,
                               c_int64, c_void_p, c_int64, c_void_p * 6, c_int64, c_int, c_void_p]),
    "e3_tp_backward_weights": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p,
                                       c_int64, c_int, c_void_p]),
    "e3_tp_backward_operands": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p,
                                        c_void_p, c_int64, c_int, c_void_p]),
    "e3_tp_backward_contract": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p,
                                        c_int64, c_int64, c_int, c_void_p]),
    "e3_tp_forward_fused_epilogue": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                             c_int64, c_int, c_int, c_void_p, c_void_p, c_int64, c_void_p, c_int, c_void_p]),
    "e3_tp_forward_update_pair": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int64, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_void_p, c_int,
                                          c_void_p]),
    "e3_tp_fused_supported": (c_int, [c_void_p, c_int]),
    "e3_tp_last_fused_kernel": (ctypes.c_char_p, []),
    "e3_tp_forward_fused_scatter": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                            c_int64, c_int64, c_int, c_int, c_void_p, c_void_p]),
    "e3_segment_sum_bf16": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p]),
    "e3_edge_geometry_l2": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "e3_gate_blocks": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_int, POINTER(c_int32),
                               POINTER(c_int32), c_void_p]),
    "e3_l1tp_backward": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, VoidP4, VoidP4, c_void_p, c_int64,
                                 c_void_p, c_int64, c_void_p, VoidP4, c_void_p, c_int64, c_int, c_void_p]),
    # per-structure strain (box = float[3] as above, or NULL for an open box)
    "e3_edge_geometry_strained": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, POINTER(ctypes.c_float), c_void_p,
                                          c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "e3_edge_geometry_backward_strained_workspace_bytes": (c_int64, [c_int64]),
    "e3_edge_geometry_backward_strained": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, POINTER(ctypes.c_float),
                                                   c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                                   c_void_p, c_void_p, c_int64, c_void_p]),
    # smooth cutoff envelope (r_c = float, p = int) and the weighted segment-sum pair
    "e3_cutoff_envelope": (c_int, [c_void_p, c_int64, ctypes.c_float, c_int, c_void_p, c_void_p]),
    "e3_cutoff_envelope_backward": (c_int, [c_void_p, c_void_p, c_int64, ctypes.c_float, c_int, c_void_p, c_void_p]),
    "e3_segment_sum_weighted": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64,
                                        c_void_p]),
    "e3_segment_sum_weighted_backward": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int,
                                                 c_void_p, c_int64, c_void_p, c_void_p]),
    # second derivatives: tangent of the edge geometry along v [N,3] (..., lmax[, box | cell], v, dY, dd, dA, stream), and the
    # backward of the gate's and the envelope's backward
    "e3_edge_geometry_jvp": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p]),
    "e3_edge_geometry_jvp_pbc": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, Float3, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p]),
    "e3_edge_geometry_jvp_cell": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, Float9, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p]),
    # ... and its backward in the positions (..., lmax[, box | cell], gY, gd, gA, v, h_pos, stream)
    "e3_edge_geometry_hvp": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p]),
    "e3_edge_geometry_hvp_pbc": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, Float3, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p]),
    "e3_edge_geometry_hvp_cell": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, Float9, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p]),
    # the strained pair (..., lmax, box | NULL or cell, strain, structure, S, [gY, gd, gA,] v, xi, outputs[, workspace, bytes],
    # stream)
    "e3_edge_geometry_jvp_strained": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, POINTER(ctypes.c_float), c_void_p,
                                              c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "e3_edge_geometry_jvp_strained_cell": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, Float9, c_void_p, c_void_p,
                                                   c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "e3_edge_geometry_hvp_strained": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, POINTER(ctypes.c_float), c_void_p,
                                              c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_void_p, c_int64, c_void_p]),
    "e3_edge_geometry_hvp_strained_cell": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, Float9, c_void_p, c_void_p,
                                                   c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                   c_void_p, c_void_p, c_int64, c_void_p]),
    "e3_gate_blocks_backward2": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p,
                                         c_int64, c_int64, c_int, c_int, POINTER(c_int32), POINTER(c_int32), c_void_p]),
    "e3_cutoff_envelope_backward2": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, ctypes.c_float, c_int, c_void_p, c_void_p,
                                             c_void_p]),
    # Verlet neighbour list: the stored graph pruned to r at the current positions (r = float)
    "e3_nl_workspace_bytes": (c_int64, [c_int64]),
    "e3_nl_update": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, ctypes.c_float, c_void_p,
                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "e3_nl_update_pbc": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, ctypes.c_float, Float3,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "e3_nl_update_cell": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, ctypes.c_float, Float9,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    # ... and the same walk with the shard's edge split (is_ghost after src; seven lists, stats [4])
    "e3_nl_update_split_workspace_bytes": (c_int64, [c_int64]),
    "e3_nl_update_split": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                                   ctypes.c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p]),
    # differentiable ghost refresh: out-of-place row copy by slot, and its backward (row sum over a CSR of the send list)
    "e3_halo_refresh": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int, c_int, c_void_p,
                                c_int64, c_void_p]),
    "e3_halo_reduce": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int,
                               c_int, c_void_p, c_int64, c_void_p]),
    # image rows of a small periodic cell: (cell, origin, r, shells int32[3], rho), the count / fill pair of the selection
    # (pos, N, cell, origin, r, ...) and the row pair (rows, ld, source, [shift, cell | ptr, rows, n_rows], M, D, dtype, out, ld)
    "e3_cell_images_plan": (c_int, [Float9, Float3, ctypes.c_float, Int3, POINTER(ctypes.c_float)]),
    "e3_cell_images_workspace_bytes": (c_int64, [c_int64]),
    "e3_cell_images_count": (c_int, [c_void_p, c_int64, Float9, Float3, ctypes.c_float, c_void_p, c_void_p, c_void_p, c_int64,
                                     c_void_p]),
    "e3_cell_images_fill": (c_int, [c_void_p, c_int64, Float9, Float3, ctypes.c_float, c_void_p, c_int64, c_void_p, c_void_p,
                                    c_void_p, c_void_p]),
    # ... and a batch of cells: (cells [B,9], origins [B,3], B, r, shells [B,3], rho [B], table) on the host, then
    # (pos, structure, N, table, table_host, counts [B] int64, B, ...) as the single pair
    "e3_cell_images_record_bytes": (c_int64, []),
    "e3_cell_images_plan_batch": (c_int, [c_void_p, c_void_p, c_int64, ctypes.c_float, c_void_p, c_void_p, c_void_p]),
    "e3_cell_images_count_batch": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                                           c_void_p, c_void_p, c_int64, c_void_p]),
    "e3_cell_images_fill_batch": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64,
                                          c_void_p, c_void_p, c_void_p, c_void_p]),
    "e3_image_rows_expand": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, POINTER(ctypes.c_float), c_int64, c_int, c_int,
                                     c_void_p, c_int64, c_void_p]),
    "e3_image_rows_reduce": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_void_p,
                                     c_int64, c_void_p]),
}


def load():
    """Load (once) and return the ctypes handle.  Raises RuntimeError when the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP library has not been built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C scalable-e3-gnn_amd/csrc`). "
            "There is no CPU fallback.")
    import torch  # noqa: F401  (maps PyTorch's libamdhip64 before ours is resolved)

    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            continue  # entry points that are declared but land later are reported by tests
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status: int, what: str = ""):
    if status != E3_OK:
        lib = load()
        msg = lib.e3_status_string(status).decode()
        if status == 5:
            msg += " — " + lib.e3_last_hip_error().decode()
        raise RuntimeError(f"libe3gnn_hip: {what}: {msg} (status {status})")


def call(name: str, *args):
    """Call the entry ``name`` and check its status: a failure names the entry that was called."""
    check(getattr(load(), name)(*args), name)


def blocks_array(blocks):
    flat = [int(v) for b in blocks for v in b]
    return (c_int32 * len(flat))(*flat), len(blocks)


def ptr4(tensors):
    """4-entry void* array from a list of 4 optional tensors."""
    return VoidP4(*[(t.data_ptr() if (t is not None and t.numel() > 0) else None) for t in tensors])


def dtype_code(dtype) -> int:
    import torch

    try:
        return {torch.float32: E3_F32, torch.float64: E3_F64, torch.bfloat16: E3_BF16}[dtype]
    except KeyError:
        raise RuntimeError(f"libe3gnn_hip supports float32 / float64 / bfloat16, got {dtype}") from None


class DevicePlans:
    """Plan handles of one operator, one per device (a C plan keeps its tables on the device that was current at its
    first use and rejects calls from any other).  Holds only the constructor arguments as state: ``copy.deepcopy``,
    ``pickle`` and ``torch.save(module)`` rebuild an empty holder, and handles are created lazily -- two owners never
    share (and double-free) a handle."""

    def __init__(self, create_name: str, destroy_name: str, *args):
        self._create, self._destroy_name, self._args = create_name, destroy_name, args
        self._handles = {}

    def _make(self):
        lib = load()
        cargs = []
        for a in self._args:
            if isinstance(a, (list, tuple)):
                arr, n = blocks_array(a)
                cargs += [arr, n]
            else:
                cargs.append(int(a))
        h = c_void_p()
        check(getattr(lib, self._create)(*cargs, ctypes.byref(h)), self._create)
        return h

    def handle(self, device=None) -> c_void_p:
        """The handle for ``device`` (a torch.device / index; None = a host-only handle for shape queries)."""
        key = -1
        if device is not None:
            import torch
            key = torch.device(device).index
            if key is None:
                key = torch.cuda.current_device()
        h = self._handles.get(key)
        if h is None:
            h = self._handles[key] = self._make()
        return h

    def __deepcopy__(self, memo):
        return DevicePlans(self._create, self._destroy_name, *self._args)

    def __reduce__(self):
        return (DevicePlans, (self._create, self._destroy_name) + tuple(self._args))

    def __del__(self):
        try:
            lib = load()
            for h in self._handles.values():
                if h:
                    getattr(lib, self._destroy_name)(h)
            self._handles = {}
        except Exception:
            pass


class PackedCache:
    """Packed weight images of one operator, one slot per ``(dtype, device)``.  A slot is rebuilt when the
    ``(data_ptr, _version)`` of one of the tensors it was packed from changes: a replaced tensor and in-place operations
    (``mul_``, ``copy_``, an optimizer step, ``load_state_dict``) are seen; writes through ``.data`` do not advance
    ``_version`` and need ``invalidate()``.  A stream other than the one that packed waits for the pack's event.
    Copies and pickles as an empty cache (an event cannot be copied, and two owners never share a buffer)."""

    def __init__(self):
        self._slots = {}

    def get(self, tensors, dtype, device, pack):
        """``pack(stream)`` checks the tensors, launches the pack on ``stream`` (the raw handle of the current stream of
        ``device``) and returns the buffer; it runs only when the slot is missing or stale."""
        import torch
        key = tuple((t.data_ptr(), t._version) if t is not None else None for t in tensors)
        stream = torch.cuda.current_stream(device)
        hit = self._slots.get((dtype, device))
        if hit is not None and hit[0] == key:
            if hit[2] != stream.cuda_stream:
                stream.wait_event(hit[3])  # packed on another stream: order this stream behind the pack kernels
            return hit[1]
        packed = pack(stream.cuda_stream)
        ev = torch.cuda.Event()
        ev.record(stream)
        self._slots[(dtype, device)] = (key, packed, stream.cuda_stream, ev)
        return packed

    def peek(self, tensors, dtype, device):
        """The slot's buffer when it was packed from exactly these tensors (same ``(data_ptr, _version)``), else None; never
        packs and never replaces the slot."""
        import torch
        hit = self._slots.get((dtype, device))
        if hit is None or hit[0] != tuple((t.data_ptr(), t._version) if t is not None else None for t in tensors):
            return None
        stream = torch.cuda.current_stream(device)
        if hit[2] != stream.cuda_stream:
            stream.wait_event(hit[3])
        return hit[1]

    def invalidate(self):
        self._slots = {}

    def __deepcopy__(self, memo):
        return PackedCache()

    def __reduce__(self):
        return (PackedCache, ())

"""Capped radius graph, host side (no GPU): the numpy restatement (tests/nearest_reference.py) against a plain fp64
k-nearest on a cloud without fp32 ties, the argument checks of ``radius_graph(max_neighbors=)`` -- refused before anything
touches a device -- the ABI's argument checks, and the new fields of ``RadiusGraph``."""
import dataclasses

import numpy as np
import pytest
import torch

import capped_cases as C
import nearest_reference as K
from scalable_e3_gnn_amd import _lib
from scalable_e3_gnn_amd.batched import batched_radius_graph
from scalable_e3_gnn_amd.radius_graph import RadiusGraph, grid_params, radius_graph

E3_ERR_INVALID_ARG = 1


@pytest.mark.parametrize("k", [1, 16, 32, 64])
def test_reference_equals_fp64_k_nearest(k):
    """Uniform N = 2000, seed 3: no two neighbours of a row tie on the fp32 d2 (asserted), so the order by (d2, id) in fp32
    is the order by distance in fp64."""
    perm, pos4, rowptr, src, _, _ = C.uncapped("open")
    d2, dst = K.edge_d2(pos4, rowptr, src)
    order = np.lexsort((d2, dst))
    assert not np.any((dst[order][1:] == dst[order][:-1]) & (d2[order][1:] == d2[order][:-1])), "the cloud has fp32 ties"
    _, _, rowptr_c, src_c, cut, full, deg = C.capped("open", k)
    rp64, src64 = K.knn64(pos4, C.R_UNIFORM, k)
    assert np.array_equal(rowptr_c, rp64) and np.array_equal(src_c, src64)
    assert cut == int((deg > k).sum()) and full == len(src)
    if k == 64:
        assert cut == 0 and np.array_equal(rowptr_c, rowptr) and np.array_equal(src_c, src)


def test_reference_cloud_has_rows_below_at_and_above_the_cap():
    deg = C.capped("open", 16)[6]
    assert deg.min() == 2 and deg.max() == 43
    assert ((deg < 16).sum(), (deg == 16).sum(), (deg > 16).sum()) == (437, 92, 1471)


@pytest.mark.parametrize("bad", [0, 65, 2.5, True, -1, "8"])
def test_max_neighbors_is_checked_before_anything_runs(bad):
    pos = torch.zeros(4, 3)   # a CPU tensor: anything past the check would raise RuntimeError instead
    with pytest.raises(ValueError, match="max_neighbors"):
        radius_graph(pos, 0.1, max_neighbors=bad)
    with pytest.raises(ValueError, match="max_neighbors"):
        radius_graph(pos, 0.1, cell=np.eye(3).tolist(), max_neighbors=bad)
    with pytest.raises(ValueError, match="max_neighbors"):
        radius_graph(pos, 0.1, C.LO, C.HI, periodic=True, max_neighbors=bad)
    with pytest.raises(ValueError, match="max_neighbors"):
        batched_radius_graph(pos, torch.zeros(4, dtype=torch.long), 0.1, max_neighbors=bad)


def test_valid_cap_still_needs_a_device_tensor():
    with pytest.raises(RuntimeError, match="ROCm"):
        radius_graph(torch.zeros(4, 3), 0.1, max_neighbors=8)


def test_graph_fields_default_to_the_uncapped_graph():
    z = torch.zeros(3, dtype=torch.int32)
    g = RadiusGraph(z[:2], torch.zeros(2, 4), z, z[:0], 0, ((1, 1, 1), 1))
    assert g.max_neighbors is None and g.truncated == 0 and g.full_edges == 0
    g = RadiusGraph(z[:2], torch.zeros(2, 4), z, torch.zeros(5, dtype=torch.int32), 5, ((1, 1, 1), 1), (1.0, 0.0, 2.0))
    assert g.full_edges == 5 and g.box == (1.0, 0.0, 2.0)
    h = dataclasses.replace(g, pos4=torch.ones(2, 4))
    assert h.full_edges == 5 and h.max_neighbors is None
    c = dataclasses.replace(g, max_neighbors=4, truncated=1, full_edges=9)
    assert (c.max_neighbors, c.truncated, c.full_edges, c.num_edges) == (4, 1, 9, 5)


def test_abi_rejects_bad_cap_arguments():
    """k outside [1, 64] or a NULL pointer: E3_ERR_INVALID_ARG before any launch (so this runs without a GPU; the pointers
    that are not NULL are never dereferenced)."""
    lib = _lib.load()
    p = grid_params(C.LO, C.HI, 0.1)
    import ctypes
    pp, some = ctypes.byref(p), 256
    assert lib.e3_rg_cap_workspace_bytes(-1) == -1 and lib.e3_rg_cap_workspace_bytes(1000) >= 4004
    for k in (0, 65, -3):
        assert lib.e3_rg_cap_rowptr(some, 10, k, some, some, some, 1 << 20, None) == E3_ERR_INVALID_ARG
        assert lib.e3_rg_fill_nearest(10, pp, some, some, k, some, some, 1 << 30, None) == E3_ERR_INVALID_ARG
        assert lib.e3_rg_fill_nearest_pbc(10, pp, 7, some, some, k, some, some, 1 << 30, None) == E3_ERR_INVALID_ARG
        assert lib.e3_rg_fill_nearest_cell(10, pp, _lib.Float9(1, 0, 0, 0, 1, 0, 0, 0, 1), _lib.Float3(0, 0, 0), some, some,
                                           k, some, some, 1 << 30, None) == E3_ERR_INVALID_ARG
    for hole in range(4):   # rowptr_full, rowptr_capped, stats, workspace
        args = [some, some, some, some]
        args[hole] = None
        assert lib.e3_rg_cap_rowptr(args[0], 10, 8, args[1], args[2], args[3], 1 << 20, None) == E3_ERR_INVALID_ARG
    assert lib.e3_rg_cap_rowptr(some, 10, 8, some, some, some, 8, None) == E3_ERR_INVALID_ARG   # workspace too small
    for hole in range(4):   # sorted_pos4, rowptr_capped, src, workspace
        args = [some, some, some, some]
        args[hole] = None
        assert lib.e3_rg_fill_nearest(10, pp, args[0], args[1], 8, args[2], args[3], 1 << 30, None) == E3_ERR_INVALID_ARG
    assert lib.e3_rg_fill_nearest(10, None, some, some, 8, some, some, 1 << 30, None) == E3_ERR_INVALID_ARG
    assert lib.e3_rg_fill_nearest(10, pp, some, some, 8, some, some, 16, None) == E3_ERR_INVALID_ARG   # workspace too small

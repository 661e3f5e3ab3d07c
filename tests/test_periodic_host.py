"""Periodic boxes without a GPU: self-checks of the numpy restatement (tests/pbc_reference.py) of the wrap and the
minimum-image edge test, the C ABI entries and their bindings, and the argument checks of radius_graph(periodic=)."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from oracle import graph_oracle as G
import pbc_reference as P
from scalable_e3_gnn_amd import _lib
from scalable_e3_gnn_amd.radius_graph import RadiusGraph, periodic_mask, radius_graph

NEW_ENTRIES = ["e3_rg_sort_count_pbc", "e3_rg_fill_pbc", "e3_edge_geometry_pbc", "e3_edge_geometry_l2_pbc",
               "e3_edge_geometry_backward_pbc", "e3_msg_forward_pbc"]


def _adj(rowptr, src):
    N = len(rowptr) - 1
    dst = np.repeat(np.arange(N), np.diff(rowptr))
    return set(zip(src.tolist(), dst.tolist()))


def test_restatement_symmetric_without_self_edges():
    rng = np.random.default_rng(0)
    pos = rng.random((1500, 3)).astype(np.float32)
    pos[:200] *= np.float32(0.05)  # a corner cluster: many pairs across the faces
    perm, pos4, rowptr, src = P.graph_pbc(pos, [0, 0, 0], [1, 1, 1], 0.09, True)
    e = _adj(rowptr, src)
    assert len(e) == len(src) > 0
    assert all(s != d for s, d in e)
    assert all((d, s) in e for s, d in e)
    assert all(np.all(np.diff(src[rowptr[i]:rowptr[i + 1]]) > 0) for i in range(len(rowptr) - 1))
    w = pos4[:, :3]
    assert np.all(w >= 0) and np.all(w < 1)
    # the face deficit of the open box is gone: strictly more edges than the open graph of the same cloud
    assert len(src) > len(G.graph(pos, [0, 0, 0], [1, 1, 1], 0.09)[2])


def test_restatement_lattice_translation_invariant():
    rng = np.random.default_rng(1)
    pos = (rng.integers(0, 64, size=(800, 3)) / 64.0).astype(np.float32)  # dyadic: every shift below is exact
    pos = np.unique(pos, axis=0)
    base = P.graph_pbc(pos, [0, 0, 0], [1, 1, 1], 0.1, True)
    for shift in ([1, 0, 0], [-2, 3, 1], [5, -7, 0]):
        got = P.graph_pbc(pos + np.float32(1) * np.asarray(shift, np.float32), [0, 0, 0], [1, 1, 1], 0.1, True)
        for a, b in zip(base, got):
            assert np.array_equal(a, b)


def test_restatement_equals_open_brute_force_away_from_faces():
    rng = np.random.default_rng(2)
    pos = rng.random((1200, 3)).astype(np.float32)
    r = 0.08
    perm, pos4, rowptr, src = P.graph_pbc(pos, [0, 0, 0], [1, 1, 1], r, True)
    # the open-box brute force of the C oracle on the same ordering
    _, o_rowptr, o_src = G.graph(pos, [0, 0, 0], [1, 1, 1], r, method="bruteforce")
    o_perm, _ = G.order(pos, G.params([0, 0, 0], [1, 1, 1], r))
    assert np.array_equal(o_perm, perm)  # positions inside [0, 1): the wrap is the identity
    inner = np.all((pos4[:, :3] > 2 * r) & (pos4[:, :3] < 1 - 2 * r), axis=1)
    keep = lambda es: {(s, d) for s, d in es if inner[s] and inner[d]}
    assert keep(_adj(rowptr, src)) == keep(_adj(o_rowptr, o_src))
    assert len(keep(_adj(rowptr, src))) > 500


def test_header_and_bindings_list_the_periodic_entries():
    text = open(os.path.join(REPO, "include", "e3gnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"#define E3GNN_ABI_VERSION 3\b", open(os.path.join(REPO, "include", "e3gnn.h")).read())


def test_library_rejects_invalid_boxes():
    """The *_pbc entries check the box before anything is launched (NULL device pointers are never touched)."""
    lib = _lib.load()
    bad = [(-1.0, 0.0, 0.0), (float("nan"), 1.0, 1.0), (float("inf"), 1.0, 1.0)]
    for box in bad:
        b = _lib.Float3(*box)
        assert lib.e3_edge_geometry_pbc(None, None, None, 10, b, None, None, None, None) == 1
        assert lib.e3_edge_geometry_l2_pbc(None, None, None, 10, b, None, None, None, None) == 1
        assert lib.e3_edge_geometry_backward_pbc(None, None, None, 10, 1, b, None, None, None, None, None) == 1
        assert lib.e3_msg_forward_pbc(None, None, 0, 10, None, None, None, 0, None, None, None, None, 0, 0, 0, 0, b,
                                      None) == 1
    from scalable_e3_gnn_amd.radius_graph import RgParams
    import ctypes
    p = RgParams()
    for a in range(3):
        p.lo[a], p.hi[a] = 0.0, 1.0
    p.r = 0.5  # 2 r = L
    assert lib.e3_rg_grid(ctypes.byref(p)) == 0
    for mask in (1, 2, 4, 7):
        assert lib.e3_rg_sort_count_pbc(None, 10, ctypes.byref(p), mask, None, None, None, None, 0, None) == 1
        assert lib.e3_rg_fill_pbc(10, ctypes.byref(p), mask, None, None, None, None, 0, None) == 1
    assert lib.e3_rg_sort_count_pbc(None, 10, ctypes.byref(p), 8, None, None, None, None, 0, None) == 1


def test_radius_graph_argument_checks():
    pos = torch.zeros(10, 3)  # a CPU tensor: every check below fires before the device is looked at
    with pytest.raises(ValueError, match="lo and hi"):
        radius_graph(pos, 0.1, periodic=True)
    with pytest.raises(ValueError, match="lo and hi"):
        radius_graph(pos, 0.1, lo=[0, 0, 0], periodic=(True, False, False))
    with pytest.raises(ValueError, match="2 r < L"):
        radius_graph(pos, 0.5, [0, 0, 0], [1, 1, 1], periodic=True)
    with pytest.raises(ValueError, match="2 r < L"):
        radius_graph(pos, 0.3, [0, 0, 0], [1, 0.6, 1], periodic=(False, True, False))
    with pytest.raises(ValueError, match="3 bools"):
        radius_graph(pos, 0.1, [0, 0, 0], [1, 1, 1], periodic=(True, True))
    # an open axis may be narrower than 2 r
    assert periodic_mask((True, False, True), 0.3, [0, 0, 0], [1, 0.5, 1]) == 5
    assert periodic_mask(False, 0.3, None, None) == 0


def test_radius_graph_keeps_positional_construction():
    g = RadiusGraph(torch.zeros(2, dtype=torch.int32), torch.zeros(2, 4), torch.zeros(3, dtype=torch.int32),
                    torch.zeros(0, dtype=torch.int32), 0, ((1, 1, 1), 1))
    assert g.box is None and g.box_arg is None
    g2 = RadiusGraph(g.perm, g.pos4, g.rowptr, g.src, 0, g.grid, (1.0, 0.0, 2.0))
    assert list(g2.box_arg) == [1.0, 0.0, 2.0]

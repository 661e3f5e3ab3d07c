"""General periodic cells, the part that needs no GPU: heights, volume and ``cell_from_lengths_angles`` against closed
forms, every argument error of ``radius_graph(cell=)``, and the numpy restatement of the builder
(tests/triclinic_reference.py) against an fp64 brute-force search over the 27 lattice images."""
import math

import numpy as np
import pytest
import torch

import triclinic_reference as R
from scalable_e3_gnn_amd.radius_graph import cell_check_cutoff, cell_from_lengths_angles, cell_params, radius_graph


def test_cubic_cell():
    cell = cell_from_lengths_angles(2.0, 2.0, 2.0, 90, 90, 90)
    assert cell == [[2.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 2.0]]
    c9, o3, hgt, vol = cell_params(cell)
    assert c9 == (2.0, 0, 0, 0, 2.0, 0, 0, 0, 2.0) and o3 == (0.0, 0.0, 0.0)
    assert hgt == (2.0, 2.0, 2.0) and vol == 8.0


def test_hexagonal_cell():
    a, c = 3.0, 5.0
    cell = cell_from_lengths_angles(a, a, c, 90, 90, 120)
    want = [[a, 0, 0], [-a / 2, a * math.sqrt(3) / 2, 0], [0, 0, c]]
    assert np.allclose(cell, want, rtol=0, atol=1e-15)
    assert cell[0][1] == 0.0 and cell[0][2] == 0.0 and cell[1][2] == 0.0 and cell[2][0] == 0.0 and cell[2][1] == 0.0
    _, _, hgt, vol = cell_params(cell)
    assert np.allclose(hgt, [a * math.sqrt(3) / 2, a * math.sqrt(3) / 2, c], rtol=2e-7)
    assert abs(vol - a * a * c * math.sqrt(3) / 2) < 2e-7 * vol


def test_general_angles_reproduce_lengths_and_angles():
    cell = np.array(cell_from_lengths_angles(3.0, 4.0, 5.0, 70, 80, 100))
    assert np.allclose(np.linalg.norm(cell, axis=1), [3.0, 4.0, 5.0])
    ang = lambda u, v: math.degrees(math.acos(u @ v / np.linalg.norm(u) / np.linalg.norm(v)))
    assert np.allclose([ang(cell[1], cell[2]), ang(cell[0], cell[2]), ang(cell[0], cell[1])], [70, 80, 100])
    assert cell[2, 2] > 0 and np.allclose(np.triu(cell, 1), 0)
    with pytest.raises(ValueError):
        cell_from_lengths_angles(1, 1, 1, 30, 30, 120)  # coplanar and beyond
    with pytest.raises(ValueError):
        cell_from_lengths_angles(1, 1, 1, 90, 90, 180)


def test_cell_t_numbers():
    _, _, hgt, vol = cell_params(R.T.tolist())
    assert vol == 0.65625
    # h_a = V / |a_b x a_c|
    want = [0.65625 / np.linalg.norm(np.cross(R.T[(a + 1) % 3], R.T[(a + 2) % 3])) for a in range(3)]
    assert np.allclose(hgt, want, rtol=2e-7)
    assert [round(float(h), 3) for h in hgt] == [0.932, 0.830, 0.750]
    _, _, hp, vp = cell_params(R.TP.tolist())
    assert vp == 0.65625 and [round(float(h), 3) for h in hp] == [0.932, 0.538, 0.533]
    # the library's derived values are the reference's, bit for bit; a tensor is taken like a nested list
    g, h, v = R.derive(R.T)
    assert tuple(float(t) for t in h) == hgt and float(v) == vol
    assert cell_params(torch.as_tensor(R.T))[2] == hgt


def test_argument_errors():
    pos = torch.zeros(4, 3)  # checked after the cell: none of these reaches the device
    hmin = min(cell_params(R.T.tolist())[2])
    for r in (hmin / 2, hmin, 0.0, -1.0):
        with pytest.raises(ValueError, match="height"):
            radius_graph(pos, r, cell=R.T.tolist())
    with pytest.raises(ValueError) as e:
        cell_check_cutoff(cell_params(R.T.tolist())[2], 0.4)
    assert "0.75" in str(e.value)  # the heights are in the message
    for singular in ([[1, 0, 0], [2, 0, 0], [0, 0, 1]], [[0, 0, 0]] * 3, [[1, 0, 0], [0, float("inf"), 0], [0, 0, 1]],
                     [[1, 0, 0], [0, float("nan"), 0], [0, 0, 1]]):
        with pytest.raises(ValueError, match="singular"):
            radius_graph(pos, 0.1, cell=singular)
    for bad in ([[1, 0, 0], [0, 1, 0]], [1, 2, 3], [[1, 0], [0, 1], [0, 0]], torch.eye(4)):
        with pytest.raises(ValueError, match="3 x 3"):
            radius_graph(pos, 0.1, cell=bad)
    for kw in (dict(lo=[0, 0, 0]), dict(hi=[1, 1, 1]), dict(lo=[0, 0, 0], hi=[1, 1, 1]), dict(periodic=True),
               dict(periodic=(True, True, True))):
        with pytest.raises(ValueError, match="cannot be combined"):
            radius_graph(pos, 0.1, cell=R.T.tolist(), **kw)
    with pytest.raises(ValueError):
        radius_graph(pos, 0.1, cell=R.T.tolist(), origin=[0, 0])
    with pytest.raises(ValueError):
        radius_graph(pos, 0.1, [0, 0, 0], [1, 1, 1], origin=[0, 0, 0])  # an origin without a cell
    with pytest.raises(RuntimeError, match="ROCm"):
        radius_graph(pos, 0.1, cell=R.T.tolist())  # a valid cell: only then the CPU tensor is refused


def test_c_entries_reject_a_bad_cell_before_any_launch():
    import ctypes

    from scalable_e3_gnn_amd import _lib
    from scalable_e3_gnn_amd.radius_graph import grid_params
    lib = _lib.load()
    c9, o3, hgt, _ = cell_params(R.T.tolist())
    cell, origin = _lib.Float9(*c9), _lib.Float3(*o3)
    flat = _lib.Float9(1, 0, 0, 2, 0, 0, 0, 0, 1)
    INVALID = 1
    assert lib.e3_edge_geometry_cell(None, None, None, 5, flat, None, None, None, None) == INVALID
    assert lib.e3_edge_geometry_backward_cell(None, None, None, 5, 1, flat, None, None, None, None, None) == INVALID
    assert lib.e3_msg_forward_cell(None, None, 0, 5, None, None, None, 0, None, None, None, None, 0, 0, 0, 0, flat,
                                   None) == INVALID
    p = grid_params([0.0, 0.0, 0.0], hgt, 0.1)
    args = (None, 5, ctypes.byref(p), cell, origin, None, None, None, None, 0, None)
    big = grid_params([0.0, 0.0, 0.0], hgt, 0.4)  # 2 r >= h_min
    assert lib.e3_rg_sort_count_cell(None, 5, ctypes.byref(big), cell, origin, None, None, None, None, 0, None) == INVALID
    other = grid_params([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], 0.1)  # a grid that is not the one of the heights
    assert lib.e3_rg_sort_count_cell(None, 5, ctypes.byref(other), cell, origin, None, None, None, None, 0, None) == INVALID
    assert lib.e3_rg_sort_count_cell(*args) == INVALID  # a valid cell and grid: the NULL buffers are what is refused
    assert lib.e3_rg_sort_count_cell(None, 0, ctypes.byref(p), flat, origin, None, None, None, None, 0, None) == INVALID


def _cloud(n, seed, cell, origin=(0, 0, 0), spread=1.0):
    s = np.random.default_rng(seed).random((n, 3)) * spread - (spread - 1) / 2
    return (s @ np.asarray(cell, np.float64) + np.asarray(origin, np.float64)).astype(np.float32)


@pytest.mark.parametrize("case", ["T", "T_prime", "skewed_unwrapped_origin"])
def test_reference_graph_vs_fp64_brute_force(case):
    """The restatement's edge set equals the fp64 search over the 27 images; pairs within 1e-6 of the cutoff are left
    out of the comparison and their share is capped at 1e-3 of the pairs.

    Sizes: 3000 to 5000 points at r = 0.06 to 0.07, not the 20 000 points at r = 0.04 quoted in the issue: the search
    is 27 n^2 fp64 distances, seconds at n = 5000 and minutes at 20 000.  The expected tie share does not depend on n: it
    is the volume of the shell |d| in [r - 1e-6, r + 1e-6] over the ball's, 3 * 2e-6 / r = 1e-4 at r = 0.06 (1.5e-4 at
    0.04), so the 1e-3 cap has the same room at either size; the 1 M-point GPU test covers the large cloud."""
    if case == "T":
        cell, origin, n, r, spread = R.T, (0, 0, 0), 5000, 0.06, 1.0
    elif case == "T_prime":
        cell, origin, n, r, spread = R.TP, (0, 0, 0), 3000, 0.07, 1.0
    else:
        cell, origin, n, r, spread = np.array([[1, 0, 0], [0.3, 0.9, 0], [0.2, -0.25, 0.8]]), (0.3, -0.2, 0.1), 3000, 0.07, 3.0
    pos = _cloud(n, 3, cell, origin, spread)
    perm, pos4, rowptr, src = R.graph_cell(pos, cell, r, origin)
    assert sorted(perm.tolist()) == list(range(n))
    w = pos4[:, :3]
    cell32 = np.asarray(cell, np.float32).astype(np.float64)
    s = (w.astype(np.float64) - np.asarray(origin, np.float32).astype(np.float64)) @ np.linalg.inv(cell32)
    assert s.min() > -1e-6 and s.max() < 1 + 1e-6  # wrapped into the cell
    # every point moved by a whole number of lattice vectors
    k = (w.astype(np.float64) - pos[perm].astype(np.float64)) @ np.linalg.inv(cell32)
    assert np.abs(k - np.rint(k)).max() < 1e-5
    dst = np.repeat(np.arange(n), np.diff(rowptr))
    ours = dst.astype(np.int64) * n + src
    assert np.all(np.diff(ours) > 0)  # CSR by dst, ascending src
    inside, ties = R.brute_pairs64(w, cell32, r)
    assert len(ties) <= 1e-3 * len(inside), (len(ties), len(inside))
    assert np.array_equal(np.setdiff1d(ours, ties), np.setdiff1d(inside, ties))
    assert len(inside) > 1000


def test_min_image64_and_tile27():
    rng = np.random.default_rng(5)
    d = rng.standard_normal((1000, 3)) * 2
    m = R.min_image64_cell(d, R.T)
    s = m @ np.linalg.inv(R.T)
    assert np.abs(s).max() <= 0.5 + 1e-12
    k = (d - m) @ np.linalg.inv(R.T)
    assert np.abs(k - np.rint(k)).max() < 1e-12
    tiled, centre = R.tile27(rng.random((7, 3)), R.T)
    assert tiled.shape == (27 * 7, 3) and centre == 13
    assert np.allclose(tiled[:7] - tiled[13 * 7:14 * 7], -(R.T[0] + R.T[1] + R.T[2]))
    # T' spans the lattice of T, and the rotation is proper
    assert abs(np.linalg.det(R.M) - 1) < 1e-12
    Q = R.rotation()
    assert np.allclose(Q @ Q.T, np.eye(3)) and abs(np.linalg.det(Q) - 1) < 1e-12

"""The Verlet list without a device: the numpy restatement of e3_nl_update* (tests/neighbor_list_reference.py) against a
brute-force fp64 all-pairs graph, the threshold arithmetic, and the ValueError paths of NeighborList that need no device."""
import numpy as np
import pytest

import neighbor_list_reference as NR
import pbc_reference as PR
import triclinic_reference as TR
from scalable_e3_gnn_amd import NeighborList
from scalable_e3_gnn_amd.neighbor_list import MAX_COORD_OVER_SKIN, verlet_threshold

f32 = np.float32
R, SKIN, N = 0.2, 0.05, 120
LO, HI = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]


def _moved(pos, rng, periods):
    """Every particle displaced by less than skin / 2 (0.05 .. 0.45 skin, random directions), a third of them also moved
    by (-2..2) whole periods / lattice vectors (``periods`` [3,3], None in an open box)."""
    u = rng.standard_normal(pos.shape)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    new = pos.astype(np.float64) + u * rng.uniform(0.05, 0.45, (len(pos), 1)) * SKIN
    if periods is not None:
        k = rng.integers(-2, 3, size=pos.shape) * (rng.random((len(pos), 1)) < 1 / 3)
        new = new + k @ np.asarray(periods, np.float64)
    return new.astype(f32)


def _case(mode, seed):
    """-> stored graph (perm, pos4, rowptr, src) at R + SKIN, build positions, moved positions, box, cell"""
    rng = np.random.default_rng(seed)
    if mode == "cell":
        pos = (rng.random((N, 3)) @ TR.T).astype(f32)
        stored = TR.graph_cell(pos, TR.T, R + SKIN)
        return stored, pos, _moved(pos, rng, TR.T), None, TR.T.astype(f32)
    pos = rng.random((N, 3)).astype(f32)
    periodic = mode == "box"
    stored = PR.graph_pbc(pos, LO, HI, R + SKIN, periodic)
    box = PR.box_lengths(LO, HI, True) if periodic else None
    return stored, pos, _moved(pos, rng, np.eye(3) if periodic else None), box, None


@pytest.mark.parametrize("mode,seed", [("open", 1), ("box", 2), ("cell", 3)])
def test_restatement_vs_fp64_all_pairs(mode, seed):
    (perm, ref4, rowptr, src), pos, new, box, cell = _case(mode, seed)
    # conditions on the inputs: no pair sits on either cutoff, where fp32 and fp64 may disagree
    d_new, d_old = NR.pair_distances64(new, box, cell), NR.pair_distances64(pos, box, cell)
    assert not (np.abs(d_new - R) < 1e-5 * R).any()
    assert not (np.abs(d_old - (R + SKIN)) < 1e-5 * R).any()
    pos4, rowptr_r, src_r, dst_r, stats = NR.update(new, perm, ref4, rowptr, src, R, box, cell)
    assert np.array_equal(pos4[:, :3], new[perm]) and not pos4[:, 3].any()
    # the displacements are below skin / 2 whatever whole periods were added, and the list says so
    assert 0.0 < NR.max_d2(stats) < float(NR.threshold(SKIN))
    assert np.sqrt(NR.max_d2(stats)) < 0.46 * SKIN
    got = NR.pairs_of(perm, dst_r, src_r)
    want = NR.pairs_within64(d_new, R)
    assert len(want) > 2 * N and np.array_equal(got, want)
    assert len(src_r) < len(src) and stats[1] == len(src_r) == rowptr_r[-1]
    # CSR in the stored order, ascending inside each row
    for i in (0, 1, N // 2, N - 1):
        row = src_r[rowptr_r[i]:rowptr_r[i + 1]]
        assert np.all(np.diff(row) > 0) and np.all(dst_r[rowptr_r[i]:rowptr_r[i + 1]] == i)
    # the stored graph itself is the fp64 graph at R + SKIN, and a particle moved past skin / 2 is seen
    assert np.array_equal(NR.pairs_of(perm, np.repeat(np.arange(N), np.diff(rowptr)), src),
                          NR.pairs_within64(d_old, R + SKIN))
    far = new.copy()
    far[7] = pos[7] + np.array([0.55 * SKIN, 0, 0], f32)
    assert not NR.max_d2(NR.update(far, perm, ref4, rowptr, src, R, box, cell)[4]) < float(NR.threshold(SKIN))


def test_restatement_edge_cases():
    (perm, ref4, rowptr, src), pos, new, box, cell = _case("box", 2)
    bad = new.copy()
    bad[5, 1] = np.nan
    stats = NR.update(bad, perm, ref4, rowptr, src, R, box, cell)[4]
    assert stats[0] > 0x7f800000 and not NR.max_d2(stats) < float(NR.threshold(SKIN))
    p4, rp, s, d, st = NR.update(np.zeros((0, 3), f32), [], np.zeros((0, 4), f32), [0], [], R)
    assert p4.shape == (0, 4) and rp.tolist() == [0] and len(s) == len(d) == 0 and st.tolist() == [0, 0]
    # unchanged positions in an open box: the builder's own test, edge for edge
    (perm, ref4, rowptr, src), pos, _, _, _ = _case("open", 1)
    _, rp, s, _, st = NR.update(pos, perm, ref4, rowptr, src, R + SKIN)
    assert np.array_equal(rp, rowptr) and np.array_equal(s, src) and st[0] == 0


def test_threshold_arithmetic():
    for skin in (0.05, 0.3, 1.0, 1e-3, 7.25):
        thr = verlet_threshold(skin)
        assert thr == float(NR.threshold(skin)) and f32(thr) == thr
        half = 0.5 * float(f32(skin))
        # below (skin / 2)^2 by the 2^-10 margin (twice, squared), to fp32 rounding
        assert thr < half * half
        assert abs(thr / (half * half) - (1 - 2.0 ** -10) ** 2) < 2.0 ** -22
    assert MAX_COORD_OVER_SKIN == 256.0
    # the budget of DESIGN.md 4.4b: 64 roundings of half an ulp of the largest admitted coordinate fit into skin 2^-10
    assert 64 * 2.0 ** -24 * MAX_COORD_OVER_SKIN <= 2.0 ** -10


def test_value_errors_without_a_device():
    box = dict(lo=LO, hi=HI, periodic=True)
    for kw in (dict(r=R, skin=0.0), dict(r=R, skin=-0.1), dict(r=R, skin=float("nan")), dict(r=0.0, skin=SKIN),
               dict(r=-1.0, skin=SKIN), dict(r=float("inf"), skin=SKIN)):
        with pytest.raises(ValueError):
            NeighborList(**kw, **box)
    batch = np.zeros(4, np.int64)  # never touched: the combination is refused first
    for kw in (box, dict(lo=LO, hi=HI), dict(cell=TR.T.tolist())):
        with pytest.raises(ValueError):
            NeighborList(R, SKIN, batch=batch, **kw)
    for kw in (dict(lo=LO), dict(hi=HI), dict(periodic=True), dict(lo=LO, hi=HI, periodic=True)):
        with pytest.raises(ValueError, match="cell= describes the whole periodic cell"):
            NeighborList(R, SKIN, cell=TR.T.tolist(), **kw)
    with pytest.raises(ValueError, match="needs cell="):
        NeighborList(R, SKIN, origin=[0, 0, 0])
    with pytest.raises(ValueError):  # periodic without a box
        NeighborList(R, SKIN, periodic=True)
    with pytest.raises(ValueError):  # the builder's check at r + skin: 2 (0.45 + 0.05) >= 1
        NeighborList(0.45, SKIN, **box)
    with pytest.raises(ValueError):  # the same for the heights of the cell
        NeighborList(0.45, SKIN, cell=TR.T.tolist())
    with pytest.raises(ValueError):
        NeighborList(R, SKIN, cell=[[1, 0, 0], [2, 0, 0], [0, 0, 1]])  # singular
    nl = NeighborList(R, SKIN, **box)
    assert (nl.builds, nl.updates, nl.rebuilt) == (0, 0, False) and nl.r == R and nl.skin == SKIN
    with pytest.raises(ValueError):
        nl.set_box(lo=LO, hi=[0.4, 1, 1])  # 2 (r + skin) >= L
    with pytest.raises(ValueError):
        nl.set_box(lo=LO, hi=HI, cell=TR.T.tolist())
    nl.set_box(lo=LO, hi=[2, 2, 2])
    # a list keeps its kind: a box does not become a cell, nor a cell a box (which would silently be an open one)
    with pytest.raises(ValueError, match="made with lo / hi"):
        nl.set_box(cell=TR.T.tolist())
    with pytest.raises(ValueError, match="made with lo / hi"):
        nl.set_box(lo=LO, hi=HI, origin=[0, 0, 0])
    assert nl._box["hi"] == [2, 2, 2] and nl._box["periodic"] is True  # a refused call leaves the list as it was
    nc = NeighborList(R, SKIN, cell=TR.T.tolist())
    for kw in (dict(lo=LO, hi=HI), dict(), dict(origin=[0, 0, 0])):
        with pytest.raises(ValueError, match="made with cell="):
            nc.set_box(**kw)
    nc.set_box(cell=(1.5 * TR.T).tolist(), origin=[0.1, 0, 0])
    assert nc._box["periodic"] is False and nc._box["origin"] == [0.1, 0, 0]
    nl.invalidate()

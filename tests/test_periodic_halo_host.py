"""Periodic spatial sharding on the host (no GPU): the ghost-image entry table of ``GridHalo(..., periodic=)``, its argument
checks, and gloo runs at world 1, 2, 4 and 8 in which every rank runs the numpy oracle on its local OPEN graph over
``[wrapped owned | ghost images]``.  The merged owned outputs must equal the fp64 oracle of the whole cloud tiled by its
periodic images, and the local edge sets (ghosts mapped back to global ids through a feature column) must equal
``radius_graph(periodic=True)``'s restatement (tests/pbc_reference.py) exactly.  Coordinates are dyadic (2^-16 grid, box
length 1), so every image shift is exact in fp32."""
import itertools

import numpy as np
import pytest
import torch

import gloo_ranks
import models  # noqa: F401  (registers scalable_e3_gnn_amd -- also in the spawned ranks, which import this module)
import pbc_reference as P
from scalable_e3_gnn_amd.sharding import GridHalo, check_cutoff, image_entries

OFFS = list(itertools.product((-1, 0, 1), repeat=3))
MASKS = [True, False, (True, False, True), (False, True, False)]


def _coords(rank, dims):
    px, py, pz = dims
    return rank // (py * pz), (rank // pz) % py, rank % pz


def _rank(c, dims):
    return (c[0] * dims[1] + c[1]) * dims[2] + c[2]


def _open_neighbours(rank, dims):
    """The open-box neighbour set as GridHalo has always computed it."""
    me = _coords(rank, dims)
    nb = set()
    for d in OFFS:
        c = [me[a] + d[a] for a in range(3)]
        if d != (0, 0, 0) and all(0 <= c[a] < dims[a] for a in range(3)):
            nb.add(_rank(c, dims))
    return sorted(nb)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the entry table
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 1, 1), (3, 1, 1), (2, 2, 2), (2, 2, 1)])
@pytest.mark.parametrize("periodic", MASKS)
def test_entry_table(dims, periodic):
    lo, hi = [0.0, -1.0, 0.5], [1.0, 1.0, 2.0]
    L = [1.0, 2.0, 1.5]
    ax = P.axes_of(periodic)
    world = dims[0] * dims[1] * dims[2]
    tables = {p: image_entries(dims, lo, hi, periodic, p) for p in range(world)}
    for p, ent in tables.items():
        me = _coords(p, dims)
        # entry count: 3 offsets per periodic axis, the in-range ones per open axis, minus d = 0
        n_axis = [3 if ax[a] else 1 + (me[a] > 0) + (me[a] < dims[a] - 1) for a in range(3)]
        assert len(ent) == n_axis[0] * n_axis[1] * n_axis[2] - 1
        assert [d for _, d, _ in ent] == [d for d in OFFS if d in {d for _, d, _ in ent}]   # OFFSETS order
        assert len({d for _, d, _ in ent}) == len(ent)
        for q, d, t in ent:
            c = _coords(q, dims)
            for a in range(3):
                # peer box + t is the box next to mine at offset d
                assert c[a] * L[a] / dims[a] + t[a] == pytest.approx((me[a] + d[a]) * L[a] / dims[a])
                assert t[a] in (0.0, L[a], -L[a]) and (t[a] == 0.0 or ax[a])
            # the partner entry on q, with the opposite translation
            back = [(qq, dd, tt) for qq, dd, tt in tables[q] if qq == p and dd == tuple(-v for v in d)]
            assert len(back) == 1 and back[0][2] == tuple(-v if v else 0.0 for v in t)
            # a self entry exactly when every nonzero component of d lies on a periodic axis with one box
            assert (q == p) == all(d[a] == 0 or (ax[a] and dims[a] == 1) for a in range(3))
        if not any(ax):
            assert [q for q, _, _ in ent] == _open_neighbours(p, dims)
            assert all(t == (0.0, 0.0, 0.0) for _, _, t in ent)
    if world == 1:
        h = GridHalo(dims, lo, hi, periodic=periodic)       # no process group at world 1
        assert h.images == tables[0] and h.neighbours == []


def test_open_mode_attributes_unchanged():
    h = GridHalo((1, 1, 1), (0, 0, 0), (1, 1, 1))
    assert h.periodic == 0 and h.neighbours == [] and h.images == []
    pos = torch.rand(50, 3, dtype=torch.float64)
    lp, lx = h.setup(pos, pos.clone(), 0.1)
    assert torch.equal(lp, pos) and h.n_ghost == 0 and h.send_counts == []


# ---------------------------------------------------------------------------------------------------------------------
# 2. argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_value_errors():
    with pytest.raises(ValueError):
        GridHalo((1, 1, 1), (0, 0, 0), (1, 1, 1), periodic=(True, False))            # wrong length
    with pytest.raises(ValueError):
        GridHalo((1, 1, 1), (0, 0, 0), (1, 1, 1), periodic=(True, True, True, True))
    h = GridHalo((1, 1, 1), (0, 0, 0), (1, 1, 1), periodic=True)
    pos = torch.rand(20, 3)
    for r in (0.5, 0.7):                                                              # 2 r >= L
        with pytest.raises(ValueError):
            h.setup(pos, pos.clone(), r)
    h.setup(pos, pos.clone(), 0.49)
    with pytest.raises(ValueError):
        GridHalo((1, 1, 1), (0, 0, 0), (1, 2, 1), periodic=(False, False, True)).setup(pos, pos.clone(), 0.5)
    # r above the box width of an axis with more than one box (the grid of a 4-rank run, checked without one)
    with pytest.raises(ValueError):
        check_cutoff((4, 1, 1), (0, 0, 0), (4, 8, 8), True, 1.5)
    check_cutoff((4, 1, 1), (0, 0, 0), (4, 8, 8), True, 1.0)
    with pytest.raises(ValueError):
        check_cutoff((1, 1, 1), (0, 0, 0), (4, 8, 8), (False, True, False), 4.0)   # periodic y: 2 r = 8 = L
    check_cutoff((1, 1, 1), (0, 0, 0), (4, 8, 8), (False, True, False), 3.9)


def test_world1_self_halo_without_a_process_group():
    """dims (1,1,1), all periodic: every entry is a self entry; the local open graph equals the periodic graph."""
    from oracle import graph_oracle as G
    N, r = 1500, 0.1
    pos = _dyadic(N, 3)
    pos[:40] += np.float32(1.0)
    pos[40:80] -= np.float32(3.0)
    h = GridHalo((1, 1, 1), (0, 0, 0), (1, 1, 1), periodic=True)
    ids = torch.arange(N, dtype=torch.float64)[:, None]
    lp, lx = h.setup(torch.as_tensor(pos), ids, r)
    assert len(h.images) == 26 and len(h.send_counts) == 26 and h.send_counts == [h.recv_counts[25 - e] for e in range(26)]
    assert np.array_equal(lp[:N].numpy(), P.wrap(pos, [0] * 3, [1] * 3, True))
    perm, rowptr, src = G.graph(lp.numpy(), [-2 * r] * 3, [1 + 2 * r] * 3, r)
    h.renumber(torch.as_tensor(perm))
    assert _owned_edges(h, perm, rowptr, src, lx[:, 0].numpy()) == _ref_edges(pos, r, True, np.arange(N))


# ---------------------------------------------------------------------------------------------------------------------
# 3. gloo runs
# ---------------------------------------------------------------------------------------------------------------------
def _dyadic(n, seed):
    return (np.random.default_rng(seed).integers(0, 1 << 16, size=(n, 3)) / float(1 << 16)).astype(np.float32)


def _cloud(N, kind, seed):
    pos = _dyadic(N, seed)
    if kind == "outside":   # whole and fractional periods on the periodic axes: wrapped by setup
        k = np.random.default_rng(seed + 1).integers(-2, 3, size=pos.shape).astype(np.float32)
        pos = (pos + k).astype(np.float32)
    elif kind == "empty":   # nothing in x >= 1/2, y >= 1/2: rank 3 of a (2, 2, 1) grid owns nothing
        hole = (pos[:, 0] >= 0.5) & (pos[:, 1] >= 0.5)
        pos[hole, 0] -= np.float32(0.5)
    x = np.random.default_rng(seed + 2).standard_normal((N, 4))
    return pos, x


def _owned_edges(halo, perm, rowptr, src, gid_col):
    """Edges (dst, src) of the local graph into owned rows, in global ids (ghosts carry their owner's id)."""
    gid = np.asarray(gid_col).astype(np.int64)[perm]
    dst = np.repeat(np.arange(len(perm)), np.diff(rowptr))
    keep = ~halo.is_ghost.numpy()[dst]
    e = np.stack([gid[dst[keep]], gid[src[keep]]], 1)
    return set(map(tuple, e.tolist()))


def _ref_edges(pos, r, periodic, rows):
    perm, _, rowptr, src = P.graph_pbc(pos, [0] * 3, [1] * 3, r, periodic)
    dst = perm[np.repeat(np.arange(len(perm)), np.diff(rowptr))].astype(np.int64)
    s = perm[src].astype(np.int64)
    m = np.isin(dst, rows)
    return set(map(tuple, np.stack([dst[m], s[m]], 1).tolist()))


def _worker(rank, world, dims, periodic, N, H, layers, kind, q):
    import torch.distributed as dist
    import models  # noqa: F401
    from oracle import graph_oracle as G
    from oracle import segnn_oracle as S
    from scalable_e3_gnn_amd.radius_graph import RadiusGraph
    from scalable_e3_gnn_amd.segnn import SEGNN

    pos, x = _cloud(N, kind, 5)
    r = 1.0 / (layers + 2.2)
    torch.manual_seed(0)
    params = {k: v.detach().double().numpy() for k, v in SEGNN("1x0e+1x1o", H, "1x1o", layers).state_dict().items()}
    halo = GridHalo(dims, (0, 0, 0), (1, 1, 1), periodic=periodic)
    own = (halo.owner_of(torch.as_tensor(pos)) == rank).nonzero().flatten().numpy()
    feats = torch.as_tensor(np.concatenate([x[own], own[:, None].astype(np.float64)], 1))   # last column: global id
    lpos, lf = halo.setup(torch.as_tensor(pos[own]), feats, r)
    assert lpos.dtype == torch.float32 and len(halo.send_counts) == len(halo.images) == len(halo.recv_counts)
    blo, bhi = halo.box(rank)
    nloc = lpos.shape[0]
    if nloc:
        perm, rowptr, src = G.graph(lpos.numpy(), [v - 2 * r for v in blo], [v + 2 * r for v in bhi], r)
    else:
        perm, rowptr, src = np.zeros(0, np.int32), np.zeros(1, np.int32), np.zeros(0, np.int32)
    halo.renumber(torch.as_tensor(perm))
    edges = _owned_edges(halo, perm, rowptr, src, lf[:, 4].numpy())
    g = RadiusGraph(torch.as_tensor(perm), torch.zeros(nloc, 4), torch.as_tensor(rowptr), torch.as_tensor(src),
                    len(src), ((1, 1, 1), 0))
    sp = halo.split_graph(g)

    def exchange(h):
        t = torch.as_tensor(h)
        return halo.finish(t, halo.start(t)).numpy()

    if len(own):
        out = S.forward(params, H, layers, "1x0e+1x1o", "1x1o", lf[:, :4].numpy()[perm],
                        lpos.numpy().astype(np.float64)[perm], sp.graph.rowptr.numpy(), sp.graph.src.numpy(),
                        exchange=exchange)
        owned_out = out[halo.owned_new.numpy()]
    else:
        for _ in range(layers):
            exchange(np.zeros((nloc, 4 * H)))   # an empty rank still takes part in every refresh
        owned_out = np.zeros((0, 3))
    q.put((rank, own, owned_out, sorted(edges), halo.n_ghost, len(halo.neighbours)))
    dist.barrier()


def _tiled_oracle(pos, x, r, periodic, H, layers):
    """fp64 oracle of the whole periodic cloud: the centre copy of the cloud tiled by its images on the periodic axes."""
    from oracle import graph_oracle as G
    from oracle import segnn_oracle as S
    ax = P.axes_of(periodic)
    w = P.wrap(pos, [0] * 3, [1] * 3, periodic).astype(np.float64)
    offs = [o for o in OFFS if all(o[a] == 0 or ax[a] for a in range(3))]
    tiled = np.concatenate([w + np.asarray(o, np.float64) for o in offs], 0).astype(np.float32)
    c, N = offs.index((0, 0, 0)), len(pos)
    perm, rowptr, src = G.graph(tiled, [-1.0] * 3, [2.0] * 3, r)
    torch.manual_seed(0)
    from scalable_e3_gnn_amd.segnn import SEGNN
    params = {k: v.detach().double().numpy() for k, v in SEGNN("1x0e+1x1o", H, "1x1o", layers).state_dict().items()}
    out = S.forward(params, H, layers, "1x0e+1x1o", "1x1o", np.tile(x, (len(offs), 1))[perm], tiled[perm].astype(np.float64),
                    rowptr, src)
    back = np.empty_like(out)
    back[perm] = out
    return back[c * N:(c + 1) * N]


def _run(dims, periodic, N, kind, H=4, layers=2):
    world = dims[0] * dims[1] * dims[2]
    got = gloo_ranks.run(_worker, world, (dims, periodic, N, H, layers, kind), world, 280)
    pos, x = _cloud(N, kind, 5)
    r = 1.0 / (layers + 2.2)
    want = _tiled_oracle(pos, x, r, periodic, H, layers)
    merged = np.full_like(want, np.nan)
    for rank, own, out, edges, _, _ in got:
        merged[own] = out
        assert set(edges) == _ref_edges(pos, r, periodic, own), f"rank {rank}: local edge set differs"
    assert not np.isnan(merged).any(), "every particle must be owned by exactly one rank"
    err = np.abs(merged - want).max() / np.abs(want).max()
    assert err < 1e-10, err
    return {g[0]: g for g in got}


@pytest.mark.timeout(300)
def test_gloo_world1_self_halo():
    got = _run((1, 1, 1), True, 300, "uniform")
    assert got[0][4] > 0 and got[0][5] == 0                    # ghosts, all from itself


@pytest.mark.timeout(300)
def test_gloo_world2_peer_on_both_faces_positions_outside():
    got = _run((2, 1, 1), True, 300, "outside")
    assert all(g[5] == 1 for g in got.values())                # one distinct peer, reached through several entries


@pytest.mark.timeout(300)
def test_gloo_world4_empty_rank():
    got = _run((2, 2, 1), True, 320, "empty")
    assert len(got[3][1]) == 0 and got[3][4] > 0               # rank 3 owns nothing but still holds ghost images


@pytest.mark.timeout(300)
def test_gloo_world4_mixed_periodicity():
    _run((2, 2, 1), (True, False, True), 320, "uniform")


@pytest.mark.timeout(420)
def test_gloo_world8_octants():
    got = _run((2, 2, 2), True, 400, "uniform")
    assert all(g[5] == 7 for g in got.values())

"""The host side of the sharded Verlet list, on CPU tensors (no GPU): ``nl_update_split_torch`` against the numpy
restatement (tests/sharded_list_reference.py), exactly; ``Halo.update_positions`` at world 1 on a periodic self-halo and at
world 2 over gloo against a fresh ``setup``; the two-rank collective decision of ``ShardedNeighborList`` (a brute-force host
builder stands in for ``radius_graph``, which has no CPU path)."""
import numpy as np
import pytest
import torch

import gloo_ranks
import models  # noqa: F401  (registers scalable_e3_gnn_amd -- also in the spawned ranks, which import this module)
import sharded_list_reference as SR
from scalable_e3_gnn_amd import OwnershipChanged, ShardedNeighborList
from scalable_e3_gnn_amd.radius_graph import RadiusGraph
from scalable_e3_gnn_amd.sharded_list import nl_update_split_torch
from scalable_e3_gnn_amd.sharding import GridHalo

f32 = np.float32
R, SKIN = 0.2, 0.05
LO, HI = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]


def _brute_graph(lpos, r, lo=None, hi=None):
    """The radius graph of a small cloud by all pairs, renumbered by a sort along x -> RadiusGraph (CPU tensors)."""
    p = lpos.detach().cpu().numpy().astype(f32)
    perm = np.argsort(p[:, 0], kind="stable").astype(np.int32)
    q = p[perm]
    d = q[None, :, :] - q[:, None, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    adj = d2 <= f32(f32(r) * f32(r))
    np.fill_diagonal(adj, False)
    dst, src = np.nonzero(adj)                                  # row-major: rows ascending, src ascending inside a row
    rowptr = np.concatenate([[0], np.cumsum(adj.sum(1))]).astype(np.int32)
    pos4 = np.concatenate([q, np.zeros((len(q), 1), f32)], 1)
    return RadiusGraph(torch.as_tensor(perm), torch.as_tensor(pos4), torch.as_tensor(rowptr),
                       torch.as_tensor(src.astype(np.int32)), int(len(src)), ((1, 1, 1), 0))


def _dyadic(n, seed, bits=10):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 1 << bits, size=(n, 3)) / float(1 << bits)).astype(f32), rng


# ---------------------------------------------------------------------------------------------------------------------
# 1: the CPU twin of the entry against the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ghosts", ["none", "all", "some"])
def test_torch_twin_equals_the_restatement(ghosts):
    rng = np.random.default_rng(3)
    pos = rng.random((150, 3)).astype(f32)
    g = _brute_graph(torch.as_tensor(pos), R + SKIN)             # edges into ghost rows included
    u = rng.standard_normal(pos.shape)
    new = (pos + 0.4 * SKIN * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(f32)
    ghost = {"none": np.zeros(150, bool), "all": np.ones(150, bool), "some": rng.random(150) < 0.3}[ghosts]
    want = SR.update_split(new, g.perm.numpy(), g.pos4.numpy(), g.rowptr.numpy(), g.src.numpy(), ghost, R)
    got = nl_update_split_torch(torch.as_tensor(new), g.perm, g.pos4, g.rowptr, g.src, torch.as_tensor(ghost).to(torch.uint8), R)
    assert np.array_equal(got[0].numpy().view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(got[1].numpy(), want[1])
    for (gs, gd), (ws, wd) in ((got[2:4], want[2]), (got[4], want[3]), (got[5], want[4])):
        assert gs.dtype == torch.int32 and np.array_equal(gs.numpy(), ws) and np.array_equal(gd.numpy(), wd)
    assert got[6].tolist() == [int(v) for v in want[5]]
    ek, ei, eb = (int(v) for v in want[5][1:])
    assert ek == ei + eb and ek < g.num_edges
    if ghosts == "some":
        assert ei > 0 and eb > 0
    if ghosts == "all":
        assert ek == 0 and want[5][0] > 0


# ---------------------------------------------------------------------------------------------------------------------
# 2: update_positions at world 1, periodic self-halo
# ---------------------------------------------------------------------------------------------------------------------
def test_update_positions_world1_periodic_self_halo():
    pos, rng = _dyadic(120, 5)
    pos[0] = [0.5, 0.03125, 0.96875]                             # near two faces: sent for several entries
    pos[1] = [0.984375, 0.5, 0.5]                                # will cross the +x face
    x = torch.arange(120, dtype=torch.float32)[:, None].repeat(1, 2)
    halo = GridHalo((1, 1, 1), LO, HI, periodic=True)
    gen = halo.generation
    lpos0, _ = halo.setup(torch.as_tensor(pos), x, R + SKIN)
    assert halo.generation == gen + 1
    n = 120
    assert torch.equal(lpos0[:n], torch.as_tensor(pos))          # inside the box: the wrap is the identity
    new = pos.copy()
    new[0] += np.array([2.0, -1.0, 0.0], f32) + f32(2.0 ** -8)   # whole periods plus a small dyadic move
    new[1, 0] += f32(2.0 ** -5)                                  # 0.984375 -> 1.015625: across the face
    new[2:] += (rng.integers(-4, 5, size=(n - 2, 3)) * 2.0 ** -10).astype(f32)
    lpos, lx = halo.update_positions(torch.as_tensor(new), x)
    assert halo.generation == gen + 1                            # no setup
    owned = lpos[:n].numpy()
    # the restatement, exactly; and for these dyadic inputs the exact continuation
    assert np.array_equal(owned, SR.continued(new, pos, pos, LO, HI, 7))
    want = pos.astype(np.float64)
    want[0] += 2.0 ** -8
    want[1, 0] += 2.0 ** -5
    want[2:] += new[2:].astype(np.float64) - pos[2:].astype(np.float64)
    assert np.array_equal(owned.astype(np.float64), want)
    assert owned[1, 0] == f32(1.015625)                          # continued, not re-wrapped: nothing jumps
    assert np.array_equal(halo.displacement(torch.as_tensor(new)).numpy(), SR.displacement(new, pos, LO, HI, 7))
    # ghosts: the owner's local position plus the entry's shift, exactly; features unshifted
    sel = halo.sel.numpy()
    shift = np.concatenate([np.tile(np.array([-v for v in halo.images[m][2]], f32), (halo.send_counts[m], 1))
                            for m in range(len(halo.images))])
    # self entry e receives what is sent for entry m = (me, -d): the received order is the send order permuted by entry
    recv = np.concatenate([np.arange(sum(halo.send_counts[:m]), sum(halo.send_counts[:m + 1]))
                           for e, m in sorted(halo._self_pairs)]).astype(np.int64)
    assert len(recv) == halo.n_ghost and (shift != 0).any()
    assert np.array_equal(lpos[n:].numpy(), (owned[sel] + shift)[recv])
    assert np.array_equal(lx[n:].numpy(), x.numpy()[sel][recv]) and torch.equal(lx[:n], x)
    assert int((sel == 0).sum()) >= 3                            # particle 0 has several images, each moved with it


# ---------------------------------------------------------------------------------------------------------------------
# 3: update_positions at world 2 (gloo, CPU tensors) against a fresh setup
# ---------------------------------------------------------------------------------------------------------------------
def _report(rank, q, fn, n_items, *args):
    """Run ``fn``; a failure is reported on the queue at once (as many items as the rank owes)."""
    import traceback
    try:
        fn(rank, q, *args)
    except Exception:
        for _ in range(n_items):
            q.put(("error", rank, traceback.format_exc()))


def _cloud2(seed):
    """Dyadic points on the 1/64 lattice shifted by 1/128: never on a box face, and +-1/256 moves keep them in their box."""
    rng = np.random.default_rng(seed)
    pos = ((rng.integers(0, 64, size=(260, 3)) + 0.5) / 64.0).astype(f32)
    move = (rng.integers(-2, 3, size=pos.shape) / 512.0).astype(f32)
    return pos, move, rng


def _positions_body(rank, q, periodic):
    import torch.distributed as dist
    pos, move, rng = _cloud2(11)
    gid = torch.arange(len(pos), dtype=torch.float32)[:, None]
    halo = GridHalo((2, 1, 1), LO, HI, periodic=periodic)
    own = (halo.owner_of(torch.as_tensor(pos)) == rank).nonzero().flatten()
    p0, x = torch.as_tensor(pos)[own], gid[own]
    halo.setup(p0, x, R + SKIN)
    p1 = p0 + torch.as_tensor(move)[own]
    if periodic:
        p1[::3] += torch.tensor([1.0, -2.0, 0.0])                # a caller that lets a third of them run unwrapped
    assert bool((halo.owner_of(p1) == rank).all())
    lpos, lx = halo.update_positions(p1, x)
    n = own.numel()
    assert torch.equal(lx[:n], x) and lx.shape[0] == n + halo.n_ghost
    fresh = GridHalo((2, 1, 1), LO, HI, periodic=periodic)
    fpos, fx = fresh.setup(p1, x, R)
    # ghosts matched by (entry, global id): everything a fresh halo at r holds is held by the stored one at r + skin
    def keyed(h, lp, lf):
        ent = np.repeat(np.arange(len(h.images)), h.recv_counts)
        return {(int(e), int(g)): lp[n + k].numpy() for k, (e, g) in enumerate(zip(ent, lf[n:, 0].tolist()))}
    stored, want = keyed(halo, lpos, lx), keyed(fresh, fpos, fx)
    assert len(want) > 20 and set(want) <= set(stored), (len(want), len(set(want) - set(stored)))
    bad = [k for k, v in want.items() if not np.array_equal(v, stored[k])]
    assert not bad, bad[:5]
    assert torch.equal(lpos[:n], fpos[:n])                        # the owned rows: dyadic, inside the box after the wrap
    q.put(("ok", rank, len(want)))
    dist.barrier()


def _positions_worker(rank, world, periodic, q):
    _report(rank, q, _positions_body, 1, periodic)


@pytest.mark.parametrize("periodic", [False, True])
def test_update_positions_world2_equals_fresh_setup(periodic):
    got = gloo_ranks.run(_positions_worker, 2, (periodic,), 2, 120)
    assert not [g for g in got if g[0] == "error"], "\n".join(g[2] for g in got if g[0] == "error")
    assert sorted(g[1] for g in got) == [0, 1]


# ---------------------------------------------------------------------------------------------------------------------
# 4: the collective decision of the list
# ---------------------------------------------------------------------------------------------------------------------
def _decision_body(rank, q):
    import torch.distributed as dist
    pos, move, rng = _cloud2(21)
    halo = GridHalo((2, 1, 1), LO, HI)
    own = (halo.owner_of(torch.as_tensor(pos)) == rank).nonzero().flatten()
    p, x = torch.as_tensor(pos)[own].clone(), torch.arange(len(pos), dtype=torch.float32)[own, None]
    nl = ShardedNeighborList(R, SKIN, halo, graph_builder=_brute_graph)
    log = []
    cloud = nl.update(p, x)
    log.append((nl.builds, nl.rebuilt))
    n_local = cloud.x.shape[0]
    assert cloud.split.graph.rowptr.numel() == n_local + 1 and cloud.pos.shape == (n_local, 3)
    p = p + torch.as_tensor(move)[own]                            # everybody a little: the list holds
    cloud = nl.update(p, x)
    log.append((nl.builds, nl.rebuilt))
    # the pruned graph is the radius graph at r of the local cloud, with the edges into ghost rows removed
    # (dyadic coordinates: no rounding anywhere)
    lp = cloud.pos.numpy().astype(np.float64)
    near = ((lp[:, None, :] - lp[None, :, :]) ** 2).sum(-1) <= np.float64(f32(R)) ** 2
    np.fill_diagonal(near, False)
    near[halo.is_ghost.numpy()] = False
    g = cloud.split.graph
    got = np.zeros_like(near)
    got[g.dst.numpy(), g.src.numpy()] = True
    assert g.num_edges == int(near.sum()) > n_local and np.array_equal(got, near)
    ghost_src = halo.is_ghost.numpy()[g.src.numpy()]
    assert np.array_equal(cloud.split.boundary[0].numpy(), g.src.numpy()[ghost_src])
    assert np.array_equal(cloud.split.interior[1].numpy(), g.dst.numpy()[~ghost_src]) and ghost_src.any()
    if rank == 1:
        p[0, 1] += 0.75 * SKIN                                    # only a rank-1 particle exceeds skin / 2
    nl.update(p, x)
    log.append((nl.builds, nl.rebuilt))
    nl.update(p, x)
    log.append((nl.builds, nl.rebuilt))
    if rank == 0:
        p[1, 0] = 0.75                                            # a rank-0 particle inside rank 1's box
    try:
        nl.update(p, x)
        log.append("no exception")
    except OwnershipChanged:
        log.append("OwnershipChanged")
    q.put(("ok", rank, log))
    dist.barrier()


def _decision_worker(rank, world, q):
    _report(rank, q, _decision_body, 1)


def test_two_rank_collective_decision():
    got = gloo_ranks.run(_decision_worker, 2, (), 2, 120)
    assert not [g for g in got if g[0] == "error"], "\n".join(g[2] for g in got if g[0] == "error")
    for _, rank, log in got:
        assert log == [(1, True), (1, False), (2, True), (2, False), "OwnershipChanged"], (rank, log)

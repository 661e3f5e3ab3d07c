"""gloo tests (world 2 and 4, CPU tensors) of particle migration: ``Halo.migrate`` on a ``GridHalo`` (open, and periodic with
unwrapped coordinates) and a ``MortonHalo``; the collective refusal of a position that is not finite; the Morton re-balance
(``partition.fit`` + ``migrate``); and ``ShardedNeighborList.redistribute`` carrying a two-rank trajectory through a face
crossing (a brute-force host builder stands in for ``radius_graph``, which has no CPU path)."""
import numpy as np
import pytest
import torch

import gloo_ranks
import models  # noqa: F401  (registers scalable_e3_gnn_amd -- also in the spawned ranks, which import this module)
from test_sharded_list_host import _brute_graph

f32 = np.float32
LO, HI = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
N = 600
R, SKIN = 0.2, 0.05


def _report(rank, q, fn, n_items, *args):
    """Run ``fn``; a failure is reported on the queue at once (as many items as the rank owes)."""
    import traceback
    try:
        fn(rank, q, *args)
    except Exception:
        for _ in range(n_items):
            q.put(("error", rank, traceback.format_exc()))


def _errors(got):
    assert not [g for g in got if g[0] == "error"], "\n".join(g[2] for g in got if g[0] == "error")


# ---------------------------------------------------------------------------------------------------------------------
# 1: Halo.migrate
# ---------------------------------------------------------------------------------------------------------------------
def _dims(world):
    return {2: (2, 1, 1), 4: (2, 2, 1)}[world]


def _cloud(layout, world):
    """The whole cloud before and after the move (the same arrays in every process), its ids' payload, and the width a
    particle may move: one rank-box width."""
    rng = np.random.default_rng({"open": 1, "periodic": 2, "morton": 3}[layout] + 10 * world)
    pos0 = rng.random((N, 3)).astype(f32)
    width = 0.5
    if layout == "morton":
        blob = rng.random(N) < 0.6
        pos0 = np.where(blob[:, None], np.array([0.3, 0.65, 0.6]) + 0.15 * rng.standard_normal((N, 3)), pos0)
        pos0 = np.clip(pos0, 0.0, 1.0 - 2.0 ** -20).astype(f32)
        width = 0.25
    third = rng.random(N) < 1.0 / 3.0
    pos1 = pos0.copy()
    pos1[third] += ((rng.random((int(third.sum()), 3)) * 2 - 1) * width).astype(f32)
    if layout == "periodic":                                     # a caller that lets its coordinates run unwrapped
        hop = rng.random(N) < 0.5
        pos1[hop] += rng.integers(-2, 3, size=(int(hop.sum()), 3)).astype(f32)
    feat = rng.standard_normal((N, 5)).astype(f32)
    return pos0, pos1, feat


def _halo(layout, world, pos0, rank):
    from scalable_e3_gnn_amd.sharding import GridHalo, MortonHalo, MortonPartition
    if layout == "morton":
        # every rank starts from an arbitrary share: the histograms are summed over the group
        return MortonHalo(MortonPartition(LO, HI, 0.1, world).fit(torch.as_tensor(pos0)[rank::world]))
    return GridHalo(_dims(world), LO, HI, periodic=layout == "periodic")


def _migrate_body(rank, q, layout, world):
    import torch.distributed as dist
    pos0, pos1, feat = _cloud(layout, world)
    halo = _halo(layout, world, pos0, rank)
    own = (halo.owner_of(torch.as_tensor(pos0)) == rank).nonzero().flatten()
    p, ids, x = torch.as_tensor(pos1)[own].clone(), own.clone(), torch.as_tensor(feat)[own].clone()
    owner_before = halo.owner_of(p).tolist()
    halo.setup(torch.as_tensor(pos0)[own], x, 0.1)               # some setup state for the migration to drop
    gen = halo.generation
    p2, ids2, x2 = halo.migrate(p, ids, x)
    assert p2.dtype == torch.float32 and ids2.dtype == torch.int64 and x2.shape == (p2.shape[0], 5)
    assert not p2.requires_grad and p2.is_contiguous() and ids2.shape == (p2.shape[0],)
    moved = dict(out=list(halo.migrated_out), into=list(halo.migrated_in), total=halo.migrated, gen=halo.generation - gen)
    with pytest.raises(RuntimeError, match="setup"):
        halo.update_positions(p2, x2)
    again = halo.migrate(p2, ids2, x2)                           # nobody moves: the inputs themselves
    same = again[0] is p2 and again[1] is ids2 and again[2] is x2 and halo.generation == gen + 1 and halo.migrated == 0
    q.put(("ok", rank, own.tolist(), owner_before, ids2.tolist(), p2.numpy().view(np.int32), x2.numpy().view(np.int32),
           bool((halo.owner_of(p2) == rank).all()), moved, same))
    dist.barrier()


def _migrate_worker(rank, world, layout, q):
    _report(rank, q, _migrate_body, 1, layout, world)


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("layout", ["open", "periodic", "morton"])
def test_migrate_moves_every_particle_to_its_owner(layout, world):
    got = gloo_ranks.run(_migrate_worker, world, (layout,), world, 120)
    _errors(got)
    by = {g[1]: g for g in got}
    assert sorted(by) == list(range(world))
    _, pos1, feat = _cloud(layout, world)
    ids_all = np.concatenate([by[r][4] for r in range(world)]).astype(np.int64)
    assert len(ids_all) == N and np.array_equal(np.sort(ids_all), np.arange(N))      # nothing lost, nothing doubled
    total = 0
    for r in range(world):
        _, _, before, owner_before, after, pbits, xbits, owned, moved, same = by[r]
        assert owned and same
        after = np.asarray(after, np.int64)
        assert np.array_equal(pbits, pos1[after].view(np.int32))                      # the caller's bits, unwrapped as they were
        assert np.array_equal(xbits, feat[after].view(np.int32))
        # the order contract from the owner arrays before the move: stayers, then arrivals by source rank, sender's order
        want = [i for i, o in zip(before, owner_before) if o == r]
        for s in range(world):
            if s != r:
                want += [i for i, o in zip(by[s][2], by[s][3]) if o == r]
        assert after.tolist() == want
        assert moved["gen"] == 1 and moved["total"] == by[0][8]["total"]
        for s in range(world):
            assert moved["out"][s] == by[s][8]["into"][r]
            assert moved["out"][s] == (0 if s == r else sum(1 for o in owner_before if o == s))
        total += sum(moved["out"])
    assert total == by[0][8]["total"] >= N // 20                 # a condition on the inputs: the move crossed many faces
    assert all(sum(by[r][8]["out"]) > 0 and sum(by[r][8]["into"]) > 0 for r in range(world))


# ---------------------------------------------------------------------------------------------------------------------
# 2: a position that is not finite: every rank raises, nobody waits
# ---------------------------------------------------------------------------------------------------------------------
def _nonfinite_body(rank, q):
    import torch.distributed as dist
    pos0, pos1, feat = _cloud("periodic", 2)
    halo = _halo("periodic", 2, pos0, rank)
    own = (halo.owner_of(torch.as_tensor(pos0)) == rank).nonzero().flatten()
    p = torch.as_tensor(pos1)[own].clone()
    if rank == 1:
        p[3, 2] = float("inf")
    gen = halo.generation
    try:
        halo.migrate(p, own.clone())
        q.put(("raised", rank, "nothing"))
    except ValueError as e:
        q.put(("raised", rank, "ValueError" if "1 particle" in str(e) and halo.generation == gen else str(e)))
    dist.barrier()


def _nonfinite_worker(rank, world, q):
    _report(rank, q, _nonfinite_body, 1)


def test_nonfinite_position_raises_on_every_rank():
    got = gloo_ranks.run(_nonfinite_worker, 2, (), 2, 120)
    _errors(got)
    assert sorted(g[1:] for g in got) == [(0, "ValueError"), (1, "ValueError")]


# ---------------------------------------------------------------------------------------------------------------------
# 3: re-balancing a Morton layout is fit + migrate
# ---------------------------------------------------------------------------------------------------------------------
def _rebalance_body(rank, q):
    import torch.distributed as dist
    world = 4
    pos0, _, feat = _cloud("morton", world)
    halo = _halo("morton", world, pos0, rank)
    part = halo.partition
    own = (halo.owner_of(torch.as_tensor(pos0)) == rank).nonzero().flatten()
    assert own.numel() == part.counts[rank]
    # the blob drifts along x: under the old splitters the ranks' shares are no longer equal
    drift = pos0.copy()
    drift[:, 0] = np.clip(drift[:, 0] * f32(0.5) + f32(0.45), 0.0, 1.0 - 2.0 ** -20)
    p, ids = torch.as_tensor(drift)[own].clone(), own.clone()
    stale = torch.bincount(halo.owner_of(torch.as_tensor(drift)), minlength=world).tolist()
    part.fit(p, halo.group)                                      # every rank: its own particles, summed over the group
    p2, ids2 = halo.migrate(p, ids)
    q.put(("ok", rank, stale, list(part.counts), part.hist_max, int(p2.shape[0]), ids2.tolist(),
           bool((halo.owner_of(p2) == rank).all())))
    dist.barrier()


def _rebalance_worker(rank, world, q):
    _report(rank, q, _rebalance_body, 1)


def test_morton_rebalance_is_fit_then_migrate():
    got = gloo_ranks.run(_rebalance_worker, 4, (), 4, 120)
    _errors(got)
    by = {g[1]: g for g in got}
    stale, counts, hist_max = by[0][2], by[0][3], by[0][4]
    assert max(stale) - min(stale) > N // 8, stale               # a condition on the inputs: the drift unbalanced the ranks
    assert sum(counts) == N and all(abs(c - N / 4) < hist_max for c in counts)
    for r in range(4):
        assert by[r][3] == counts and by[r][5] == counts[r] and by[r][7]
    assert sorted(i for r in range(4) for i in by[r][6]) == list(range(N))


# ---------------------------------------------------------------------------------------------------------------------
# 4: ShardedNeighborList.redistribute through a face crossing, two ranks, periodic
# ---------------------------------------------------------------------------------------------------------------------
def _trajectory():
    """Dyadic points on the 1/64 lattice shifted by 1/128 (tests/test_sharded_list_host.py) and four steps: the build, a
    small move of everybody, ONE particle of rank 0 next to the plane x = 1/2 crossing it by 1/32 > skin / 2, a small move."""
    rng = np.random.default_rng(31)
    p0 = ((rng.integers(0, 64, size=(260, 3)) + 0.5) / 64.0).astype(f32)
    p1 = p0 + (rng.integers(-2, 3, size=p0.shape) / 512.0).astype(f32)
    left = np.where(p0[:, 0] < 0.5)[0]
    star = int(left[np.argmax(p0[left, 0])])
    p2 = p1.copy()
    p2[star, 0] = p0[star, 0] + f32(1.0 / 32.0)
    assert p0[star, 0] > 0.5 - 1.0 / 32.0 and p2[star, 0] > 0.5
    p3 = p2 + (rng.integers(-1, 2, size=p0.shape) / 512.0).astype(f32)
    return [p0, p1, p2, p3], star


def _periodic_pairs(p):
    """Codes dst * n + src of the directed pairs within R under the minimum image, by all pairs in fp64 (exact: dyadic)."""
    d = p[None, :, :].astype(np.float64) - p[:, None, :].astype(np.float64)
    d -= np.rint(d)
    near = (d * d).sum(-1) <= np.float64(f32(R)) ** 2
    np.fill_diagonal(near, False)
    dst, src = np.nonzero(near)
    return np.sort(dst * len(p) + src)


def _list_body(rank, q):
    import torch.distributed as dist
    from scalable_e3_gnn_amd import OwnershipChanged, ShardedNeighborList
    from scalable_e3_gnn_amd.sharding import GridHalo

    steps, star = _trajectory()
    M = len(steps[0])
    calls = [0]
    plain_all_reduce = dist.all_reduce

    def counted(*a, **k):
        calls[0] += 1
        return plain_all_reduce(*a, **k)

    dist.all_reduce = counted
    log = {}
    for mode in ("update alone", "redistribute first"):
        halo = GridHalo((2, 1, 1), LO, HI, periodic=True)
        nl = ShardedNeighborList(R, SKIN, halo, graph_builder=_brute_graph)
        ids = (halo.owner_of(torch.as_tensor(steps[0])) == rank).nonzero().flatten()
        n0 = ids.numel()
        x = ids.float()[:, None].clone()
        per_step, pairs, kept_inputs = [], [], []
        for k, P in enumerate(steps):
            p = torch.as_tensor(P)[ids]
            calls[0] = 0
            try:
                if mode == "redistribute first":
                    out = nl.redistribute(p, x, ids)
                    kept_inputs.append(out[0] is p and out[1] is x and out[2] is ids)
                    p, x, ids = out
                cloud = nl.update(p, x)
            except OwnershipChanged:
                per_step.append("OwnershipChanged")
                break
            per_step.append((calls[0], nl.rebuilt, nl.builds, nl.migrations, nl.migrated, int(p.shape[0]) - n0))
            g = cloud.split.graph
            gid = cloud.x[:, 0].long()
            pairs.append((gid[g.dst.long()] * M + gid[g.src.long()]).numpy())
            assert torch.equal(gid[halo.owned_new], ids) and bool((halo.owner_of(p) == rank).all())
        log[mode] = (per_step, pairs, kept_inputs)
    dist.all_reduce = plain_all_reduce
    q.put(("ok", rank, log, star))
    dist.barrier()


def _list_worker(rank, world, q):
    _report(rank, q, _list_body, 1)


def test_list_redistributes_through_a_crossing():
    got = gloo_ranks.run(_list_worker, 2, (), 2, 120)
    _errors(got)
    by = {g[1]: g[2] for g in got}
    steps, _ = _trajectory()
    for r in (0, 1):
        alone, _, _ = by[r]["update alone"]
        # the existing behaviour: build, hold, and the crossing raises on BOTH ranks
        assert [s if isinstance(s, str) else s[1:3] for s in alone] == [(True, 1), (False, 1), "OwnershipChanged"], alone
        first, _, kept = by[r]["redistribute first"]
        assert [s[1:4] for s in first] == [(True, 1, 0), (False, 1, 0), (True, 2, 1), (False, 2, 1)], first
        assert [s[4] for s in first] == [0, 0, 1, 1]                                  # one particle changed rank, once
        assert [s[5] for s in first] == [0, 0, (-1, 1)[r], (-1, 1)[r]]
        assert kept == [True, True, False, True]                  # nobody moved, or the list held: the inputs themselves
        # a holding step costs one all-reduce, with redistribute or without
        assert alone[1][0] == first[1][0] == first[3][0] == 1, (alone, first)
    for k in range(4):
        both = np.sort(np.concatenate([by[r]["redistribute first"][1][k] for r in (0, 1)]))
        want = _periodic_pairs(steps[k])
        assert len(want) > 260 and np.array_equal(both, want), k

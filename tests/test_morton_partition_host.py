"""Equal-count Morton key ranges (sharding.MortonPartition / select_morton_torch / MortonHalo), host side: the balance
guarantee ``|n_q - N/P| < max(hist)``, distributed ``fit`` == single-process ``fit``, the ghost predicate against a brute
force that shares no code with ``sharding.py``, the superset property against the whole-cloud fp32 graph, and the errors.
Runs without a GPU (the C entry's argument check precedes every HIP call)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.distributed as dist

import gloo_ranks
import models  # noqa: F401
from scalable_e3_gnn_amd import _lib
from scalable_e3_gnn_amd.sharding import MortonHalo, MortonPartition, select_morton_torch


def clustered_slab_cloud(N, world):
    """tests/test_sharding_gloo.py's ``clustered`` cloud: 70 % of the particles in a blob across the 1|2 face."""
    g = torch.Generator().manual_seed(7)
    pos = torch.rand(N, 3, generator=g, dtype=torch.float64)
    blob = torch.rand(N, generator=g) < 0.7
    pos[:, 0] = torch.where(blob, 2.0 + 0.35 * torch.randn(N, generator=g, dtype=torch.float64), pos[:, 0] * world)
    pos[:, 0].clamp_(0.0, world - 1e-9)
    return pos.float()


def blob_x_cloud(N, seed=11):
    """Box [0,2) x [0,1)^2, 60 % of x drawn from 1.45 + 0.18 randn, clamped to [0, 2 - 2^-20]."""
    g = torch.Generator().manual_seed(seed)
    pos = torch.rand(N, 3, generator=g)
    pos[:, 0] *= 2.0
    blob = torch.rand(N, generator=g) < 0.6
    pos[:, 0] = torch.where(blob, 1.45 + 0.18 * torch.randn(N, generator=g), pos[:, 0])
    pos[:, 0].clamp_(0.0, 2.0 - 2.0 ** -20)
    return pos


def blob_3d_cloud(N, seed=11):
    """Unit cube, 60 % of the particles in a blob at (0.3, 0.65, 0.6), sigma 0.15, clamped into the cube."""
    g = torch.Generator().manual_seed(seed)
    pos = torch.rand(N, 3, generator=g)
    blob = torch.rand(N, generator=g) < 0.6
    c = torch.tensor([0.3, 0.65, 0.6])
    pos = torch.where(blob[:, None], c + 0.15 * torch.randn(N, 3, generator=g), pos)
    return pos.clamp_(0.0, 1.0 - 2.0 ** -20)


def _density_r(k, n_per_volume):
    return float((3 * k / (4 * np.pi * n_per_volume)) ** (1 / 3))


# name -> (positions, lo, hi, world, r, equal-volume grid)
def _clouds():
    return {
        "slab4": (clustered_slab_cloud(2400, 4), (0, 0, 0), (4, 1, 1), 4, _density_r(10.0, 600), (4, 1, 1)),
        "blob_x2": (blob_x_cloud(6000), (0, 0, 0), (2, 1, 1), 2, _density_r(16.0, 3000), (2, 1, 1)),
        "blob_3d8": (blob_3d_cloud(6000), (0, 0, 0), (1, 1, 1), 8, _density_r(10.0, 6000), (2, 2, 2)),
    }


# regression pin (equal-volume counts, Morton counts): the fp32 restatement reproduces the prototype's table exactly
PINNED = {
    "slab4": ([190, 1018, 1017, 175], [632, 576, 604, 588]),
    "blob_x2": ([1207, 4793], [3011, 2989]),
    "blob_3d8": ([449, 670, 1008, 2340, 304, 358, 363, 508], [753, 750, 751, 750, 773, 733, 749, 741]),
}
CROSS_EDGES = {"slab4": 6874, "blob_x2": 9492, "blob_3d8": 46842}


@pytest.mark.parametrize("name", ["slab4", "blob_x2", "blob_3d8"])
def test_balance_bound_and_ownership(name):
    pos, lo, hi, world, r, dims = _clouds()[name]
    N = pos.shape[0]
    part = MortonPartition(lo, hi, r, world).fit(pos)
    keys = part.keys(pos)
    hist = torch.bincount(keys, minlength=part.n_keys)
    owner = part.owner_of(pos)
    inner = torch.as_tensor(part.splitters[1:-1], dtype=torch.long)
    assert torch.equal(owner, torch.searchsorted(inner, keys, right=True))
    counts = torch.bincount(owner, minlength=world).tolist()
    assert counts == part.counts and sum(counts) == N          # every particle owned exactly once
    assert part.splitters[0] == 0 and part.splitters[-1] == part.n_keys and len(part.splitters) == world + 1
    assert all(a <= b for a, b in zip(part.splitters, part.splitters[1:]))
    for a in range(3):                                           # a cell is never narrower than r
        assert part.cell_width(a) >= r and (part.grid[a] & (part.grid[a] - 1)) == 0
    vol = torch.bincount(_volume_owner(pos, dims, lo, hi), minlength=world).tolist()
    print(f"\n{name}: N={N} world={world} grid={part.grid} equal-volume {vol}  Morton {counts}  fullest cell {int(hist.max())}")
    assert part.hist_max == int(hist.max())
    for n_q in counts:
        assert abs(n_q - N / world) < int(hist.max())
    assert max(vol) > 3 * min(vol)                               # the equal-volume cut of these clouds is unbalanced
    assert (vol, counts) == PINNED[name]


def _volume_owner(pos, dims, lo, hi):
    """Equal-volume ownership (GridHalo's rule): rank = (ix py + iy) pz + iz of the box that holds the position."""
    c = [((pos[:, a] - lo[a]) / ((hi[a] - lo[a]) / dims[a])).floor().long().clamp_(0, dims[a] - 1) for a in range(3)]
    return (c[0] * dims[1] + c[1]) * dims[2] + c[2]


def _fit_worker(rank, world, q):
    pos, lo, hi, _, r, _ = _clouds()["blob_3d8"]
    perm = torch.randperm(pos.shape[0], generator=torch.Generator().manual_seed(3))
    mine = perm[rank::world][: 900 + 300 * rank] if rank < world - 1 else None    # arbitrary, unequal parts
    if mine is None:
        taken = torch.cat([perm[k::world][: 900 + 300 * k] for k in range(world - 1)])
        keep = torch.ones(pos.shape[0], dtype=torch.bool)
        keep[taken] = False
        mine = keep.nonzero().flatten()
    part = MortonPartition(lo, hi, r, world).fit(pos[mine])
    q.put((rank, int(mine.numel()), part.splitters, part.counts, part.hist_max))
    dist.barrier()


@pytest.mark.timeout(300)
def test_distributed_fit_equals_single_process_fit():
    world = 4
    got = gloo_ranks.run(_fit_worker, world, (), world, 120)
    pos, lo, hi, _, r, _ = _clouds()["blob_3d8"]
    assert sum(g[1] for g in got) == pos.shape[0]
    whole = MortonPartition(lo, hi, r, world).fit(pos)
    for _, _, splitters, counts, hist_max in got:
        assert splitters == whole.splitters and counts == whole.counts and hist_max == whole.hist_max


def test_world_13_empty_ranks_and_empty_cloud():
    pos, lo, hi, _, r, _ = _clouds()["blob_3d8"]
    part = MortonPartition(lo, hi, r, 13).fit(pos)
    assert sum(part.counts) == 6000 and all(abs(c - 6000 / 13) < part.hist_max for c in part.counts)
    assert torch.equal(torch.bincount(part.owner_of(pos), minlength=13), torch.as_tensor(part.counts))
    # more ranks than non-empty cells: 5 particles in 2 cells over 8 ranks
    few = torch.tensor([[0.1, 0.1, 0.1]] * 3 + [[0.9, 0.9, 0.9]] * 2)
    part = MortonPartition(lo, hi, 0.2, 8).fit(few)
    assert sorted(c for c in part.counts if c) == [2, 3] and part.counts.count(0) == 6
    assert torch.equal(torch.bincount(part.owner_of(few), minlength=8), torch.as_tensor(part.counts))
    for q in range(8):                                           # the selection works with ranks that own nothing
        own = few[part.owner_of(few) == q]
        idx, cnt = select_morton_torch(own, lo, hi, part.grid, 0.2, part.splitters, q)
        assert len(cnt) == 8 and cnt[q] == 0 and sum(cnt) == idx.numel()
    empty = MortonPartition(lo, hi, 0.2, 4).fit(torch.zeros(0, 3))
    assert empty.counts == [0, 0, 0, 0] and empty.splitters[0] == 0 and empty.splitters[-1] == empty.n_keys
    idx, cnt = select_morton_torch(torch.zeros(0, 3), lo, hi, empty.grid, 0.2, empty.splitters, 1)
    assert idx.numel() == 0 and cnt == [0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------------
# the predicate against a brute force (python loops, no code shared with sharding.py), dyadic cloud on cell faces +- r
# ---------------------------------------------------------------------------------------------------------------------
R_EXACT = 0.125


def face_cloud():
    """Dyadic positions (1/256 grid) in the unit cube plus every combination of cell faces (k / 4) and faces +- r."""
    rng = np.random.default_rng(17)
    pos = rng.integers(0, 256, size=(1500, 3)) / 256.0
    v = [0.25 - R_EXACT, 0.25, 0.25 + R_EXACT, 0.5, 0.75 - R_EXACT, 0.75]
    extra = [[a, b, c] for a in v for b in v for c in v]
    return np.concatenate([pos, np.asarray(extra, np.float64)])


def _brute_key(cx, cy, cz):
    k = 0
    for b in range(10):
        k |= ((cx >> b) & 1) << (3 * b) | ((cy >> b) & 1) << (3 * b + 1) | ((cz >> b) & 1) << (3 * b + 2)
    return k


def _brute_owner(splitters, key):
    return max(q for q in range(len(splitters) - 1) if splitters[q] <= key)


def _brute_cell(x, n):
    return min(max(int(np.floor(x * n)), 0), n - 1)     # unit cube, n a power of two, dyadic x: exact


def test_predicate_equals_brute_force_on_cell_faces():
    pos = face_cloud()
    n, world = 4, 5                                      # cells 1/4 wide, r = 1/8
    part = MortonPartition((0, 0, 0), (1, 1, 1), R_EXACT, world, max_bits=2).fit(torch.as_tensor(pos).float())
    assert part.grid == (n, n, n)
    owner = [_brute_owner(part.splitters, _brute_key(*[_brute_cell(x, n) for x in p])) for p in pos]
    assert owner == part.owner_of(torch.as_tensor(pos).float()).tolist()
    on_hi = on_lo = 0
    for me in range(world):
        own = [i for i in range(len(pos)) if owner[i] == me]
        want = {q: [] for q in range(world)}
        for local, i in enumerate(own):
            rng = [range(_brute_cell(x - R_EXACT, n), _brute_cell(x + R_EXACT, n) + 1) for x in pos[i]]
            dests = {_brute_owner(part.splitters, _brute_key(cx, cy, cz)) for cx in rng[0] for cy in rng[1] for cz in rng[2]}
            for q in dests - {me}:
                want[q].append(local)
            on_hi += any((x + R_EXACT) * n == np.floor((x + R_EXACT) * n) and 0 < x + R_EXACT < 1 for x in pos[i])
            on_lo += any((x - R_EXACT) * n == np.floor((x - R_EXACT) * n) and 0 < x - R_EXACT < 1 for x in pos[i])
        idx, cnt = select_morton_torch(torch.as_tensor(pos[own]).float(), part.lo, part.hi, part.grid, R_EXACT,
                                       part.splitters, me)
        assert cnt == [len(want[q]) for q in range(world)]
        assert idx.tolist() == [i for q in range(world) for i in want[q]]     # grouped by rank, ascending inside
    assert on_hi > 0 and on_lo > 0                        # both ends of the cell range sit exactly on faces


# ---------------------------------------------------------------------------------------------------------------------
# superset: no cross-owner edge of the whole-cloud fp32 graph lacks its source among the destination owner's ghosts
# ---------------------------------------------------------------------------------------------------------------------
def _fp32_edges(pos, r):
    """(dst, src) of the brute-force fp32 graph: d2 = fl32(fl32(dx dx + dy dy) + dz dz) <= fl32(r r), the builder's order."""
    p = pos.numpy().astype(np.float32)
    r2 = np.float32(r) * np.float32(r)
    out = []
    for s in range(0, len(p), 500):
        d = p[s:s + 500, None, :] - p[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        i, j = np.nonzero(d2 <= r2)
        keep = (i + s) != j
        out.append(np.stack([i[keep] + s, j[keep]], 1))
    return np.concatenate(out)


@pytest.mark.parametrize("name", ["slab4", "blob_x2", "blob_3d8"])
def test_ghosts_cover_every_cross_edge(name):
    pos, lo, hi, world, r, _ = _clouds()[name]
    part = MortonPartition(lo, hi, r, world).fit(pos)
    owner = part.owner_of(pos).numpy()
    sent = np.zeros((world, pos.shape[0]), dtype=bool)           # sent[q, j]: j is a ghost of rank q
    for me in range(world):
        own = np.nonzero(owner == me)[0]
        idx, cnt = select_morton_torch(pos[own], part.lo, part.hi, part.grid, r, part.splitters, me)
        dest = np.repeat(np.arange(world), cnt)
        sent[dest, own[idx.numpy()]] = True
    e = _fp32_edges(pos, r)
    cross = e[owner[e[:, 0]] != owner[e[:, 1]]]
    missing = int((~sent[owner[cross[:, 0]], cross[:, 1]]).sum())
    print(f"\n{name}: {len(e)} edges, {len(cross)} between owners, {missing} without a ghost; ghosts / owned = "
          f"{sent.sum() / pos.shape[0]:.3f}")
    assert len(cross) == CROSS_EDGES[name] and missing == 0


# ---------------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------------
def test_errors():
    box = ((0, 0, 0), (1, 1, 1))
    with pytest.raises(NotImplementedError, match="GridHalo"):
        MortonPartition(*box, 0.1, 4, periodic=True)
    with pytest.raises(NotImplementedError, match="GridHalo"):
        MortonPartition(*box, 0.1, 4, periodic=(False, True, False))
    with pytest.raises(ValueError):
        MortonPartition(*box, 0.1, 65)
    with pytest.raises(ValueError):
        MortonPartition(*box, 0.1, 0)
    with pytest.raises(ValueError):
        MortonPartition(*box, 0.0, 4)
    with pytest.raises(ValueError):
        MortonPartition(*box, 0.1, 4, max_bits=8)
    with pytest.raises(ValueError):
        MortonPartition((0, 0, 0), (1, 0, 1), 0.1, 4)
    with pytest.raises(ValueError):
        MortonPartition((0, 0, 0), (1, float("inf"), 1), 0.1, 4)
    pos = torch.rand(200, 3, generator=torch.Generator().manual_seed(1))
    part = MortonPartition(*box, 0.1, 1).fit(pos)                 # world 1: no process group needed
    assert part.grid == (8, 8, 8)
    halo = MortonHalo(part)
    with pytest.raises(ValueError, match="cell width"):
        halo.setup(pos, pos, 0.126)
    with pytest.raises(TypeError):
        halo.setup(pos.double(), pos, 0.1)
    lp, lf = halo.setup(pos, pos.to(torch.bfloat16), 0.125)       # r == cell width is legal; world 1 has no ghosts
    assert lp.shape == (200, 3) and lf.dtype == torch.bfloat16 and halo.n_ghost == 0 and halo.neighbours == []
    with pytest.raises(ValueError, match="ranks"):
        MortonHalo(MortonPartition(*box, 0.1, 4).fit(pos))        # no group: world 1, the partition wants 4
    with pytest.raises(RuntimeError):
        MortonHalo(MortonPartition(*box, 0.1, 1))                 # not fitted


def test_c_entry_rejects_bad_arguments_before_any_hip_call():
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()                                # host memory: never touched, nothing is launched
    p = ctypes.addressof(buf)
    lo, hi = _lib.Float3(0, 0, 0), _lib.Float3(1, 1, 1)

    def count(n=10, n_cells=(8, 8, 8), r=0.1, splitters=(0, 100, 512), self_rank=0, lo=lo, hi=hi):
        P = len(splitters) - 1
        return lib.e3_morton_select_count(p, n, lo, hi, _lib.Int3(*n_cells), r, (ctypes.c_int32 * (P + 1))(*splitters), P,
                                          self_rank, p, p, 4096, None)

    def fill(splitters=(0, 100, 512), **kw):
        P = len(splitters) - 1
        return lib.e3_morton_select_fill(p, 10, lo, hi, _lib.Int3(8, 8, 8), 0.1, (ctypes.c_int32 * (P + 1))(*splitters), P, 0,
                                         5, p, p, 4096, None)

    bad = 1                                                       # E3_ERR_INVALID_ARG
    assert count(splitters=(0, 300, 200, 512)) == bad             # decreasing
    assert count(splitters=(1, 100, 512)) == bad                  # s_0 != 0
    assert fill(splitters=(0, 300, 200, 512)) == bad
    assert count(splitters=tuple([0] * 66)) == bad                # 65 ranks
    assert count(self_rank=2) == bad and count(self_rank=-1) == bad
    assert count(n_cells=(8, 6, 8)) == bad and count(n_cells=(256, 8, 8)) == bad and count(n_cells=(0, 8, 8)) == bad
    assert count(r=0.126) == bad and count(r=0.0) == bad and count(r=float("nan")) == bad      # cell narrower than r
    assert count(hi=_lib.Float3(1, 0, 1)) == bad and count(lo=_lib.Float3(float("nan"), 0, 0)) == bad
    assert count(n=2 ** 30, splitters=(0, 100, 512)) == bad       # n * n_ranks >= 2^31 - 1
    assert lib.e3_morton_select_workspace_bytes(10, 65) == -1 and lib.e3_morton_select_workspace_bytes(-1, 2) == -1
    assert lib.e3_morton_keys(p, 10, lo, hi, _lib.Int3(8, 6, 8), p, None) == bad

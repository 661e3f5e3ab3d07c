"""The sharded Verlet list on the GPU (include/e3gnn.h: e3_nl_update_split; sharded_list.ShardedNeighborList; envelope=,
skin= and neighbors= of ``ShardedEnergyModel``).

  1. the fused entry against the composition e3_nl_update -> e3_split_edges and against the numpy restatement
     (tests/sharded_list_reference.py), exactly, on the clustered cloud of tests/test_neighbor_list_gpu.py;
  2. world 1, periodic self-halo: the enveloped sharded model against the enveloped ``PeriodicEnergyModel``, skin invariance,
     the no-grad route;
  3. world 1, a trajectory: the model with ``neighbors=`` against the same model without, the rebuild schedule, re-wrapped
     coordinates, and the list's pairs against a fresh build as sets;
  4. two ranks sharing cuda:0 over gloo: three steps against the whole cloud's reference, the collective rebuild and the
     collective ``OwnershipChanged``;
  5. error paths, ``invalidate``, a foreign ``halo.setup``, a ``MortonHalo``."""
import numpy as np
import pytest
import torch

import gloo_ranks
import models  # noqa: F401  (registers scalable_e3_gnn_amd -- also in the spawned ranks, which import this module)
import sharded_list_reference as SR
from scalable_e3_gnn_amd import OwnershipChanged, ShardedEnergyModel, ShardedNeighborList, _lib
from scalable_e3_gnn_amd.batched import PeriodicEnergyModel
from scalable_e3_gnn_amd.radius_graph import radius_graph
from scalable_e3_gnn_amd.sharding import GridHalo, MortonHalo, MortonPartition
from test_neighbor_list_gpu import BUILDS, _band_free, _clustered, _compare, _moved, _quiet, _trajectory, _uniform

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
R, SKIN = 0.2, 0.05                      # the entry tests and the trajectory: those of tests/test_neighbor_list_gpu.py
LO, HI = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
IN = "1x0e+1x1o"
LAYERS = 2
RM = 1.0 / (LAYERS + 2.2)                # the model tests: the cutoff of tests/test_sharded_forces_gpu.py


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# 1: the entry
# ---------------------------------------------------------------------------------------------------------------------
def _fused(pos, g, ghost8, r):
    """One call of e3_nl_update_split on the stored graph g -> numpy [pos4, rowptr, src, dst, src_i, dst_i, src_b, dst_b,
    stats]; nothing may be written past the counts."""
    lib = _lib.load()
    N, E = g.perm.numel(), g.num_edges
    pos = torch.as_tensor(pos).to(DEV).contiguous()
    pos4 = torch.full((N, 4), 7.0, device=DEV)
    rowptr = torch.full((N + 1,), -5, dtype=torch.int32, device=DEV)
    outs = [torch.full((max(E, 1),), -5, dtype=torch.int32, device=DEV) for _ in range(6)]
    stats = torch.full((4,), -1, dtype=torch.int32, device=DEV)
    ws = torch.empty(max(int(lib.e3_nl_update_split_workspace_bytes(N)), 16), dtype=torch.uint8, device=DEV)
    status = lib.e3_nl_update_split(pos.data_ptr(), g.perm.data_ptr(), g.pos4.data_ptr(), g.rowptr.data_ptr(), g.src.data_ptr(),
                                    ghost8.data_ptr() if N else None, N, E, float(r), pos4.data_ptr(), rowptr.data_ptr(),
                                    *[o.data_ptr() for o in outs], stats.data_ptr(), ws.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
    assert status == 0, status
    st = stats.cpu().numpy().view(np.uint32)
    counts = [int(st[1]), int(st[1]), int(st[2]), int(st[2]), int(st[3]), int(st[3])]
    for o, c in zip(outs, counts):
        assert bool(torch.all(o[c:] == -5))
    return [pos4.cpu().numpy(), rowptr.cpu().numpy()] + [o[:c].cpu().numpy() for o, c in zip(outs, counts)] + [st]


def _composed(pos, g, ghost8, r):
    """e3_nl_update, then e3_split_edges on its result -> the same nine arrays."""
    lib = _lib.load()
    N, E = g.perm.numel(), g.num_edges
    pos = torch.as_tensor(pos).to(DEV).contiguous()
    pos4 = torch.empty((N, 4), device=DEV)
    rowptr = torch.empty(N + 1, dtype=torch.int32, device=DEV)
    src, dst = (torch.empty(max(E, 1), dtype=torch.int32, device=DEV) for _ in range(2))
    st2 = torch.zeros(2, dtype=torch.int32, device=DEV)
    ws = torch.empty(max(int(lib.e3_nl_workspace_bytes(N)), 16), dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.e3_nl_update(pos.data_ptr(), g.perm.data_ptr(), g.pos4.data_ptr(), g.rowptr.data_ptr(), g.src.data_ptr(), N, E,
                            float(r), pos4.data_ptr(), rowptr.data_ptr(), src.data_ptr(), dst.data_ptr(), st2.data_ptr(),
                            ws.data_ptr(), stream) == 0
    bits, e_r = (int(v) for v in st2.cpu().numpy().view(np.uint32))
    rowptr2 = torch.empty(N + 1, dtype=torch.int32, device=DEV)
    outs = [torch.empty(max(e_r, 1), dtype=torch.int32, device=DEV) for _ in range(6)]
    counts = torch.empty(4, dtype=torch.int32, device=DEV)
    work = torch.empty(max(int(lib.e3_split_edges_workspace_bytes(N)), 16), dtype=torch.uint8, device=DEV)
    assert lib.e3_split_edges(rowptr.data_ptr(), src.data_ptr(), ghost8.data_ptr(), N, e_r, rowptr2.data_ptr(),
                              *[o.data_ptr() for o in outs], counts.data_ptr(), work.data_ptr(), stream) == 0
    ek, ei, eb = (int(v) for v in counts[:3].tolist())
    cs = [ek, ek, ei, ei, eb, eb]
    return ([pos4.cpu().numpy(), rowptr2.cpu().numpy()] + [o[:c].cpu().numpy() for o, c in zip(outs, cs)] +
            [np.array([bits, ek, ei, eb], np.uint32)])


def _restated(pos, g, ghost8, r):
    p4, rp, k, i, b, st = SR.update_split(pos, g.perm.cpu().numpy(), g.pos4.cpu().numpy(), g.rowptr.cpu().numpy(),
                                          g.src.cpu().numpy(), ghost8.cpu().numpy(), r)
    return [p4, rp, *k, *i, *b, st]


NAMES = ("pos4", "rowptr", "src", "dst", "src_interior", "dst_interior", "src_boundary", "dst_boundary", "stats")


def _assert_same(got, want):
    for name, a, b in zip(NAMES, got, want):
        assert a.shape == b.shape and torch.equal(torch.as_tensor(a.view(np.int32)), torch.as_tensor(b.view(np.int32))), name


def _ghost_flags(kind, deg):
    n = len(deg)
    if kind == "none":
        return np.zeros(n, bool)
    if kind == "all":
        return np.ones(n, bool)
    if kind == "seeded":
        return np.random.default_rng(5).random(n) < 0.3
    return deg == 64                                             # exactly the rows of the clique of 65 points


@pytest.mark.parametrize("n", [None, 369])                       # 380 points, and a count with N mod 16 = 1
@pytest.mark.parametrize("flags", ["none", "all", "seeded", "clique"])
def test_entry_equals_composition_and_restatement(flags, n):
    pos, rng = _clustered("open", 12)
    assert len(pos) <= 400
    new = _moved(pos, rng, None)                                 # every point displaced by 0.05 .. 0.45 skin
    if n is not None:
        pos, new = pos[:n], new[:n]
        assert len(pos) % 16 == 1
    g = radius_graph(torch.as_tensor(pos).to(DEV), R + SKIN, LO, [4.0, 4.0, 4.0])     # edges into every row
    deg = np.diff(g.rowptr.cpu().numpy())
    ghost = _ghost_flags(flags, deg)
    ghost8 = torch.as_tensor(ghost).to(torch.uint8).to(DEV)
    got = _fused(new, g, ghost8, R)
    _assert_same(got, _composed(new, g, ghost8, R))
    _assert_same(got, _restated(new, g, ghost8, R))
    deg_r = np.diff(got[1])
    st = got[8]
    assert st[1] == st[2] + st[3] == len(got[2]) and np.all(deg_r[ghost] == 0)
    if n is None:
        # preconditions on the inputs: the group and wave boundaries of the row walk, rows of different lengths in one
        # wave (four rows), an owned row that loses all its edges
        assert {0, 1, 15, 16, 17, 63, 64, 65} <= set(deg.tolist()) and deg.max() >= 130, sorted(set(deg.tolist()))
        assert any(len(set(deg[w:w + 4].tolist())) > 1 for w in range(0, len(deg), 4))
        if flags == "none":
            assert np.any((deg > 0) & (deg_r == 0)) and np.any((deg >= 130) & (deg_r < deg)) and st[3] == 0
        if flags == "all":
            assert st[1] == 0 and st[0] > 0
        if flags in ("seeded", "clique"):
            assert st[2] > 0 and ghost.any() and not ghost.all()
        if flags == "seeded":
            assert st[3] > 0
        if flags == "clique":
            assert ghost.sum() == 65 and st[3] == 0              # a clique's edges stay inside it: dropped with its rows


def test_entry_empty_single_and_no_edges():
    g0 = radius_graph(torch.zeros((0, 3), device=DEV), R + SKIN, LO, HI)
    got = _fused(np.zeros((0, 3), f32), g0, torch.zeros(0, dtype=torch.uint8, device=DEV), R)
    assert got[1].tolist() == [0] and got[8].tolist() == [0, 0, 0, 0] and got[0].shape == (0, 4)
    one = np.array([[0.3, 0.4, 0.2]], f32)
    g1 = radius_graph(torch.as_tensor(one).to(DEV), R + SKIN, LO, HI)
    for flag in (0, 1):
        gh = torch.full((1,), flag, dtype=torch.uint8, device=DEV)
        got = _fused(one + f32(0.01), g1, gh, R)
        _assert_same(got, _restated(one + f32(0.01), g1, gh, R))
        assert got[1].tolist() == [0, 0] and got[8][1:].tolist() == [0, 0, 0] and got[8][0] > 0
    far = np.array([[0.1, 0.1, 0.1], [0.9, 0.9, 0.9], [0.1, 0.9, 0.5]], f32)
    g3 = radius_graph(torch.as_tensor(far).to(DEV), R + SKIN, LO, HI)
    assert g3.num_edges == 0
    gh = torch.tensor([0, 1, 0], dtype=torch.uint8, device=DEV)
    got = _fused(far, g3, gh, R)
    _assert_same(got, _restated(far, g3, gh, R))
    assert got[1].tolist() == [0, 0, 0, 0] and got[8].tolist() == [0, 0, 0, 0]


def test_entry_argument_checks():
    lib = _lib.load()
    t = torch.zeros(64, dtype=torch.int32, device=DEV)
    p = t.data_ptr()
    ok = [p, p, p, p, p, p, 4, 4, 0.2]
    out = [p] * 10 + [None]
    fn = lib.e3_nl_update_split
    for bad_r in (0.0, -1.0, float("nan"), float("inf")):
        assert fn(*ok[:8], bad_r, *out) == 1
    assert fn(*ok[:6], 2 ** 31, 4, 0.2, *out) == 1 and fn(*ok[:7], 2 ** 31 + 1, 0.2, *out) == 1
    assert fn(*ok[:6], -1, 4, 0.2, *out) == 1
    for k in range(6):                                           # is_ghost (k = 5) among them
        assert fn(*[None if i == k else v for i, v in enumerate(ok)], *out) == 1
    for k in range(10):
        assert fn(*ok, *[None if i == k else v for i, v in enumerate(out)]) == 1
    assert lib.e3_nl_update_split_workspace_bytes(-1) == -1 and lib.e3_nl_update_split_workspace_bytes(2 ** 31) == -1
    assert lib.e3_nl_update_split_workspace_bytes(0) > 0
    assert torch.all(t == 0)  # refused before any launch


# ---------------------------------------------------------------------------------------------------------------------
# 2: world 1, periodic self-halo: envelope and skin
# ---------------------------------------------------------------------------------------------------------------------
def _cloud(M, seed, bits=16):
    rng = np.random.default_rng(seed)
    pos = (rng.integers(0, 1 << bits, size=(M, 3)) / float(1 << bits)).astype(f32)
    return torch.as_tensor(pos), torch.as_tensor(rng.standard_normal((M, 4)).astype(f32))


def _pair(H, lmax, seed, envelope=6):
    torch.manual_seed(seed)
    ref = PeriodicEnergyModel(IN, H, LAYERS, lmax=lmax, envelope=envelope).to(DEV)
    sh = ShardedEnergyModel(IN, H, LAYERS, lmax, envelope=envelope).to(DEV)
    sh.load_state_dict(ref.state_dict())
    return ref.eval(), sh.eval()


@pytest.mark.parametrize("H,lmax", [(8, 1), (32, 1), (8, 2), (32, 2)])
def test_world1_enveloped_model_equals_periodic_model(H, lmax):
    pos, x = _cloud(250, 51)
    pos[:20] += 1.0                                              # outside the box: wrapped by the halo
    pos[20:30, 1] -= 1.0
    ref, sh = _pair(H, lmax, 52)
    pd, xd = pos.to(DEV), x.to(DEV)
    want_kw = dict(forces=True, virial=True, stress=True)
    with _quiet():
        got = sh(xd, pd, RM, GridHalo((1, 1, 1), LO, HI, periodic=True), **want_kw)
        want = ref(xd, pd, RM, LO, HI, periodic=True, **want_kw)
    errs = [_rel(a, b) for a, b in zip(got, want)]
    print(f"\nenveloped world-1 self-halo vs PeriodicEnergyModel, H={H} l_max={lmax}: energy {errs[0]:.2e}, forces "
          f"{errs[1]:.2e}, virial {errs[2]:.2e}, stress {errs[3]:.2e}")
    assert got[1].shape == pd.shape and got[2].shape == (3, 3) and float(want[1].abs().max()) > 0
    assert errs[0] < 2e-5 and max(errs[1:]) < 4e-5, errs
    # skin: the halo and the graph at r + skin, the envelope at r
    g0, g1 = radius_graph(pd, RM, LO, HI, periodic=True), radius_graph(pd, RM + SKIN, LO, HI, periodic=True)
    assert g1.num_edges - g0.num_edges >= 200, (g0.num_edges, g1.num_edges)
    with _quiet():
        e1, f1, W1, s1 = sh(xd, pd, RM, GridHalo((1, 1, 1), LO, HI, periodic=True), skin=SKIN, **want_kw)
    e0, f0, W0, s0 = got
    print(f"skin {SKIN} vs 0: energy {abs(float(e1) - float(e0)):.2e}, forces {_rel(f1, f0):.2e}, virial {_rel(W1, W0):.2e}")
    assert abs(float(e1) - float(e0)) < 2e-5 * max(1.0, abs(float(e0)))
    assert _rel(f1, f0) < 2e-5 and _rel(s1, s0) < 2e-5 and _rel(W1, W0) < 2e-5, (_rel(f1, f0), _rel(s1, s0))
    # the no-grad route: blocking exchange + per-product kernels + weighted segment sum
    with torch.no_grad():
        e_fast = sh(xd, pd, RM, GridHalo((1, 1, 1), LO, HI, periodic=True))
    assert e_fast.dim() == 0 and abs(float(e_fast) - float(e0)) < 1e-5 * abs(float(e0)), (float(e_fast), float(e0))


# ---------------------------------------------------------------------------------------------------------------------
# 3: world 1, a trajectory with the list
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("envelope,lmax", [(6, 1), (None, 2)])
def test_world1_model_on_a_trajectory(envelope, lmax):
    pos, rng = _uniform("box", 200, 41)
    x = torch.as_tensor(rng.standard_normal((200, 4)).astype(f32)).to(DEV)
    torch.manual_seed(42)
    model = ShardedEnergyModel(IN, 16, 2, lmax, envelope=envelope).to(DEV).eval()
    halo = GridHalo((1, 1, 1), LO, HI, periodic=True)
    nl = ShardedNeighborList(R, SKIN, halo)
    want = dict(forces=True, virial=True, stress=True)
    steps = _trajectory(pos, 45)                                 # a seed whose every step is band-free (asserted below)
    box = np.ones(3, f32)
    built = steps[0]
    for k, p in enumerate(steps):
        if k in (4, 8):
            built = p
        if envelope is None:
            assert _band_free(built, p, box, None)               # a condition on the inputs (the seed), not on the code
        pd = torch.as_tensor(p).to(DEV)
        with _quiet():
            a = model(x, pd, R, halo, neighbors=nl, **want)
            b = model(x, pd, R, GridHalo((1, 1, 1), LO, HI, periodic=True), **want)
        assert len(a) == 4 and a[1].shape == (200, 3) and a[3].shape == (3, 3)
        _compare(a, b)
        assert nl.builds == BUILDS[k] and nl.updates == k + 1, (k, nl.builds)
        assert nl.rebuilt == (k in (0, 4, 8))
    assert float(b[1].abs().max()) > 0 and float(b[3].abs().max()) > 0
    # a third of the particles re-wrapped by whole periods: nothing has moved
    hop = steps[8].astype(np.float64)
    hop[::3] += rng.integers(-2, 3, size=hop[::3].shape)
    with _quiet():
        c = model(x, torch.as_tensor(hop.astype(f32)).to(DEV), R, halo, neighbors=nl, **want)
    assert nl.builds == 3 and not nl.rebuilt and nl.updates == 10
    _compare(c, b)
    # the no-grad route on the list's cloud, and training mode
    with torch.no_grad():
        e_nl = model(x, pd, R, halo, neighbors=nl)
    assert not nl.rebuilt and abs(float(e_nl) - float(b[0])) < 2e-5 * max(1.0, abs(float(b[0])))
    model.train()
    with _quiet():
        e_train = model(x, pd, R, halo, neighbors=nl)
        e_train.backward()
    assert abs(float(e_train.detach()) - float(b[0])) < 2e-5 * max(1.0, abs(float(b[0])))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())


def _global_pairs(lists, gid, M):
    """(src, dst) local index lists -> sorted codes gid[dst] * M + gid[src]."""
    return [torch.sort(gid[d.long()] * M + gid[s.long()]).values for s, d in lists]


def _fresh_pairs(p1, gid, M):
    """kept / interior / boundary pairs (global ids) of setup + radius_graph + split_graph at R for the positions p1."""
    fresh = GridHalo((1, 1, 1), LO, HI, periodic=True)
    lpos, lx = fresh.setup(p1, gid, R)
    g = radius_graph(lpos, R, *fresh.local_bounds(R))
    fresh.renumber(g.perm)
    fs = fresh.split_graph(g)
    return _global_pairs([(fs.graph.src, fs.graph.dst), fs.interior, fs.boundary], lx[g.perm.long()][:, 0].long(), M)


def test_world1_list_pairs_equal_a_fresh_build():
    """Positions and moves are multiples of 2^-10, so every d2 is exact in fp32 and the two sides test the same numbers.

    First cloud: every particle starts at least 9 / 1024 inside the box and moves at most 8 / 1024 per axis, so nobody
    crosses a periodic face: the three lists are those of a fresh build.  Second cloud: particles anywhere in the box.  One
    that crosses a face between two builds is CONTINUED by the list (its owned row leaves [lo, hi) and its images follow,
    ``Halo.update_positions``), whereas a fresh ``setup`` wraps it: a neighbour across that face then sees it as an owned
    src in one graph and as an image in the other.  The pair is the same, the list it lands in is not; there the kept
    pairs, and the union of interior and boundary, are compared."""
    M = 250
    rng = np.random.default_rng(62)
    move = torch.as_tensor((rng.integers(-8, 9, size=(M, 3)) / 1024.0).astype(f32))   # |move| <= 0.0136 < skin / 2
    gid = torch.arange(M, dtype=torch.float32)[:, None].to(DEV)
    for inside in (True, False):
        pos, _ = _cloud(M, 61, bits=10)
        if inside:
            pos = pos.clamp(9 / 1024.0, 1015 / 1024.0)
        halo = GridHalo((1, 1, 1), LO, HI, periodic=True)
        nl = ShardedNeighborList(R, SKIN, halo)
        nl.update(pos.to(DEV), gid)
        p1 = (pos + move).to(DEV)
        crossed = int(((p1 < 0) | (p1 >= 1)).any(1).sum())
        assert (crossed == 0) == inside                          # a condition on the inputs
        cloud = nl.update(p1, gid)
        assert nl.builds == 1 and not nl.rebuilt
        sp = cloud.split
        got = _global_pairs([(sp.graph.src, sp.graph.dst), sp.interior, sp.boundary], cloud.x[:, 0].long(), M)
        want = _fresh_pairs(p1, gid, M)
        assert got[0].numel() == want[0].numel() > 0 and torch.equal(got[0], want[0])
        assert nl.stored.graph.num_edges > sp.graph.num_edges    # the stored list at r + skin was cut down
        if inside:
            for name, a, b in zip(("interior", "boundary"), got[1:], want[1:]):
                assert a.numel() == b.numel() > 0 and torch.equal(a, b), name
        else:
            assert got[1].numel() > 0 and got[2].numel() > 0
            assert torch.equal(torch.sort(torch.cat(got[1:])).values, torch.sort(torch.cat(want[1:])).values)
        # the whole graph against the periodic radius graph of the cloud
        gp = radius_graph(p1, R, LO, HI, periodic=True)
        perm = gp.perm.long()
        assert torch.equal(got[0], torch.sort(perm[gp.dst.long()] * M + perm[gp.src.long()]).values)


# ---------------------------------------------------------------------------------------------------------------------
# 4: two ranks on one GPU
# ---------------------------------------------------------------------------------------------------------------------
STEPS = 3
OWED = {0: 2 * STEPS + 2, 1: STEPS + 2}


def _cloud2(M, seed):
    """Dyadic particles at least 0.03 away from the planes x = 0, 1 / 2, 1: three steps of 0.15 skin keep their owner."""
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, 1 << 16, size=(4 * M, 3)) / float(1 << 16)
    far = np.abs((pos[:, 0] + 0.25) % 0.5 - 0.25) >= 0.03
    pos = pos[far][:M].astype(f32)
    assert len(pos) == M
    return pos, rng.standard_normal((M, 4)).astype(f32)


def _worker(rank, world, periodic, q):
    import traceback
    try:
        _rank_body(rank, periodic, q)
    except Exception:
        for _ in range(OWED[rank]):
            q.put(("error", rank, traceback.format_exc()))


def _rank_body(rank, periodic, q):
    import torch.distributed as dist
    from oracle import segnn_oracle as S

    H, lmax, M = 8, 2, 300
    pos, x = _cloud2(M, 71)
    steps = _trajectory(pos, 72, steps=STEPS)
    ref, model = _pair(H, lmax, 73, envelope=6 if periodic else None)
    halo = GridHalo((2, 1, 1), LO, HI, periodic=periodic)
    own = (halo.owner_of(torch.as_tensor(pos)) == rank).nonzero().flatten()
    xd = torch.as_tensor(x)[own].to(DEV)
    nl = ShardedNeighborList(RM, SKIN, halo)
    for k, p in enumerate(steps):
        pd = torch.as_tensor(p)[own].to(DEV)
        with _quiet():
            e, f = model(xd, pd, RM, halo, forces=True, neighbors=nl)
        assert nl.builds == 1 and nl.rebuilt == (k == 0)
        q.put(("part", rank, k, own.numpy(), float(e), f.double().cpu().numpy()))
        if rank == 0 and periodic:
            with _quiet():
                e_ref, f_ref = ref(torch.as_tensor(x).to(DEV), torch.as_tensor(p).to(DEV), RM, LO, HI, periodic=True, forces=True)
            q.put(("ref", rank, k, None, float(e_ref), f_ref.double().cpu().numpy()))
        elif rank == 0:
            g = radius_graph(torch.as_tensor(p).to(DEV), RM, LO, HI)
            perm = g.perm.cpu().numpy()
            params = {n[len("net."):]: v.detach().cpu().numpy() for n, v in model.state_dict().items()}
            E64, F64, _ = S.energy_forces_torch(params, H, LAYERS, lmax, IN, x.astype(np.float64)[perm],
                                                p.astype(np.float64)[perm], g.rowptr.cpu().numpy(), g.src.cpu().numpy(),
                                                np.zeros(M, np.int64), 1)
            F = np.empty_like(F64)
            F[perm] = F64
            q.put(("ref", rank, k, None, float(E64[0]), F))
    # only a rank-1 particle exceeds skin / 2: both ranks rebuild
    pd = torch.as_tensor(steps[-1])[own].to(DEV)
    if rank == 1:
        pd[0, 1] += 0.75 * SKIN
    with _quiet():
        model(xd, pd, RM, halo, forces=True, neighbors=nl)
    q.put(("rebuilt", rank, nl.rebuilt, nl.builds))
    # a rank-0 particle has crossed into rank 1's box: every rank raises, nobody waits
    if rank == 0:
        pd[0, 0] = 0.75
    try:
        with _quiet():
            model(xd, pd, RM, halo, forces=True, neighbors=nl)
        q.put(("raised", rank, "nothing"))
    except OwnershipChanged:
        q.put(("raised", rank, "OwnershipChanged"))
    dist.barrier()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("periodic", [False, True])
def test_two_ranks_on_one_gpu(periodic):
    got = gloo_ranks.run(_worker, 2, (periodic,), OWED[0] + OWED[1], 240)
    assert not [g for g in got if g[0] == "error"], "\n".join(g[2] for g in got if g[0] == "error")
    e_tol, f_tol = (2e-5, 4e-5) if periodic else (1e-5, 2e-5)    # the bounds of tests/test_sharded_forces_gpu.py
    for k in range(STEPS):
        _, _, _, _, E_ref, F_ref = [g for g in got if g[0] == "ref" and g[2] == k][0]
        parts = [g for g in got if g[0] == "part" and g[2] == k]
        assert len(parts) == 2
        F = np.full_like(F_ref, np.nan)
        for _, _, _, own, e, f in parts:
            F[own] = f
            assert e == parts[0][4]                              # the all-reduced energy is the same number on both ranks
        assert not np.isnan(F).any(), "every particle must be owned by exactly one rank"
        e_err = abs(parts[0][4] - E_ref) / abs(E_ref)
        f_err = float(np.abs(F - F_ref).max() / np.abs(F_ref).max())
        print(f"\ntwo ranks with the list, periodic={periodic}, step {k}: energy {e_err:.2e}, forces {f_err:.2e}")
        assert e_err < e_tol and f_err < f_tol, (k, e_err, f_err)
    assert sorted(g[1:] for g in got if g[0] == "rebuilt") == [(0, True, 2), (1, True, 2)]
    assert sorted(g[1:] for g in got if g[0] == "raised") == [(0, "OwnershipChanged"), (1, "OwnershipChanged")]


# ---------------------------------------------------------------------------------------------------------------------
# 5: errors and state
# ---------------------------------------------------------------------------------------------------------------------
def test_errors_invalidate_foreign_setup_and_morton_halo():
    pos, x = _cloud(200, 81)
    pd, xd = pos.to(DEV), x.to(DEV)
    _, sh = _pair(8, 1, 82)
    _, plain = _pair(8, 1, 82, envelope=None)
    halo = GridHalo((1, 1, 1), LO, HI, periodic=True)
    nl = ShardedNeighborList(RM, SKIN, halo)
    with pytest.raises(ValueError, match="r = "):
        sh(xd, pd, 0.2, halo, neighbors=nl)
    with pytest.raises(ValueError, match="halo"):
        sh(xd, pd, RM, GridHalo((1, 1, 1), LO, HI, periodic=True), neighbors=nl)
    with pytest.raises(ValueError, match="skin"):
        sh(xd, pd, RM, halo, neighbors=nl, skin=SKIN)
    with pytest.raises(ValueError, match="skin"):
        plain(xd, pd, RM, halo, skin=SKIN)                       # a skin needs the envelope
    assert nl.updates == 0 and nl.builds == 0                    # all refused before the list was touched
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="fp32"):
            sh(xd.bfloat16(), pd, RM, halo)                      # bf16 keeps raising
        with pytest.raises(RuntimeError, match="fp32"):
            sh(xd.bfloat16(), pd, RM, halo, neighbors=nl)
        nl.invalidate()
        e0 = sh(xd, pd, RM, halo, neighbors=nl)
        builds = nl.builds
        assert nl.rebuilt
        e1 = sh(xd, pd, RM, halo, neighbors=nl)
        assert nl.builds == builds and not nl.rebuilt and e0.dim() == 0
        assert abs(float(e1) - float(e0)) < 1e-5 * max(1.0, abs(float(e0)))
        nl.invalidate()
        sh(xd, pd, RM, halo, neighbors=nl)
        assert nl.builds == builds + 1 and nl.rebuilt
        halo.setup(pd, xd, RM)                                   # a foreign setup: the list's index state is gone
        sh(xd, pd, RM, halo, neighbors=nl)
        assert nl.builds == builds + 2 and nl.rebuilt
        sh(xd, pd, RM, halo, neighbors=nl)
        assert nl.builds == builds + 2 and not nl.rebuilt
        # a MortonHalo builds and updates once
        mh = MortonHalo(MortonPartition(LO, HI, RM + SKIN, 1).fit(pd))
        ml = ShardedNeighborList(RM, SKIN, mh)
        e_m0 = plain(xd, pd, RM, mh, neighbors=ml)
        e_m1 = plain(xd, pd + 0.1 * SKIN, RM, mh, neighbors=ml)
        assert (ml.builds, ml.updates, ml.rebuilt) == (1, 2, False)
        e_open = plain(xd, pd + 0.1 * SKIN, RM, GridHalo((1, 1, 1), LO, HI))
        assert abs(float(e_m1) - float(e_open)) < 1e-5 * max(1.0, abs(float(e_open))) and e_m0.dim() == 0
    with pytest.raises(ValueError):
        ShardedNeighborList(RM, 0.0, halo)
    with pytest.raises(ValueError):
        ShardedNeighborList(RM, SKIN, halo).update(pd + 300.0 * SKIN, xd)     # beyond what the threshold's margin covers

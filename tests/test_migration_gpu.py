"""Particle migration on the GPU (include/e3gnn.h: e3_migrate_count / e3_migrate_fill; sharding.Halo.migrate;
ShardedNeighborList.redistribute).

  1. the kernel pair against ``migrate_rows_torch``, exactly, at the shapes where it branches: the wave and block edges of
     ``n``, 1 / 2 / 8 / 64 ranks, row widths below, at and above the lane-group sizes, this rank first and last, waves with one
     destination and with 64; invalid owners; the argument checks;
  2. world 1, device tensors: ``Halo.migrate`` returns its inputs;
  3. two ranks sharing cuda:0 over gloo: a four-step trajectory in which a handful of particles cross the plane between the
     ranks, against the whole cloud's reference at every step (the cases, references and bounds of
     tests/test_sharded_list_gpu.py)."""
import ctypes

import numpy as np
import pytest
import torch

import gloo_ranks
import models  # noqa: F401  (registers scalable_e3_gnn_amd -- also in the spawned ranks, which import this module)
from scalable_e3_gnn_amd import ShardedNeighborList, _lib
from scalable_e3_gnn_amd.radius_graph import radius_graph
from scalable_e3_gnn_amd.sharding import GridHalo, migrate_rows, migrate_rows_torch
from test_neighbor_list_gpu import _quiet, _trajectory
from test_sharded_list_gpu import IN, LAYERS, LO, HI, RM, SKIN, _cloud2, _pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
CANARY = -77


# ---------------------------------------------------------------------------------------------------------------------
# 1: the kernel pair
# ---------------------------------------------------------------------------------------------------------------------
def _entries(table, owner, rank, world, spare=3):
    """workspace query, count, the host read, fill -> (stay, send, the world + 1 counts); ``spare`` canary rows behind each
    output must come back untouched."""
    lib = _lib.load()
    n, W = table.shape
    stream = torch.cuda.current_stream().cuda_stream
    wbytes = int(lib.e3_migrate_workspace_bytes(n, world))
    assert wbytes > 0
    ws = torch.empty(wbytes, dtype=torch.uint8, device=DEV)
    counts = torch.full((world + 2,), CANARY, dtype=torch.int32, device=DEV)
    assert lib.e3_migrate_count(owner.data_ptr(), n, world, rank, counts.data_ptr(), ws.data_ptr(), wbytes, stream) == 0
    cnt = counts.tolist()
    assert cnt[world + 1] == CANARY
    cnt = cnt[:world + 1]
    n_stay, n_send = cnt[rank], sum(cnt[:world]) - cnt[rank]
    stay = torch.full((n_stay + spare, W), CANARY, dtype=torch.int32, device=DEV)
    send = torch.full((n_send + spare, W), CANARY, dtype=torch.int32, device=DEV)
    assert lib.e3_migrate_fill(table.data_ptr(), owner.data_ptr(), n, W, world, rank, (ctypes.c_int32 * (world + 1))(*cnt),
                               n_stay, n_send, stay.data_ptr(), send.data_ptr(), ws.data_ptr(), wbytes, stream) == 0
    assert bool((stay[n_stay:] == CANARY).all()) and bool((send[n_send:] == CANARY).all())
    return stay[:n_stay], send[:n_send], cnt


def _owners(pattern, n, world, rank, rng):
    others = [q for q in range(world) if q != rank] or [rank]
    i = np.arange(n)
    if pattern == "all stay":
        return np.full(n, rank)
    if pattern == "all to one":
        return np.full(n, others[len(others) // 2])
    if pattern == "none stay":
        return np.asarray(others)[i % len(others)]
    if pattern == "30 % leave":
        return np.where(rng.random(n) < 0.3, np.asarray(others)[rng.integers(0, len(others), n)], rank)
    return i % world                                             # "by index": every destination in every wave


def _check(n, world, W, rank, pattern, rng):
    owner = torch.as_tensor(_owners(pattern, n, world, rank, rng).astype(np.int32)).to(DEV)
    table = torch.as_tensor(rng.integers(-2 ** 31, 2 ** 31, size=(n, W), dtype=np.int64).astype(np.int32)).to(DEV)
    w_stay, w_send, w_counts, w_invalid = migrate_rows_torch(table.cpu(), owner.cpu(), rank, world)
    stay, send, cnt = _entries(table, owner, rank, world)
    where = (n, world, W, rank, pattern)
    assert cnt == w_counts.tolist() + [w_invalid], where
    assert torch.equal(stay.cpu(), w_stay) and torch.equal(send.cpu(), w_send), where
    # the host wrapper gives the restatement's four results
    got = migrate_rows(table, owner, rank, world)
    assert torch.equal(got[0].cpu(), w_stay) and torch.equal(got[1].cpu(), w_send), where
    assert torch.equal(got[2].cpu(), w_counts) and got[2].dtype == torch.int64 and got[3] == w_invalid == 0, where
    return cnt


PATTERNS = ("all stay", "all to one", "none stay", "30 % leave", "by index")
BASE = (257, 8, 17)
SWEEPS = ([(n, BASE[1], BASE[2]) for n in (0, 1, 63, 64, 65, 255, 256, 257, 513, 1000)] +
          [(BASE[0], p, BASE[2]) for p in (1, 2, 64)] + [(BASE[0], BASE[1], w) for w in (1, 3, 4, 40, 300)])


@pytest.mark.parametrize("n,world,W", SWEEPS)
def test_kernel_equals_the_restatement(n, world, W):
    rng = np.random.default_rng(n * 1000 + world * 10 + W)
    for rank in sorted({0, world - 1}):
        for pattern in PATTERNS:
            cnt = _check(n, world, W, rank, pattern, rng)
            if pattern == "by index" and world == 64:
                assert min(cnt[:64]) >= 4                        # a condition on the inputs: 64 destinations in every wave
            if pattern == "30 % leave" and n >= 255 and world > 1:
                assert 0 < cnt[rank] < n


def test_invalid_owners_are_counted_and_never_written():
    n, world, W = BASE
    rng = np.random.default_rng(9)
    for rank in (0, world - 1):
        own = _owners("30 % leave", n, world, rank, rng).astype(np.int32)
        own[0], own[64], own[n - 1] = -1, world, -(2 ** 31)
        own[65], own[130] = world + 1000, 2 ** 31 - 1
        owner = torch.as_tensor(own).to(DEV)
        table = torch.as_tensor(rng.integers(-2 ** 31, 2 ** 31, size=(n, W), dtype=np.int64).astype(np.int32)).to(DEV)
        w_stay, w_send, w_counts, w_invalid = migrate_rows_torch(table.cpu(), owner.cpu(), rank, world)
        stay, send, cnt = _entries(table, owner, rank, world)    # both entries return E3_OK
        assert w_invalid == 5 and cnt == w_counts.tolist() + [5]
        assert torch.equal(stay.cpu(), w_stay) and torch.equal(send.cpu(), w_send)
        assert stay.shape[0] + send.shape[0] == n - 5
        assert migrate_rows(table, owner, rank, world)[3] == 5


def test_argument_checks():
    lib = _lib.load()
    t = torch.zeros(256, dtype=torch.int32, device=DEV)
    p = t.data_ptr()
    ws = torch.zeros(int(lib.e3_migrate_workspace_bytes(5, 2)), dtype=torch.uint8, device=DEV)
    wp, wb = ws.data_ptr(), ws.numel()
    count, fill = lib.e3_migrate_count, lib.e3_migrate_fill
    host = lambda *v: (ctypes.c_int32 * len(v))(*v)            # noqa: E731
    ok_c = dict(owner=p, n=5, n_ranks=2, self_rank=0, counts=p, ws=wp, wb=wb, stream=None)
    ok_f = dict(table=p, owner=p, n=5, W=4, n_ranks=2, self_rank=0, counts=host(3, 2, 0), stay_rows=3, send_rows=2, stay=p,
                send=p, ws=wp, wb=wb, stream=None)
    # the base calls themselves are accepted (on buffers of their own: the refusals below must leave ``t`` untouched)
    owner = torch.tensor([0, 1, 0, 1, 0], dtype=torch.int32, device=DEV)
    table = torch.arange(20, dtype=torch.int32, device=DEV).reshape(5, 4)
    cnt, stay, send = torch.zeros(3, dtype=torch.int32, device=DEV), torch.zeros_like(table), torch.zeros_like(table)
    assert count(*{**ok_c, "owner": owner.data_ptr(), "counts": cnt.data_ptr()}.values()) == 0 and cnt.tolist() == [3, 2, 0]
    assert fill(*{**ok_f, "table": table.data_ptr(), "owner": owner.data_ptr(), "stay": stay.data_ptr(),
                  "send": send.data_ptr()}.values()) == 0
    assert torch.equal(stay[:3], table[0::2]) and torch.equal(send[:2], table[1::2])
    bad_both = [dict(n_ranks=0), dict(n_ranks=65), dict(self_rank=-1), dict(self_rank=2), dict(n=-1),
                dict(n=2 ** 30, n_ranks=2), dict(wb=15)]
    for bad in bad_both:
        assert count(*{**ok_c, **bad}.values()) == 1, bad
        assert fill(*{**ok_f, **bad}.values()) == 1, bad
    for bad in (dict(W=0), dict(W=4097), dict(n=2 ** 20, W=2048, n_ranks=1, counts=host(2 ** 20, 0), stay_rows=2 ** 20),
                dict(stay_rows=2), dict(send_rows=1), dict(counts=host(3, 1, 0)), dict(counts=host(3, 3, -1)),
                dict(counts=None), dict(stay=None), dict(send=None), dict(table=None), dict(owner=None), dict(ws=None)):
        assert fill(*{**ok_f, **bad}.values()) == 1, bad
    for bad in (dict(owner=None), dict(counts=None), dict(ws=None)):
        assert count(*{**ok_c, **bad}.values()) == 1, bad
    assert lib.e3_migrate_workspace_bytes(-1, 2) == -1 and lib.e3_migrate_workspace_bytes(5, 0) == -1
    assert lib.e3_migrate_workspace_bytes(5, 65) == -1 and lib.e3_migrate_workspace_bytes(2 ** 30, 2) == -1
    assert lib.e3_migrate_workspace_bytes(0, 1) > 0
    torch.cuda.synchronize()
    assert bool(torch.all(t == 0))                               # every refusal came before any launch
    # n = 0 is legal: the counts are zeroed, nothing is launched that reads owner
    c = torch.full((3,), CANARY, dtype=torch.int32, device=DEV)
    assert count(None, 0, 2, 1, c.data_ptr(), wp, wb, None) == 0 and c.tolist() == [0, 0, 0]
    assert fill(None, None, 0, 4, 2, 1, host(0, 0, 0), 0, 0, None, None, wp, wb, None) == 0


# ---------------------------------------------------------------------------------------------------------------------
# 2: world 1, device tensors
# ---------------------------------------------------------------------------------------------------------------------
def test_world1_migrate_on_device_returns_the_inputs():
    rng = np.random.default_rng(4)
    pos = torch.as_tensor((rng.random((300, 3)) * 5 - 2).astype(f32)).to(DEV)    # up to two box lengths outside
    x, vel, ids = torch.randn(300, 4, device=DEV), torch.randn(300, 3, device=DEV), torch.arange(300, device=DEV)
    halo = GridHalo((1, 1, 1), LO, HI, periodic=True)
    halo.setup(pos, x, RM)
    gen = halo.generation
    out = halo.migrate(pos, x, vel, ids)
    assert all(a is b for a, b in zip(out, (pos, x, vel, ids))) and len(out) == 4
    assert halo.generation == gen and halo.migrated == 0
    halo.update_positions(pos, x)                                # the setup state is still there
    nl = ShardedNeighborList(RM, SKIN, halo)
    out = nl.redistribute(pos, x, vel, ids)                      # no list yet: a migration that moves nobody
    assert all(a is b for a, b in zip(out, (pos, x, vel, ids))) and nl.migrations == 0
    nl.update(pos, x)
    out = nl.redistribute(pos, x, vel, ids)                      # the list holds
    assert all(a is b for a, b in zip(out, (pos, x, vel, ids)))
    nl.update(pos, x)
    assert (nl.builds, nl.updates, nl.rebuilt, nl.migrations) == (1, 2, False, 0)
    bad = pos.clone()
    bad[11, 0] = float("nan")
    with pytest.raises(ValueError, match="no owner"):
        halo.migrate(bad, x, vel, ids)


# ---------------------------------------------------------------------------------------------------------------------
# 3: two ranks on one GPU, a trajectory through a crossing
# ---------------------------------------------------------------------------------------------------------------------
STEPS = 4
CROSS = 5
OWED = {0: 2 * STEPS + 1, 1: STEPS + 1}


def _steps():
    """The cloud and trajectory of tests/test_sharded_list_gpu.py (nobody else comes within 0.0075 of a plane); from step 2
    on the CROSS particles of rank 0 nearest to the plane x = 1 / 2 are 0.1 further along x: more than skin / 2 inside
    rank 1's box, where the steps of 0.15 skin keep them."""
    pos, x = _cloud2(300, 71)
    steps = _trajectory(pos, 72, steps=STEPS)
    left = np.where(pos[:, 0] < 0.5)[0]
    cross = left[np.argsort(pos[left, 0])[-CROSS:]]
    for k in (2, 3):
        steps[k][cross, 0] += f32(0.1)
    assert all((p[cross, 0] > 0.5 + 0.5 * SKIN).all() for p in steps[2:]) and (steps[1][cross, 0] < 0.5).all()
    assert all((p[cross, 0] < 1.0 - SKIN).all() for p in steps)
    return steps, x, cross


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
    steps, x, cross = _steps()
    ref, model = _pair(H, lmax, 73, envelope=6 if periodic else None)
    halo = GridHalo((2, 1, 1), LO, HI, periodic=periodic)
    ids = (halo.owner_of(torch.as_tensor(steps[0])) == rank).nonzero().flatten().to(DEV)
    xd = torch.as_tensor(x).to(DEV)[ids]
    nl = ShardedNeighborList(RM, SKIN, halo)
    log = []
    for k, p in enumerate(steps):
        pd = torch.as_tensor(p).to(DEV)[ids]
        before = (pd, xd, ids)
        pd, xd, ids = nl.redistribute(pd, xd, ids)
        with _quiet():
            e, f = model(xd, pd, RM, halo, forces=True, neighbors=nl)
        log.append((nl.builds, nl.rebuilt, nl.migrations, nl.migrated, int(pd.shape[0]),
                    pd is before[0] and xd is before[1] and ids is before[2]))
        q.put(("part", rank, k, ids.cpu().numpy(), float(e), f.double().cpu().numpy()))
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
    q.put(("log", rank, log, sorted(ids.tolist()), sorted(cross.tolist())))
    dist.barrier()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("periodic", [True, False])
def test_two_ranks_on_one_gpu_through_a_crossing(periodic):
    got = gloo_ranks.run(_worker, 2, (periodic,), OWED[0] + OWED[1], 240)
    assert not [g for g in got if g[0] == "error"], "\n".join(g[2] for g in got if g[0] == "error")
    e_tol, f_tol = (2e-5, 4e-5) if periodic else (1e-5, 2e-5)    # the bounds of tests/test_sharded_forces_gpu.py
    for k in range(STEPS):
        _, _, _, _, E_ref, F_ref = [g for g in got if g[0] == "ref" and g[2] == k][0]
        parts = [g for g in got if g[0] == "part" and g[2] == k]
        assert len(parts) == 2
        F = np.full_like(F_ref, np.nan)
        for _, _, _, own, e, f in parts:
            assert np.isnan(F[own]).all()                        # nobody is owned twice
            F[own] = f
            assert e == parts[0][4]                              # the all-reduced energy is the same number on both ranks
        assert not np.isnan(F).any(), "every particle must be owned by exactly one rank"
        e_err = abs(parts[0][4] - E_ref) / abs(E_ref)
        f_err = float(np.abs(F - F_ref).max() / np.abs(F_ref).max())
        print(f"\ntwo ranks through a crossing, periodic={periodic}, step {k}: energy {e_err:.2e}, forces {f_err:.2e}")
        assert e_err < e_tol and f_err < f_tol, (k, e_err, f_err)
    logs = {g[1]: g for g in got if g[0] == "log"}
    n0 = {r: logs[r][2][0][4] for r in (0, 1)}
    for r in (0, 1):
        log = logs[r][2]
        # (builds, rebuilt, migrations, migrated) per step: one rebuild, through one migration of CROSS particles
        assert [s[:4] for s in log] == [(1, True, 0, 0), (1, False, 0, 0), (2, True, 1, CROSS), (2, False, 1, CROSS)], log
        assert [s[4] - n0[r] for s in log] == [0, 0, (-CROSS, CROSS)[r], (-CROSS, CROSS)[r]]
        assert [s[5] for s in log] == [True, True, False, True]  # nobody moved, or the list held: the inputs themselves
    assert set(logs[0][4]) <= set(logs[1][3]) and not set(logs[0][4]) & set(logs[0][3])     # the crossers live on rank 1 now

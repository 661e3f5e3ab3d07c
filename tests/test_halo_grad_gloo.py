"""gloo tests (worlds 2 and 4, CPU tensors) of the differentiable ghost refresh: ``Halo.refresh`` (an autograd node whose
backward sends ghost-row gradients back to their owners), ``Halo.reduce_ghosts`` and ``sharding.all_reduce_grads``, on their
torch restatements (the HIP kernels are compared with those bit for bit in tests/test_halo_grad_gpu.py).

A toy message-passing net written here, in fp64, runs per rank on the split graph of the local cloud,

    d_e = |p_src - p_dst|;   per layer:  h <- halo.refresh(h);   h <- h + sum_{e -> i} tanh([h_dst | h_src | d_e] W)

with the energy a fixed linear form of the owned rows.  Merged over the ranks, the energy, dE/dx, dE/dpos (through
``reduce_ghosts``) and dE/dW (after ``all_reduce_grads``) must equal those of the same net on the whole cloud within 1e-10
relative (two fp64 computations in a different summation order; the bound of tests/test_sharding_gloo.py).  Positions lie on
the 1/256 grid, so every pair's squared distance is exact in fp32 and the sharded and the whole-cloud edge sets are equal.
One world-4 case has a rank that owns nothing but holds ghosts: its backward must still answer its peer (the run would
otherwise end at the timeout)."""
import numpy as np
import pytest
import torch
import torch.distributed as dist

import gloo_ranks

R = 0.3
F = 3
COEF = (1.0, -0.5, 0.25)


def _cloud(layout, world):
    """-> (pos [N,3] fp32 on the 1/256 grid, no point twice; x [N,F] fp64; lo, hi)."""
    rng = np.random.default_rng(5)
    if layout == "gap":
        # 4 slabs along x over [0, 4): rank 1 holds particles only in the middle of its slab, rank 2 owns NOTHING but gets
        # ghosts from rank 3 (tests/test_sharding_gloo.py's "gap" cloud on a dyadic grid)
        n = 360
        u = rng.random(n)
        xs = np.where(u < 0.5, 0.9 * u / 0.5, np.where(u < 0.6, 1.4 + 0.2 * (u - 0.5) / 0.1, 3.0 + (u - 0.6) / 0.4))
        pos = np.stack([np.floor(xs * 256) / 256, rng.integers(0, 256, n) / 256, rng.integers(0, 256, n) / 256], 1)
        lo, hi = [0.0, 0.0, 0.0], [4.0, 1.0, 1.0]
    else:
        pos = rng.integers(0, 256, size=(260, 3)) / 256.0
        lo, hi = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
    pos = np.unique(pos, axis=0)
    pos = pos[rng.permutation(len(pos))]
    x = rng.standard_normal((len(pos), F))
    return torch.as_tensor(pos, dtype=torch.float32), torch.as_tensor(x), lo, hi


class _Toy(torch.nn.Module):
    def __init__(self, layers):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.W = torch.nn.ParameterList([torch.nn.Parameter(0.4 * torch.randn(2 * F + 1, F, generator=g, dtype=torch.float64))
                                         for _ in range(layers)])

    def forward(self, h, rel, src, dst, refresh):
        d = rel.norm(dim=1, keepdim=True)
        for W in self.W:
            h = refresh(h)
            m = torch.tanh(torch.cat([h[dst], h[src], d], 1) @ W)
            h = h + torch.zeros_like(h).index_add(0, dst, m)
        return h


def _energy(h_owned):
    return (h_owned * torch.tensor(COEF, dtype=torch.float64)).sum()


def _reference(pos, x, lo, hi, periodic, layers):
    """The toy net on the whole cloud: all ordered pairs within R (minimum image on periodic axes) -> E, dE/dx, dE/dpos,
    [dE/dW]."""
    p = pos.double().requires_grad_(True)
    xx = x.clone().requires_grad_(True)
    L = torch.tensor([hi[a] - lo[a] if periodic else 0.0 for a in range(3)], dtype=torch.float64)

    def rel_of(a, b):
        v = a - b
        return v - L * torch.round(v / L) if periodic else v

    with torch.no_grad():
        d2 = rel_of(p[None, :, :], p[:, None, :]).square().sum(-1)
        d2.fill_diagonal_(9.0)
        dst, src = (d2 <= np.float32(R) * np.float32(R)).nonzero(as_tuple=True)
    toy = _Toy(layers)
    E = _energy(toy(xx, rel_of(p[src], p[dst]), src, dst, lambda h: h))
    E.backward()
    return float(E.detach()), xx.grad.numpy(), p.grad.numpy(), [W.grad.numpy() for W in toy.W], int(src.numel())


def _worker(rank, world, layout, layers, q):
    import models  # noqa
    from oracle import graph_oracle as G
    from scalable_e3_gnn_amd.radius_graph import RadiusGraph
    from scalable_e3_gnn_amd.sharding import GridHalo, MortonHalo, MortonPartition, all_reduce_grads, all_reduce_sum

    pos, x, lo, hi = _cloud(layout, world)
    periodic = layout == "periodic"
    if layout == "morton":
        part = MortonPartition(lo, hi, R, world).fit(pos[rank::world])
        halo = MortonHalo(part)
    else:
        dims = {"gap": (4, 1, 1), 2: (2, 1, 1), 4: (2, 2, 1)}["gap" if layout == "gap" else world]
        halo = GridHalo(dims, lo, hi, periodic=periodic)
    own = (halo.owner_of(pos) == rank).nonzero().flatten()
    lpos, lx = halo.setup(pos[own], x[own], R)
    blo, bhi = halo.local_bounds(R)
    nloc = lpos.shape[0]
    if nloc:
        perm, rowptr, src = G.graph(lpos.double().numpy(), blo, bhi, R)
    else:
        perm, rowptr, src = np.zeros(0, np.int32), np.zeros(1, np.int32), np.zeros(0, np.int32)
    halo.renumber(torch.as_tensor(perm))
    g = RadiusGraph(torch.as_tensor(perm), torch.zeros(nloc, 4), torch.as_tensor(rowptr), torch.as_tensor(src), len(src),
                    ((1, 1, 1), 0))
    sp = halo.split_graph(g)
    es, ed = sp.graph.src.long(), sp.graph.dst.long()
    pidx = torch.as_tensor(perm).long()
    xl = lx[pidx].clone().requires_grad_(True)
    pl = lpos[pidx].double().requires_grad_(True)
    toy = _Toy(layers)
    h = toy(xl, pl[es] - pl[ed], es, ed, halo.refresh)
    E = _energy(h[halo.owned_new])
    # three backward passes; every one runs the reverse exchange of every refresh on every rank (halo.anchor among the
    # inputs: the first refresh does not depend on the positions, and rank 2 of the "gap" cloud owns no row at all)
    gx, _ = torch.autograd.grad(E, [xl, halo.anchor], retain_graph=True)
    gp, _ = torch.autograd.grad(E, [pl, halo.anchor], retain_graph=True)
    assert not gx[halo.is_ghost].any()                        # the refresh never reads the stale ghost rows
    gpos = halo.reduce_ghosts(gp)
    E.backward()
    all_reduce_grads(toy, halo.group)
    E_tot = all_reduce_sum(E.detach().reshape(1), halo.group)
    q.put(("part", rank, own.numpy(), gx[halo.owned_new].numpy(), gpos.numpy(), int(es.numel()), halo.n_ghost,
           max(halo.send_counts, default=0)))
    if rank == 0:
        q.put(("total", float(E_tot), [W.grad.numpy() for W in toy.W]))
        q.put(("ref",) + _reference(pos, x, lo, hi, periodic, layers))
    dist.barrier()


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


CASES = [("open", 2, 3), ("periodic", 2, 2), ("morton", 2, 2), ("gap", 4, 2), ("periodic", 4, 2), ("morton", 4, 3)]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("layout,world,layers", CASES)
def test_sharded_gradients_equal_whole_cloud(layout, world, layers):
    got = gloo_ranks.run(_worker, world, (layout, layers), world + 2, 280)
    _, E_ref, gx_ref, gp_ref, gW_ref, n_edges = [g for g in got if g[0] == "ref"][0]
    _, E_tot, gW = [g for g in got if g[0] == "total"][0]
    parts = {g[1]: g for g in got if g[0] == "part"}
    gx, gp = np.full_like(gx_ref, np.nan), np.full_like(gp_ref, np.nan)
    for _, rank, own, gx_r, gp_r, _, _, _ in parts.values():
        gx[own], gp[own] = gx_r, gp_r
    assert not np.isnan(gx).any() and not np.isnan(gp).any(), "every particle must be owned by exactly one rank"
    assert sum(p[5] for p in parts.values()) == n_edges      # every edge of the whole cloud on exactly one rank
    assert sum(p[6] for p in parts.values()) > 0              # ghosts exist: the gradients do cross ranks
    errs = {"E": abs(E_tot - E_ref) / abs(E_ref), "dE/dx": _rel(gx, gx_ref), "dE/dpos": _rel(gp, gp_ref),
            "dE/dW": max(_rel(a, b) for a, b in zip(gW, gW_ref))}
    print(f"\n{layout} world {world}, {layers} layers, N={len(gx_ref)}, E={n_edges}: " +
          ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert all(v < 1e-10 for v in errs.values()), errs
    if layout == "gap":
        assert len(parts[2][2]) == 0 and parts[2][6] > 0     # rank 2 owns nothing and holds ghosts

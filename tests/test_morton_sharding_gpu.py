"""Two ranks share cuda:0 (gloo transport, host-staged halo) and run the real kernels on a NON-UNIFORM cloud cut into
equal-count Morton key ranges: ``MortonPartition.fit`` over the group (``e3_morton_keys``), ``MortonHalo.setup`` (the HIP
selection ``e3_morton_select_*``), then the sharded SEGNN forward -- overlapped on the split graph and blocking on the unsplit
one -- must match the single-process forward over the whole cloud and, for the small l_max = 2 case, the numpy fp64 oracle.
Tolerances are those of tests/test_sharding_gpu.py for the same comparisons."""
import numpy as np
import pytest
import torch

import gloo_ranks

pytestmark = pytest.mark.gpu


def _cloud(N):
    """Box [0,2) x [0,1)^2, 60 % of x drawn from 1.45 + 0.18 randn, clamped to [0, 2 - 2^-20]."""
    g0 = torch.Generator().manual_seed(11)
    pos = torch.rand(N, 3, generator=g0)
    pos[:, 0] *= 2.0
    blob = torch.rand(N, generator=g0) < 0.6
    pos[:, 0] = torch.where(blob, 1.45 + 0.18 * torch.randn(N, generator=g0), pos[:, 0])
    pos[:, 0].clamp_(0.0, 2.0 - 2.0 ** -20)
    x = torch.randn(N, 4, generator=g0)
    return pos, x


def _worker(rank, world, N, H, L, lmax, q):
    import torch.distributed as dist
    import models  # noqa
    from scalable_e3_gnn_amd.radius_graph import radius_graph
    from scalable_e3_gnn_amd.segnn import SEGNN
    from scalable_e3_gnn_amd.sharding import MortonHalo, MortonPartition

    dev = "cuda:0"
    pos, x = _cloud(N)
    lo, hi = [0.0, 0.0, 0.0], [2.0, 1.0, 1.0]
    r = float((3 * 16.0 / (4 * np.pi * (N / world))) ** (1 / 3))
    torch.manual_seed(0)
    model = SEGNN("1x0e+1x1o", H, "1x1o", L, lmax=lmax).to(dev)
    part = MortonPartition(lo, hi, r, world).fit(pos[rank::world].to(dev))     # keys on the GPU, histogram summed over gloo
    own = (part.owner_of(pos) == rank).nonzero().flatten()
    assert own.numel() == part.counts[rank]
    halo = MortonHalo(part)
    lpos, lx = halo.setup(pos[own].to(dev), x[own].to(dev), r)
    assert halo.n_ghost > 0 and halo.neighbours == [1 - rank]
    blo, bhi = halo.local_bounds(r)
    g = radius_graph(lpos, r, blo, bhi)
    halo.renumber(g.perm)
    split = halo.split_graph(g)
    with torch.no_grad():
        out = model(lx[g.perm.long()], g, halo=halo, split=split)   # overlapped refresh, interior / boundary edges
        out_b = model(lx[g.perm.long()], g, halo=halo)              # blocking refresh on the unsplit graph
    o, ob = out[halo.owned_new], out_b[halo.owned_new]
    assert float((o - ob).abs().max() / ob.abs().max()) < 2e-5
    slab = int((pos[:, 0].floor().long().clamp_(0, 1) == rank).sum())
    q.put(("part", o.cpu().numpy(), own.numpy()))
    q.put(("own", (own.numel(), slab, part.hist_max, halo.n_ghost), rank))
    if rank == 0:
        gg = radius_graph(pos.to(dev), r, lo, hi)
        with torch.no_grad():
            full = model(x.to(dev)[gg.perm.long()], gg)
        ref = torch.empty_like(full)
        ref[gg.perm.long()] = full
        q.put(("ref", ref.cpu().numpy(), None))
        if lmax == 2 and N <= 8000:   # an independent reference too: the fp64 oracle of the unsharded cloud
            from oracle import segnn_oracle as S
            params = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
            perm = gg.perm.cpu().numpy()
            want = S.forward_l2(params, H, L, "1x0e+1x1o", "1x1o", x.double().numpy()[perm], pos.numpy()[perm],
                                gg.rowptr.cpu().numpy(), gg.src.cpu().numpy())
            o64 = np.empty_like(want)
            o64[perm] = want
            q.put(("oracle", o64, None))
    dist.barrier()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("H,lmax,N", [(16, 1, 20000), (32, 2, 20000), (32, 2, 6000)])
def test_morton_sharded_gpu_forward_equals_single_process(H, lmax, N):
    world, L = 2, 3
    oracle = lmax == 2 and N <= 8000
    got = gloo_ranks.run(_worker, world, (N, H, L, lmax), 2 * world + 1 + (1 if oracle else 0), 240)
    ref = [g for g in got if g[0] == "ref"][0][1]
    merged = np.full_like(ref, np.nan)
    for tag, val, idx in got:
        if tag == "part":
            merged[idx] = val
    assert not np.isnan(merged).any()
    err = np.abs(merged - ref).max() / np.abs(ref).max()
    owned = dict((rank, val) for tag, val, rank in got if tag == "own")
    print(f"\nN={N}: owned per rank: slabs {[owned[k][1] for k in range(world)]}  Morton ranges "
          f"{[owned[k][0] for k in range(world)]} (fullest cell {owned[0][2]}, ghosts {[owned[k][3] for k in range(world)]}); "
          f"sharded vs single-process forward {err:.2e}")
    assert err < 2e-5                                              # fp32, different summation order per row
    assert sum(owned[k][0] for k in range(world)) == N
    for k in range(world):
        assert abs(owned[k][0] - N / world) < owned[k][2]          # the balance guarantee
    assert any(tag == "oracle" for tag, _, _ in got) == oracle
    for tag, val, _ in got:
        if tag == "oracle":
            e64 = np.abs(merged - val).max() / np.abs(val).max()
            print(f"sharded HIP forward (2 Morton ranges) vs fp64 oracle of the whole cloud: {e64:.2e}")
            assert e64 < 1e-5, e64

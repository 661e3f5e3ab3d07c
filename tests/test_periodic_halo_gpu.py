"""Periodic spatial sharding with the real kernels: the HIP image selection (csrc/e3_halo.hip) bit for bit against its torch
restatement, the world-1 self-halo (all 26 entries served by local copies) against the periodic graph and forward of the
whole cloud, and two ranks sharing cuda:0 over gloo against the single-process periodic forward and the fp64 oracle of the
tiled cloud.  Tolerances: 2e-5 between fp32 forwards (different summation order per row), 1e-5 against the fp64 oracle
(as tests/test_periodic_gpu.py), 2e-2 between bf16-storage forwards (one bf16 rounding of differently ordered sums)."""
import itertools

import numpy as np
import pytest
import torch

import gloo_ranks
import models  # noqa: F401  (registers scalable_e3_gnn_amd -- also in the spawned ranks, which import this module)
import pbc_reference as P
from scalable_e3_gnn_amd import _lib
from scalable_e3_gnn_amd.sharding import GridHalo, select_images, select_images_torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OFFS = list(itertools.product((-1, 0, 1), repeat=3))


def _dyadic(n, seed):
    return (np.random.default_rng(seed).integers(0, 1 << 16, size=(n, 3)) / float(1 << 16)).astype(np.float32)


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ---------------------------------------------------------------------------------------------------------------------
# 4. HIP selection == torch restatement, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def _geometries():
    lo, hi = (0.25, -1.0, 0.0), (1.5, 0.75, 2.0)
    out = []
    for per, r in ((True, 0.11), ((True, False, True), 0.2), ((False, True, False), 0.3)):
        h = GridHalo((1, 1, 1), lo, hi, periodic=per)
        out.append((lo, hi, per, r, h._selection(r)))
    # hand-made entries: one that nothing falls into, one that takes everything, a shift that is not a period
    sel = [([5.0, 5.0, 5.0], [6.0, 6.0, 6.0], [0.0, 0.0, 0.0]),
           ([-1e30] * 3, [1e30] * 3, [0.125, -0.3, 7.0]),
           ([0.3, -0.5, 0.1], [0.9, 0.0, 1.7], [-1.25, 0.0, 2.0])]
    out.append((lo, hi, (True, True, False), 0.05, sel))
    return out


@pytest.mark.parametrize("n", [0, 1, 63, 5000, 70001])
@pytest.mark.parametrize("case", range(4))
def test_hip_selection_equals_torch(n, case):
    lo, hi, per, r, sel = _geometries()[case]
    rng = np.random.default_rng(n + case)
    pos = (rng.random((n, 3)) * 4.0 - 1.5).astype(np.float32)   # non-dyadic, many points outside the box
    pt = torch.as_tensor(pos).to(DEV)
    pw, idx, cnt, gp = select_images(pt, lo, hi, per, r, sel)
    pw2, idx2, cnt2, gp2 = select_images_torch(pt, lo, hi, per, r, sel)
    assert cnt == cnt2 and len(cnt) == len(sel)
    assert torch.equal(idx, idx2) and idx.dtype == torch.long
    assert torch.equal(pw, pw2) and torch.equal(gp, gp2)
    # the wrap is the graph builder's (tests/pbc_reference.py restates it bit for bit)
    assert np.array_equal(pw.cpu().numpy(), P.wrap(pos, lo, hi, per))
    if case == 3 and n:
        assert cnt[0] == 0 and cnt[1] == n


def test_hip_selection_rejects_bad_arguments():
    lib = _lib.load()
    E = (_lib.HaloEntry * 27)()
    pos = torch.zeros((8, 3), device=DEV)
    out = torch.zeros((8, 3), device=DEV)
    counts = torch.zeros(27, dtype=torch.int32, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    F3 = _lib.Float3

    def call(lo=(0, 0, 0), hi=(1, 1, 1), per=7, r=0.1, ne=2):
        return lib.e3_halo_select_count(pos.data_ptr(), 8, F3(*lo), F3(*hi), per, r, E, ne, out.data_ptr(),
                                        counts.data_ptr(), ws.data_ptr(), ws.numel(), s)

    assert call() == 0
    assert call(ne=27) == 1 and call(ne=-1) == 1
    assert call(per=8) == 1 and call(per=-1) == 1
    assert call(r=0.5) == 1 and call(r=0.6) == 1 and call(per=6, r=0.5) == 1
    assert call(per=0, r=0.6) == 0                               # 2 r >= L only matters on a periodic axis
    assert call(lo=(0, float("nan"), 0)) == 1 and call(hi=(1, float("inf"), 1)) == 1 and call(hi=(1, 0, 1)) == 1
    assert lib.e3_halo_select_workspace_bytes(8, 27) == -1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 5. world-1 self-halo == the periodic graph and forward of the whole cloud
# ---------------------------------------------------------------------------------------------------------------------
def _self_halo_run(model, pos, x, r, dtype):
    """-> (owned outputs split / blocking [N, out] in original order, owned edge set in global ids)"""
    from scalable_e3_gnn_amd.radius_graph import radius_graph
    N = len(pos)
    halo = GridHalo((1, 1, 1), (0, 0, 0), (1, 1, 1), periodic=True)
    feats = torch.cat([torch.as_tensor(x), torch.arange(N, dtype=torch.float32)[:, None]], 1).to(DEV)
    lpos, lf = halo.setup(torch.as_tensor(pos).to(DEV), feats, r)
    assert halo.neighbours == [] and len(halo.images) == 26
    g = radius_graph(lpos, r, [-2 * r] * 3, [1 + 2 * r] * 3)
    assert g.box is None
    halo.renumber(g.perm)
    split = halo.split_graph(g)
    xs = lf[g.perm.long(), :4].to(dtype)
    with torch.no_grad():
        o_split = model(xs, g, halo=halo, split=split)[halo.owned_new]
        o_block = model(xs, g, halo=halo)[halo.owned_new]
    gid = lf[g.perm.long(), 4].long().cpu().numpy()
    rowptr, src = g.rowptr.cpu().numpy(), g.src.cpu().numpy()
    dst = np.repeat(np.arange(len(gid)), np.diff(rowptr))
    keep = ~halo.is_ghost.cpu().numpy()[dst]
    edges = np.unique(gid[dst[keep]] * N + gid[src[keep]])
    assert len(edges) == int(keep.sum())                         # no pair twice
    return (o_split.float().double().cpu().numpy(), o_block.float().double().cpu().numpy(), edges, halo.ghost_fraction())


def _whole_cloud(model, pos, x, r, dtype):
    from scalable_e3_gnn_amd.radius_graph import radius_graph
    N = len(pos)
    gg = radius_graph(torch.as_tensor(pos).to(DEV), r, [0, 0, 0], [1, 1, 1], periodic=True)
    perm = gg.perm.long()
    with torch.no_grad():
        out = model(torch.as_tensor(x).to(DEV)[perm].to(dtype), gg)
    back = torch.empty_like(out)
    back[perm] = out
    p = gg.perm.cpu().numpy().astype(np.int64)
    dst = p[np.repeat(np.arange(N), np.diff(gg.rowptr.cpu().numpy()))]
    edges = np.unique(dst * N + p[gg.src.cpu().numpy()])
    return back.float().double().cpu().numpy(), edges


@pytest.mark.parametrize("lmax,H,dtype", [(1, 16, torch.float32), (2, 32, torch.float32), (2, 32, torch.bfloat16)])
def test_world1_self_halo_equals_periodic_forward(lmax, H, dtype):
    from scalable_e3_gnn_amd.segnn import SEGNN
    N, layers = 20000, 3
    r = float((3 * 16.0 / (4 * np.pi * N)) ** (1 / 3))
    pos = _dyadic(N, 31)
    pos[:500] += np.float32(1.0)                                 # outside the box on every axis: wrapped by setup
    x = np.random.default_rng(32).standard_normal((N, 4)).astype(np.float32)
    torch.manual_seed(33)
    model = SEGNN("1x0e+1x1o", H, "1x1o", layers, lmax=lmax).to(DEV)
    if dtype == torch.bfloat16:
        model = model.bfloat16()
        x = torch.as_tensor(x).bfloat16().float().numpy()
    o_split, o_block, edges, frac = _self_halo_run(model, pos, x, r, dtype)
    want, want_edges = _whole_cloud(model, pos, x, r, dtype)
    assert np.array_equal(edges, want_edges)
    tol = 2e-5 if dtype == torch.float32 else 2e-2
    print(f"\nworld-1 self-halo N={N} r={r:.4f}: ghosts/owned {frac:.3f}; split {_rel(o_split, want):.2e}, "
          f"blocking {_rel(o_block, want):.2e} vs the whole-cloud periodic forward")
    assert _rel(o_split, want) < tol and _rel(o_block, want) < tol


def _tiled_oracle(params, H, layers, pos, x, r, periodic):
    """fp64 oracle: the centre copy of the cloud tiled by its images on the periodic axes, as an open cloud."""
    from oracle import graph_oracle as G
    from oracle import segnn_oracle as S
    ax = P.axes_of(periodic)
    w = P.wrap(pos, [0] * 3, [1] * 3, periodic).astype(np.float64)
    offs = [o for o in OFFS if all(o[a] == 0 or ax[a] for a in range(3))]
    tiled = np.concatenate([w + np.asarray(o, np.float64) for o in offs], 0).astype(np.float32)
    c, M = offs.index((0, 0, 0)), len(pos)
    perm, rowptr, src = G.graph(tiled, [-1.0] * 3, [2.0] * 3, r)
    out = S.forward_l2(params, H, layers, "1x0e+1x1o", "1x1o", np.tile(x, (len(offs), 1)).astype(np.float64)[perm],
                       tiled[perm].astype(np.float64), rowptr, src)
    back = np.empty_like(out)
    back[perm] = out
    return back[c * M:(c + 1) * M]


def test_world1_self_halo_vs_27_image_oracle():
    from scalable_e3_gnn_amd.segnn import SEGNN
    M, H, layers = 200, 32, 2
    r = 1.0 / (layers + 2.2)
    pos = _dyadic(M, 34)
    x = np.random.default_rng(35).standard_normal((M, 4)).astype(np.float32)
    torch.manual_seed(36)
    model = SEGNN("1x0e+1x1o", H, "1x1o", layers, lmax=2).to(DEV)
    o_split, o_block, _, _ = _self_halo_run(model, pos, x, r, torch.float32)
    params = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    want = _tiled_oracle(params, H, layers, pos, x, r, True)
    assert _rel(o_split, want) < 1e-5 and _rel(o_block, want) < 1e-5, (_rel(o_split, want), _rel(o_block, want))


# ---------------------------------------------------------------------------------------------------------------------
# 6. two ranks on cuda:0 over gloo, dims (2, 1, 1)
# ---------------------------------------------------------------------------------------------------------------------
def _worker(rank, world, periodic, M, H, layers, q):
    import torch.distributed as dist
    from scalable_e3_gnn_amd.radius_graph import radius_graph
    from scalable_e3_gnn_amd.segnn import SEGNN

    r = 1.0 / (layers + 2.2)
    pos = _dyadic(M, 41)
    x = np.random.default_rng(42).standard_normal((M, 4)).astype(np.float32)
    torch.manual_seed(43)
    model = SEGNN("1x0e+1x1o", H, "1x1o", layers, lmax=2).to(DEV)
    halo = GridHalo((2, 1, 1), (0, 0, 0), (1, 1, 1), periodic=periodic)
    own = (halo.owner_of(torch.as_tensor(pos)) == rank).nonzero().flatten()
    lpos, lx = halo.setup(torch.as_tensor(pos)[own].to(DEV), torch.as_tensor(x)[own].to(DEV), r)
    blo, bhi = halo.box(rank)
    g = radius_graph(lpos, r, [v - 2 * r for v in blo], [v + 2 * r for v in bhi])
    halo.renumber(g.perm)
    split = halo.split_graph(g)
    with torch.no_grad():
        o = model(lx[g.perm.long()], g, halo=halo, split=split)[halo.owned_new]
        ob = model(lx[g.perm.long()], g, halo=halo)[halo.owned_new]
    assert float((o - ob).abs().max() / ob.abs().max()) < 2e-5
    q.put(("part", o.double().cpu().numpy(), own.numpy(), len(halo.neighbours), len(halo.images)))
    if rank == 0:
        gg = radius_graph(torch.as_tensor(pos).to(DEV), r, [0, 0, 0], [1, 1, 1], periodic=periodic)
        with torch.no_grad():
            full = model(torch.as_tensor(x).to(DEV)[gg.perm.long()], gg)
        ref = torch.empty_like(full)
        ref[gg.perm.long()] = full
        q.put(("ref", ref.double().cpu().numpy(), None, 0, 0))
        params = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
        q.put(("oracle", _tiled_oracle(params, H, layers, pos, x, r, periodic), None, 0, 0))
    dist.barrier()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("periodic", [True, (True, True, False)])
def test_two_ranks_on_one_gpu(periodic):
    world, M, H, layers = 2, 300, 32, 2
    got = gloo_ranks.run(_worker, world, (periodic, M, H, layers), world + 2, 240)
    ref = [g for g in got if g[0] == "ref"][0][1]
    oracle = [g for g in got if g[0] == "oracle"][0][1]
    merged = np.full_like(ref, np.nan)
    for tag, val, idx, nn, ne in got:
        if tag == "part":
            merged[idx] = val
            assert nn == 1 and ne == (26 if periodic is True else 8)
    assert not np.isnan(merged).any()
    assert _rel(merged, ref) < 2e-5, _rel(merged, ref)
    assert _rel(merged, oracle) < 1e-5, _rel(merged, oracle)

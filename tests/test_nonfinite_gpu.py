"""Non-finite row isolation: NaN or inf in chosen FEATURE rows must stay in the rows the math sends it to, and every other
row must stay finite and as accurate as without it.  Every case compares with the fp64 oracles the suite already uses
(oracle/tp_oracle.py, oracle/l1tp_oracle.py, segnn_oracle.forward_l2 and energy_forces_torch):

  (a) NaN injected: the set of output rows holding any non-finite value equals the oracle's.  inf injected: it holds the
      injected rows and lies inside the oracle's set (the rows the graph can reach).  Element-level equality is not asked
      for: the kernels skip zero CG entries, the dense oracle computes 0 * inf = NaN.
  (b) Every other row is finite and within the tolerance of the kernel's existing test, relative to the largest finite
      oracle value.

The adversarial layout of the per-row products puts a bad row next to a finite row whose maximum is 1e4 in a background of
|x| <= 4: an operand scale that lost the 1e4 (one inf discarding the maximum of its lane or wave) puts that row above the
fp16 range and turns it non-finite.  Positions are always finite here (non-finite positions need an argument check of their
own)."""
import numpy as np
import pytest
import torch

import models  # noqa: F401
from oracle import cg
from oracle import l1tp_oracle as O
from oracle import segnn_oracle as S
from oracle import tp_oracle as T
from scale_reference import expected_scale
from scalable_e3_gnn_amd import ops
from scalable_e3_gnn_amd.radius_graph import radius_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAD = {"nan": float("nan"), "inf": float("inf")}
TDT = {"float32": torch.float32, "bfloat16": torch.bfloat16}


def _np(t):
    return t.detach().double().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def check_rows(got, want, injected, kind, tol, what=""):
    """(a) and (b) above; `injected`: output rows that hold an injected value themselves (per-row products), or None."""
    got, want = _np(got), _np(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gb, wb = ~np.isfinite(got).all(1), ~np.isfinite(want).all(1)
    assert wb.any(), (what, "the oracle has no non-finite row: nothing was injected")
    if kind == "nan":
        diff = np.flatnonzero(gb != wb)
        assert diff.size == 0, (what, "non-finite rows differ from the oracle's", diff[:8], gb[diff[:8]])
    else:
        if injected is not None:
            assert gb[injected].all(), (what, "an injected inf row came out finite", np.asarray(injected)[~gb[injected]])
        out = np.flatnonzero(gb & ~wb)
        assert out.size == 0, (what, "non-finite rows the oracle keeps finite", out[:8])
    ok = ~wb
    assert np.isfinite(got[ok]).all(), (what, np.flatnonzero(~np.isfinite(got[ok]).all(1))[:8])
    scale = float(np.abs(want[ok]).max()) if ok.any() else 0.0
    if scale == 0.0:   # every finite row is zero (rows without an edge of the subset): exactly zero
        assert not ok.any() or float(np.abs(got[ok]).max()) == 0.0, what
        return
    err = float(np.abs(got[ok] - want[ok]).max()) / scale
    assert err <= tol, (what, err, tol)


# ---------------------------------------------------------------------------------------------------------------------
# per-row products
# ---------------------------------------------------------------------------------------------------------------------
def _rows(B, D, kind, seed):
    """[B, D] fp64 features |x| <= 4; the last element of row 36 holds 1e4 and the first of row 37 the injected value
    (adjacent float4s: one wave of the dense absmax path for D = 128 and 288), as do rows 0, 120 and B - 1."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(B, D, generator=g, dtype=torch.float64) * 8 - 4)
    x[36, D - 1] = 1e4
    bad = [37, 0, 120, B - 1]
    x[37, 0] = BAD[kind]
    x[0, 0] = BAD[kind]
    x[120, D - 1] = BAD[kind]
    x[B - 1, D // 2] = BAD[kind]
    return x, bad


def _WN(mod, classes):
    W = {c: getattr(mod, "weights_" + c).detach().double().cpu().numpy() for c in classes if hasattr(mod, "weights_" + c)}
    N = {c: getattr(mod, "norm_" + c).double().cpu().numpy() if hasattr(mod, "norm_" + c) else np.zeros(0) for c in classes}
    return W, N


@pytest.mark.parametrize("kind", list(BAD))
@pytest.mark.parametrize("dtype", list(TDT))
@pytest.mark.parametrize("lmax", [1, 2])
def test_sh_tensor_product_rows(lmax, dtype, kind):
    from scalable_e3_gnn_amd.tensor_product import SHTensorProduct
    irreps = "32x0e+32x1o" if lmax == 1 else "32x0e+32x1o+32x2e"
    dt = TDT[dtype]
    tol = 1e-5 if dtype == "float32" else 1e-2                     # test_tp_l2.py / test_bf16_gpu.py
    torch.manual_seed(lmax)
    mod = SHTensorProduct(irreps, irreps, lmax).to(dt).to(DEV)
    assert mod.fused_supported(False)
    B = 203
    x64, bad = _rows(B, mod.in1_dim, kind, seed=lmax)
    y64 = torch.randn(B, mod.in2_dim, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    x, y = x64.to(dt).to(DEV), y64.float().to(DEV)                # the SH operand stays fp32 in bf16 storage
    xr, yr = x.double().cpu().numpy(), y.double().cpu().numpy()      # the oracle sees the stored (rounded) values
    W, N = _WN(mod, T.CLASSES)
    with np.errstate(invalid="ignore", over="ignore"):
        want = T.forward(irreps, irreps, lmax, xr, yr, W, N)
    with torch.no_grad():
        check_rows(mod(x, y), want, bad, kind, tol, "forward")
        if dtype == "float32":
            mod.exact = True
            check_rows(mod(x, y), want, bad, kind, tol, "exact")
            mod.exact = False
        # gathered segment: rows in another order, some twice
        idx = torch.cat([torch.arange(B - 1, -1, -1), torch.tensor([37, 36, 36, 5])]).int()
        got = mod.forward_fused([(x, idx.to(DEV))], y[idx.long().to(DEV)], gate=False)
        with np.errstate(invalid="ignore", over="ignore"):
            wantg = T.forward(irreps, irreps, lmax, xr[idx.long()], yr[idx.long()], W, N)
        inj = np.flatnonzero(np.isin(idx.numpy(), bad))
        check_rows(got, wantg, inj, kind, tol, "gathered")
        # fused segment sum: rows summed per node (ascending node ids, runs of 1 .. 5 rows)
        node = torch.repeat_interleave(torch.arange(70), torch.tensor([1, 2, 3, 4, 5] * 14))[:B]
        node = torch.cat([node, torch.full((B - node.numel(),), 70)]).int()
        got = mod.forward_fused([(x, None)], y, gate=False, scatter=(node.to(DEV), 71))
        if got is not None:   # (None: the library has no fused segment-sum kernel for this plan)
            wants = np.zeros((71, want.shape[1]))
            with np.errstate(invalid="ignore"):
                np.add.at(wants, node.long().numpy(), want)
            check_rows(got, wants, np.unique(node.numpy()[bad]), kind, tol, "scatter")
        # epilogue: residual add (+ the operand scale of the result in fp32)
        res = (torch.rand(B, want.shape[1], generator=torch.Generator().manual_seed(3)) * 8 - 4).to(dt).to(DEV)
        if dtype == "float32":
            got, sc = mod.forward_fused([(x, None)], y, gate=False, residual=res, out_scale=10)
            s, inv, bits = expected_scale([got.cpu().numpy()], 10)
            assert (float(sc[0]), float(sc[1])) == (s, inv), "the scale of the result is over its finite values"
        else:
            got = mod.forward_fused([(x, None)], y, gate=False, residual=res)
        check_rows(got, want + res.double().cpu().numpy(), bad, kind, tol, "epilogue")


@pytest.mark.parametrize("kind", list(BAD))
@pytest.mark.parametrize("dtype", list(TDT))
@pytest.mark.parametrize("kernel", [1, 0])   # generic kernel / auto (the MFMA kernel where the plan has one)
def test_l1_tensor_product_rows(kernel, dtype, kind):
    from models.segnn.l1_tensor_prod import L1TensorProduct
    from scalable_e3_gnn_amd import Irreps
    irreps = "16x0e+16x1o"
    dt = TDT[dtype]
    torch.manual_seed(2)
    mod = L1TensorProduct(Irreps(irreps)).to(dt).to(DEV)
    mod.kernel = kernel
    B = 300
    x64, bad = _rows(B, mod.in1_dim, kind, seed=3)
    x = x64.to(dt).to(DEV)
    y = torch.randn(B, 4, generator=torch.Generator().manual_seed(4)).to(dt).to(DEV)
    W, N = _WN(mod, O.CLASSES)
    with np.errstate(invalid="ignore", over="ignore"):
        want = O.forward_closed_form(O.make_layout(irreps), _np(x), _np(y), W, N)
    with torch.no_grad():
        got = mod(x, y)
    check_rows(got, want, bad, kind, 1e-5 if dtype == "float32" else 2e-2, f"kernel {kernel}")   # test_l1tp_gpu.py


# ---------------------------------------------------------------------------------------------------------------------
# message function
# ---------------------------------------------------------------------------------------------------------------------
def _graph(N, k, seed):
    pos = torch.rand(N, 3, generator=torch.Generator().manual_seed(seed))
    r = float((3 * k / (4 * np.pi * N)) ** (1 / 3))
    return radius_graph(pos.to(DEV), r, [0, 0, 0], [1, 1, 1])


def _edge_messages64(layer, H, lmax, h, g):
    """fp64 per-edge messages of the layer's message function on the graph's edges (numpy; tp_oracle + gate_blocks)."""
    hid = f"{H}x0e+{H}x1o" + (f"+{H}x2e" if lmax == 2 else "")
    gated = f"{H}x0e+{lmax * H}x0e+{H}x1o" + (f"+{H}x2e" if lmax == 2 else "")
    blocks = [(l, H) for l in range(1, lmax + 1)]
    src, dst = g.src.cpu().long().numpy(), g.dst.cpu().long().numpy()
    p64 = g.pos4[:, :3].double().cpu().numpy()
    rel = p64[src] - p64[dst]
    Y = cg.sh_component(lmax, rel)
    dd = np.sqrt((rel * rel).sum(1))
    hd = _np(h)
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.concatenate([hd[dst], hd[src], dd[:, None]], 1)
        m = S.gate_blocks(T.forward(f"{hid}+{hid}+1x0e", gated, lmax, m, Y, *_WN(layer.msg1, T.CLASSES)), H, blocks)
        m = S.gate_blocks(T.forward(hid, gated, lmax, m, Y, *_WN(layer.msg2, T.CLASSES)), H, blocks)
    return m, dst


def _sum64(m, dst, N):
    out = np.zeros((N, m.shape[1]))
    with np.errstate(invalid="ignore"):
        np.add.at(out, dst, m)
    return out


def _bad_features(N, D, kind, nodes, seed, dtype):
    h = torch.randn(N, D, generator=torch.Generator().manual_seed(seed))
    for i, n in enumerate(nodes):
        h[n, (7 * i) % D] = BAD[kind]
    return h.to(dtype).to(DEV)


MSG_CASES = [("float32", 1, 16), ("float32", 1, 32), ("float32", 1, 64), ("float32", 2, 16), ("float32", 2, 32),
             ("float32", 2, 64), ("bfloat16", 2, 32), ("bfloat16", 1, 32), ("bfloat16", 2, 64)]


@pytest.mark.parametrize("kind", list(BAD))
@pytest.mark.parametrize("dtype,lmax,H", MSG_CASES)
def test_fused_message_rows(dtype, lmax, H, kind):
    from scalable_e3_gnn_amd.segnn import SEGNNLayer
    dt = TDT[dtype]
    torch.manual_seed(30 + lmax + H)
    N = 600
    g = _graph(N, 9.0, seed=H + lmax)
    layer = SEGNNLayer(H, lmax).to(dt).to(DEV)
    assert layer._msg.supports(dt)
    D = H * (lmax + 1) ** 2
    bad = [0, 17, 300, N - 1]
    h = _bad_features(N, D, kind, bad, seed=lmax + H, dtype=dt)
    m, dst = _edge_messages64(layer, H, lmax, h, g)
    want = _sum64(m, dst, N)
    tol = 1e-5 if dtype == "float32" else 2e-2                    # test_msg_fused_gpu.py / test_bf16_gpu.py
    with torch.no_grad():
        for tpb in (0, -4):
            layer._msg.tiles_per_block = tpb
            check_rows(layer._msg.forward(h, g, layer.msg1, layer.msg2), want, None, kind, tol, f"tpb {tpb}")
        if dtype == "float32":   # the unfused chain: gather_concat, exact fp32 products, gate_blocks, segment_sum
            Y, d, _ = ops.edge_geometry(g, lmax=lmax)
            for tp in (layer.msg1, layer.msg2):
                if hasattr(tp, "exact"):
                    tp.exact = True
                else:
                    tp.kernel = 1
            a = ops.gather_concat(h, g, d)
            a = layer._gate(layer.msg1(a, Y))
            a = layer._gate(layer.msg2(a, Y))
            check_rows(ops.segment_sum(a, g), want, None, kind, tol, "unfused chain")


@pytest.mark.parametrize("kind", list(BAD))
def test_fused_message_edge_subsets_rows(kind):
    """The `edges=` subsets of test_fused_message_edge_subsets, with bad source rows in tiles that hold one dst run (the
    hub), two runs and a tail tile."""
    from scalable_e3_gnn_amd.segnn import SEGNNLayer
    torch.manual_seed(21)
    gen = torch.Generator().manual_seed(8)
    N = 1200
    pos = torch.rand(N, 3, generator=gen)
    pos[:300] = 0.5 + 0.02 * torch.randn(300, 3, generator=gen)
    g = radius_graph(pos.to(DEV), 0.06, [0, 0, 0], [1, 1, 1])
    E = g.num_edges
    deg = (g.rowptr[1:] - g.rowptr[:-1])
    hub = int(deg.argmax())
    lo, hi = int(g.rowptr[hub]), int(g.rowptr[hub + 1])
    src = g.src.cpu().long()
    bad = sorted({int(src[lo + 3]), int(src[16]), int(src[0]), int(src[120])})
    layer = SEGNNLayer(32, 2).to(DEV)
    h = _bad_features(N, 288, kind, bad, seed=5, dtype=torch.float32)
    m, dst = _edge_messages64(layer, 32, 2, h, g)
    ar = torch.arange(E)
    subsets = {"one edge": ar[:1], "17 edges": ar[:17], "33 edges": ar[100:133], "hub only": ar[lo:hi],
               "hub + neighbours": ar[max(0, lo - 5):min(E, hi + 7)], "every 3rd": ar[::3], "every 7th": ar[3::7],
               "all": ar}
    with torch.no_grad():
        for name, sel in subsets.items():
            s, dd = g.src[sel.to(DEV)].contiguous(), g.dst[sel.to(DEV)].contiguous()
            want = _sum64(m[sel.numpy()], dst[sel.numpy()], N)
            if np.isfinite(want).all():
                continue   # this subset reaches no bad row (checked by the `all` subset)
            for tpb in (0, 1, -1):
                layer._msg.tiles_per_block = tpb
                got = layer._msg.forward(h, g, layer.msg1, layer.msg2, edges=(s, dd))
                check_rows(got, want, None, kind, 1e-5, (name, tpb))


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
def _segnn_case(N, seed):
    from scalable_e3_gnn_amd.segnn import SEGNN
    torch.manual_seed(seed)
    pos = torch.rand(N, 3, generator=torch.Generator().manual_seed(seed))
    r = float((3 * 16.0 / (4 * np.pi * N)) ** (1 / 3))
    model = SEGNN("1x0e+1x1o", 32, "1x1o", 4, lmax=2).to(DEV)
    g = radius_graph(pos.to(DEV), r, [0, 0, 0], [1, 1, 1])
    perm = g.perm.cpu().long()
    xs = torch.randn(N, 4, generator=torch.Generator().manual_seed(seed + 1))[perm]
    corner = int(pos[perm].norm(dim=1).argmin())       # a node in a corner: its 4-hop reach stays a fraction of the cloud
    return model, g, xs, pos[perm].numpy(), corner


@pytest.mark.parametrize("kind", list(BAD))
def test_segnn_four_layers_rows(kind):
    """The 4-layer bench-mode SEGNN (one-launch message kernel, fp32 and bf16 storage) and the r16 path (per-product
    fused kernels) with one bad node, against forward_l2."""
    from scalable_e3_gnn_amd.segnn import SEGNN
    model, g, xs, pos, corner = _segnn_case(2000, seed=5)
    xs[corner, 1] = BAD[kind]
    geo = (pos, g.rowptr.cpu().numpy(), g.src.cpu().numpy())
    params = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    with np.errstate(invalid="ignore", over="ignore"):
        want = S.forward_l2(params, 32, 4, "1x0e+1x1o", "1x1o", xs.double().numpy(), *geo)
    assert (~np.isfinite(want).all(1)).sum() < 1000
    with torch.no_grad():
        check_rows(model(xs.to(DEV), g), want, [corner], kind, 1e-5, "bench mode fp32")   # test_parity_bench_mode_gpu.py
        for l in model.layers:
            l.fuse_message = False
        check_rows(model(xs.to(DEV), g), want, [corner], kind, 1e-5, "r16 path fp32")
    m16 = SEGNN("1x0e+1x1o", 32, "1x1o", 4, lmax=2).to(DEV)
    m16.load_state_dict(model.state_dict())
    m16 = m16.bfloat16()
    p16 = {k: v.detach().float().double().cpu().numpy() for k, v in m16.state_dict().items()}
    x16 = xs.bfloat16()
    with np.errstate(invalid="ignore", over="ignore"):
        want16 = S.forward_l2(p16, 32, 4, "1x0e+1x1o", "1x1o", x16.double().numpy(), *geo)
    with torch.no_grad():
        check_rows(m16(x16.to(DEV), g), want16, [corner], kind, 2e-2, "bench mode bf16")   # BF16_FOUR_LAYER_BOUND


def test_batched_energy_nan_molecule():
    """NaN in one molecule's node features: every other molecule's energy and forces are finite and match
    energy_forces_torch at the tolerances of test_forces_gpu.py."""
    from scalable_e3_gnn_amd.batched import BatchedEnergyModel, batched_radius_graph
    rng = np.random.default_rng(5)
    n_mol, H, L, lmax, r = 24, 16, 2, 1, 3.0
    sizes = rng.integers(3, 30, n_mol)
    pos = np.concatenate([rng.normal(size=(n, 3)) * 1.5 + rng.uniform(-40, 40, 3) for n in sizes]).astype(np.float32)
    batch = np.concatenate([np.full(n, i) for i, n in enumerate(sizes)])
    order = rng.permutation(len(batch))
    pos, batch = pos[order], batch[order]
    torch.manual_seed(6)
    model = BatchedEnergyModel("1x0e+1x1o", H, L, lmax=lmax).to(DEV)
    x = torch.randn(len(batch), 4, generator=torch.Generator().manual_seed(7))
    sick = 5
    x[int(np.flatnonzero(batch == sick)[0]), 0] = float("nan")
    xd, pd, bd = x.to(DEV), torch.from_numpy(pos).to(DEV), torch.from_numpy(batch).to(DEV)
    model.eval()
    with torch.no_grad():
        e_fast = model(xd, pd, bd, r)
        e, f = model(xd, pd, bd, r, forces=True)
    g, mol = batched_radius_graph(pd, bd, r)
    perm = g.perm.cpu().numpy()
    params = {k[len("net."):]: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    E64, F64, _ = S.energy_forces_torch(params, H, L, lmax, "1x0e+1x1o", x.double().numpy()[perm],
                                        pos.astype(np.float64)[perm], g.rowptr.cpu().numpy(), g.src.cpu().numpy(),
                                        mol.cpu().numpy(), n_mol)
    E64 = np.asarray(E64, dtype=np.float64)
    F_want = np.empty_like(F64)
    F_want[perm] = F64
    others = np.arange(n_mol) != sick
    assert not np.isfinite(E64[sick])
    for name, got in (("energy", e), ("energy (fused inference)", e_fast)):
        got = _np(got)
        assert not np.isfinite(got[sick]), name
        assert np.isfinite(got[others]).all(), (name, np.flatnonzero(~np.isfinite(got) & others))
        assert np.abs(got[others] - E64[others]).max() / np.abs(E64[others]).max() < 1e-5, name
    fo = batch != sick
    fg = _np(f)
    assert np.isfinite(fg[fo]).all(), np.flatnonzero(~np.isfinite(fg).all(1) & fo)[:8]
    assert np.isfinite(F_want[fo]).all()
    ferr = np.abs(fg[fo] - F_want[fo]).max() / np.abs(F_want[fo]).max()
    assert ferr < 2e-5, ferr


def _shard_worker(rank, world, N, kind, q):
    import torch.distributed as dist
    owed = 2 if rank == 0 else 1   # items this rank puts on the queue
    try:
        import models  # noqa
        from scalable_e3_gnn_amd.radius_graph import radius_graph as rg
        from scalable_e3_gnn_amd.segnn import SEGNN
        from scalable_e3_gnn_amd.sharding import SlabHalo
        dev = "cuda:0"
        g0 = torch.Generator().manual_seed(11)
        pos = torch.rand(N, 3, generator=g0)
        pos[:, 0] *= world
        x = torch.randn(N, 4, generator=g0)
        face = int((pos[:, 0] - 1.0).abs().argmin())        # the particle nearest the slab face: a ghost of both ranks
        x[face, 2] = BAD[kind]
        r = float((3 * 16.0 / (4 * np.pi * (N / world))) ** (1 / 3))
        torch.manual_seed(0)
        model = SEGNN("1x0e+1x1o", 32, "1x1o", 3, lmax=2).to(dev)
        own = ((pos[:, 0] >= rank) & (pos[:, 0] < rank + 1)).nonzero().flatten()
        halo = SlabHalo()
        lpos, lx = halo.setup(pos[own].to(dev), x[own].to(dev), float(rank), float(rank + 1), r)
        g = rg(lpos, r, [rank - 2 * r, 0, 0], [rank + 1 + 2 * r, 1, 1])
        halo.renumber(g.perm)
        split = halo.split_graph(g)
        with torch.no_grad():
            out = model(lx[g.perm.long()], g, halo=halo, split=split)   # overlapped refresh: the overflow guard runs
            out_b = model(lx[g.perm.long()], g, halo=halo)              # blocking refresh
        q.put(("part", out[halo.owned_new].cpu().numpy(), out_b[halo.owned_new].cpu().numpy(), own.numpy()))
        owed -= 1
        if rank == 0:
            gg = rg(pos.to(dev), r, [0, 0, 0], [world, 1, 1])
            with torch.no_grad():
                full = model(x.to(dev)[gg.perm.long()], gg)
            ref = torch.empty_like(full)
            ref[gg.perm.long()] = full
            q.put(("ref", ref.cpu().numpy(), None, np.array([face])))
            owed -= 1
    except Exception as e:  # noqa: BLE001  (reported to the parent instead of a queue timeout)
        for _ in range(owed):
            q.put(("error", f"rank {rank}: {type(e).__name__}: {e}", None, None))
    dist.barrier()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", list(BAD))
def test_sharded_forward_bad_ghost_rows(kind):
    """Two ranks on one GPU (test_sharding_gpu.py): a bad particle at the slab face is a refreshed ghost row of the other
    rank.  The forward must not raise (the overflow guard reads finite row maxima), and the merged result has the
    single-process forward's non-finite rows and its values elsewhere."""
    import gloo_ranks
    world, N = 2, 6000
    got = gloo_ranks.run(_shard_worker, world, (N, kind), world + 1, 240)
    errs = [g[1] for g in got if g[0] == "error"]
    assert not errs, errs
    ref = [g for g in got if g[0] == "ref"][0]
    ref, face = ref[1], int(ref[3][0])
    assert not np.isfinite(ref[face]).all()
    for which in (1, 2):   # overlapped, blocking
        merged = np.full_like(ref, 7.0)
        for tag, a, b, idx in got:
            if tag == "part":
                merged[idx] = a if which == 1 else b
        gb, wb = ~np.isfinite(merged).all(1), ~np.isfinite(ref).all(1)
        assert np.array_equal(gb, wb), (which, np.flatnonzero(gb != wb)[:8])
        ok = ~wb
        assert np.abs(merged[ok] - ref[ok]).max() / np.abs(ref[ok]).max() < 2e-5   # test_sharding_gpu.py

"""Owned sums of the weights-stationary message kernel (e3_msg_forward_owned: every row of the aggregated messages is written
exactly once -- by the kernel's plain stores, by the merge of the chunk-boundary rows or by the isolated-rows kernel -- and
the operand scale of the sums comes out of the same launches) against the zero-fill + atomics path (``owned_sums = False``),
the exact fp32 chain and the numpy restatement of the scale contract.

Graphs are built by hand (48 nodes, dst-sorted edges with prescribed in-degrees), so that every case of the ownership
rule occurs at 16 edges per chunk: isolated nodes at row 0, at row N - 1, two in a row, and between a run that ends on a chunk
boundary and one that starts on it; degree 1; a run of exactly one chunk that starts on a chunk boundary; a run of 70 edges
that spans 5 chunks.  E = 227 is no multiple of 16; the second graph has E = 40, which leaves five of the eight XCD eighths
empty.

The comparison with the exact fp32 chain (3e-6, the bound of tests/test_msg_fused_gpu.py) is made in fp32 storage: that
chain is no reference for bf16 storage, whose products round to bf16 (bf16 cases check new against old path, the scale and
reproducibility)."""
import numpy as np
import pytest
import torch

import scale_reference as R
from scalable_e3_gnn_amd import ops
from scalable_e3_gnn_amd.radius_graph import RadiusGraph, radius_graph
from scalable_e3_gnn_amd.segnn import SEGNN, SEGNNLayer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, H, LMAX, W = 48, 32, 2, 288

# in-degrees, node by node (edge ranges in brackets)
_DEG_A = ([0,          # 0: isolated, row 0
           5,          # 1: [0, 5)
           11,         # 2: [5, 16)    ends on a chunk boundary
           16,         # 3: [16, 32)   exactly one chunk, starting on a chunk boundary
           1,          # 4: [32, 33)   degree 1
           15,         # 5: [33, 48)   ends on a chunk boundary
           0,          # 6: isolated between a run that ends on the boundary 48 and one that starts on it
           2,          # 7: [48, 50)
           70,         # 8: [50, 120)  chunks 3 .. 7 at 16 edges per chunk
           0, 0,       # 9, 10: two isolated nodes in a row
           8,          # 11: [120, 128) ends on a chunk boundary
           0,          # 12: isolated directly behind that boundary
           3]          # 13: [128, 131)
          + [(i % 5) + 1 for i in range(33)]   # 14 .. 46
          + [0])       # 47: isolated, row N - 1
_DEG_B = [0] * N
_DEG_B[3], _DEG_B[4], _DEG_B[20] = 10, 12, 18   # E = 40: runs across the boundaries 16 and 32, eighths 3 .. 7 empty


def _hand_graph(deg, seed, box=None):
    assert len(deg) == N
    gen = torch.Generator().manual_seed(seed)
    degt = torch.tensor(deg, dtype=torch.int64)
    rowptr = torch.zeros(N + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(degt, 0).int()
    E = int(rowptr[-1])
    dst = torch.repeat_interleave(torch.arange(N), degt)
    src = (dst + 1 + torch.randint(0, N - 1, (E,), generator=gen)) % N   # never a self edge
    src = torch.cat([s.sort().values for s in torch.split(src, deg)]) if E else src
    pos4 = torch.zeros(N, 4)
    pos4[:, :3] = torch.rand(N, 3, generator=gen)
    g = RadiusGraph(perm=torch.arange(N, dtype=torch.int32, device=DEV), pos4=pos4.to(DEV), rowptr=rowptr.to(DEV),
                    src=src.int().to(DEV), num_edges=E, grid=(1, 1, 1), box=box)
    assert torch.equal(g.dst.cpu().long(), dst)
    return g


def _parts(deg, tpb):
    """Partial sums per node: the (XCD eighth, chunk) pairs its run touches -- the kernel's split of the edge range."""
    E = sum(deg)
    chunk = 16 * tpb if tpb > 0 else 256
    e_per_xcd = ((E + 7) // 8 + 15) // 16 * 16
    out, e = [], 0
    for d in deg:
        out.append(len({(k // e_per_xcd, (k % e_per_xcd) // chunk) for k in range(e, e + d)}))
        e += d
    return torch.tensor(out)


def _unfused(layer, h, g):
    Y, d, _ = ops.edge_geometry(g, lmax=LMAX)
    for tp in (layer.msg1, layer.msg2):
        tp.exact = True
    m = ops.gather_concat(h, g, d)
    m = layer._gate(layer.msg1(m, Y))
    m = layer._gate(layer.msg2(m, Y))
    return ops.segment_sum(m, g)


def _run(layer, h, g, owned, tpb):
    layer._msg.owned_sums, layer._msg.tiles_per_block = owned, tpb
    out = torch.full((N, W), float("nan"), device=DEV)   # an unwritten row shows up
    with torch.no_grad():
        got, scale = layer._msg.forward(h, g, layer.msg1, layer.msg2, return_scale=True, out=out)
    assert got.data_ptr() == out.data_ptr()
    return got, scale


def _check_scale(scale, a, tag):
    s, inv, bits = R.expected_scale([a.cpu().numpy()], 10)
    got = scale.cpu()
    print(f"{tag}: scale {float(got[0])} 1/s {float(got[1])} bits {int(got.view(torch.int32)[2]):#x} | expected {s} {inv} {bits:#x}")
    assert float(got[0]) == s and float(got[1]) == inv and int(got.view(torch.int32)[2]) == bits, tag


_EXACT = {}


def _exact(key, layer, h, g):
    """The exact fp32 chain, once per (graph, features)."""
    if key not in _EXACT:
        with torch.no_grad():
            _EXACT[key] = _unfused(layer, h, g)
    return _EXACT[key]


def _layer(dtype):
    torch.manual_seed(17)
    layer = SEGNNLayer(H, LMAX)
    return (layer.bfloat16() if dtype == torch.bfloat16 else layer).to(DEV)


def _features(dtype, seed=5):
    return torch.randn(N, W, generator=torch.Generator().manual_seed(seed)).to(dtype).to(DEV)


def test_hand_graph_has_the_cases():
    for tpb in (1, 2, 0):
        assert int(_parts(_DEG_A, tpb).max()) > 2
    p = _parts(_DEG_A, 1)
    assert int(p[8]) == 5 and int(p[3]) == 1 and sum(_DEG_A) % 16 and sum(_DEG_A[:3]) == 16 and sum(_DEG_A[:8]) % 16 == 2
    assert sum(_DEG_B) == 40 and int(_parts(_DEG_B, 1).max()) == 2


_CASES = [(gr, tpb, dt) for gr in ("A", "B") for tpb in (1, 2, 0) for dt in (torch.float32, torch.bfloat16)] + \
         [("A-periodic", 1, torch.float32)]


@pytest.mark.parametrize("graph,tpb,dtype", _CASES, ids=[f"{c[0]}-tpb{c[1]}-{str(c[2])[6:]}" for c in _CASES])
def test_owned_sums_against_atomics_path(graph, tpb, dtype):
    deg = _DEG_B if graph == "B" else _DEG_A
    g = _hand_graph(deg, seed=3, box=(1.0, 1.0, 1.0) if graph == "A-periodic" else None)
    layer, h = _layer(dtype), _features(dtype)
    old, no_scale = _run(layer, h, g, False, tpb)
    new, scale = _run(layer, h, g, True, tpb)
    assert no_scale is None and scale is not None
    assert not torch.isnan(new).any() and not torch.isnan(old).any()
    degt, parts = torch.tensor(deg), _parts(deg, tpb)
    # (1) new against old path
    iso = (degt == 0).to(DEV)
    assert float(new[iso].abs().max()) == 0.0
    few = (parts <= 2).to(DEV)
    assert torch.equal(new[few], old[few])
    many = ~few
    if many.any():
        top = torch.maximum(new[many].abs().amax(1), old[many].abs().amax(1))
        ulp = torch.exp2(torch.floor(torch.log2(top)) - 23)
        dev_ulp = ((new[many] - old[many]).abs().amax(1) / ulp).max()
        print(f"{graph} tpb={tpb} {dtype}: rows with > 2 parts differ by {float(dev_ulp):.2f} ulp of the row maximum")
        assert float(dev_ulp) <= 4.0
    # (2) against the exact fp32 chain
    if dtype == torch.float32:
        want = _exact(graph, layer, h, g)
        err = float((new - want).abs().max() / want.abs().max())
        print(f"{graph} tpb={tpb}: owned sums vs exact fp32 chain {err:.2e}")
        assert err < 3e-6, err
    # (3) the scale of the sums
    _check_scale(scale, new, f"{graph} tpb={tpb} {dtype}")
    # (4) reproducible
    for _ in range(2):
        again, scale2 = _run(layer, h, g, True, tpb)
        assert torch.equal(again, new) and torch.equal(scale2.view(torch.int32), scale.view(torch.int32))


@pytest.mark.parametrize("tpb", [1, 0])
def test_scale_with_nonfinite_and_zero_features(tpb):
    g = _hand_graph(_DEG_A, seed=3)
    layer, h = _layer(torch.float32), _features(torch.float32)
    # one src row of h holds inf: a finite maximum elsewhere
    srcs = set(g.src.cpu().tolist())
    row = next(n for n in range(N) if n in srcs and _DEG_A[n] > 0)
    hi = h.clone()
    hi[row, 7] = float("inf")
    layer._msg.owned_sums, layer._msg.tiles_per_block = True, tpb
    with torch.no_grad():
        a, scale = layer._msg.forward(hi, g, layer.msg1, layer.msg2, return_scale=True)
    fin = torch.isfinite(a)
    assert (~fin).any() and fin.any() and float(a[fin].abs().max()) > 0
    _check_scale(scale, a, f"inf row tpb={tpb}")
    with torch.no_grad():
        a, scale = layer._msg.forward(torch.zeros_like(h), g, layer.msg1, layer.msg2, return_scale=True)
    assert torch.isfinite(a).all()
    _check_scale(scale, a, f"zero h tpb={tpb}")


def test_model_owned_sums_equal_atomics_and_embedding_scale():
    n, k = 2000, 12.0
    pos = torch.rand(n, 3, generator=torch.Generator().manual_seed(4))
    g = radius_graph(pos.to(DEV), float((3 * k / (4 * np.pi * n)) ** (1 / 3)), [0, 0, 0], [1, 1, 1])
    # no node exceeds two partial sums at the default chunk: its run touches at most two (eighth, chunk) ranges
    rp = g.rowptr.cpu().long()
    E = int(rp[-1])
    e_per_xcd = ((E + 7) // 8 + 15) // 16 * 16
    cid = (np.arange(E) // e_per_xcd) * (1 << 20) + (np.arange(E) % e_per_xcd) // 256   # (eighth, chunk) of every edge
    steps = np.concatenate([[0], np.cumsum(cid[1:] != cid[:-1])])                        # chunk switches before edge e
    lo, hi = rp[:-1].numpy(), rp[1:].numpy()
    nz = hi > lo
    parts = 1 + steps[hi[nz] - 1] - steps[lo[nz]]
    assert int(parts.max()) == 2   # some runs cross a chunk boundary, none has more than two parts
    torch.manual_seed(3)
    model = SEGNN("1x0e+1x1o", H, "1x1o", 4, lmax=LMAX).to(DEV)
    x = torch.randn(n, 4, generator=torch.Generator().manual_seed(2)).to(DEV)
    outs = []
    with torch.no_grad():
        for owned in (True, False):
            for layer in model.layers:
                layer._msg.owned_sums = owned
            outs.append(model(x, g))
        assert torch.isfinite(outs[0]).all()
        assert torch.equal(outs[0], outs[1])
        # the scale the embedding's epilogue emits is the one a scan of h gives
        _, _, A = ops.edge_geometry(g, lmax=LMAX, want_edge=False)
        h, sc = model.embed.forward_fused([(x, None)], A, gate=False, out_scale=10)
        assert torch.equal(h, model.embed(x, A))
        want = ops.pow2_scale([h])
        assert torch.equal(sc.view(torch.int32)[:3], want.view(torch.int32)[:3])

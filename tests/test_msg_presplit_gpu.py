"""Pre-split feature rows of the weights-stationary message kernel (fp32 storage, H = 32, l_max = 2).

The pre-mix launch leaves, per node, the fp16 (hi, lo) B fragments of product #1 behind its table (include/e3gnn.h, "pre-mix
buffer"); the edge kernel gathers them instead of converting h[src] once per edge.  Checked here: the rows bit for bit against a
numpy restatement, the refresh of rows that changed after the pre-mix launch, the tile stream of the edge kernel on edge lists
that stress its tile cutter and both parities of its double-buffered image, and the size of the buffer."""
import functools

import numpy as np
import pytest
import torch

from scalable_e3_gnn_amd import ops
from scalable_e3_gnn_amd.radius_graph import RadiusGraph, radius_graph
from scalable_e3_gnn_amd.segnn import SEGNNLayer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, LMAX, W = 32, 2, 288
NC = (LMAX + 1) ** 2


def _graph_of(pos, src, dst):
    """A graph object over an explicit edge list (any order): CSR by dst, src ascending inside a row."""
    N = pos.shape[0]
    src, dst = torch.as_tensor(src, dtype=torch.int64), torch.as_tensor(dst, dtype=torch.int64)
    order = torch.argsort(dst * N + src)
    src, dst = src[order], dst[order]
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(dst, minlength=N), 0)
    pos4 = torch.zeros(N, 4)
    pos4[:, :3] = pos
    return RadiusGraph(perm=torch.arange(N, dtype=torch.int32, device=DEV), pos4=pos4.to(DEV),
                       rowptr=rowptr.to(torch.int32).to(DEV), src=src.to(torch.int32).to(DEV).contiguous(),
                       num_edges=int(src.numel()), grid=())


@functools.lru_cache(maxsize=None)
def _layer():
    torch.manual_seed(17)
    return SEGNNLayer(H, LMAX).to(DEV)


def _ring_graph(N, seed):
    pos = torch.rand(N, 3, generator=torch.Generator().manual_seed(seed))
    i = torch.arange(N)
    return _graph_of(pos, torch.cat([(i + 1) % N, (i + 5) % N]), torch.cat([i, i]))


def _rows_h(N, seed, ld):
    """[N, W] view (row stride ld) with row magnitudes 1e-4 .. 1e3 and one all-zero row.  The tensor's scale puts the
    largest row at 2^6 .. 2^10, so the small rows have lo halves that are fp16 subnormals (|s v| < 2^-3) or zero."""
    gen = torch.Generator().manual_seed(seed)
    big = torch.zeros(N, ld)
    mag = 10.0 ** torch.linspace(-4, 3, N)[torch.randperm(N, generator=gen)]
    big[:, :W] = torch.randn(N, W, generator=gen) * mag[:, None]
    big[N // 2, :W] = 0.0
    big[:, W:] = 7.0   # the row tail is not part of h
    return big.to(DEV)[:, :W]


def _split_reference(h, s):
    """numpy restatement: uint16 [N, NC fragments, 2 halves, 4 k groups, 8 k slots]"""
    v = h.detach().cpu().numpy().astype(np.float32)
    s = np.float32(s)
    N = v.shape[0]
    out = np.zeros((N, NC, 2, 4, 8), dtype=np.uint16)
    for l in range(LMAX + 1):
        for a in range(2 * l + 1):
            for g in range(4):
                for jj in range(8):
                    ch = 16 * (jj >> 2) + 4 * g + (jj & 3)
                    x = (s * v[:, H * l * l + ch * (2 * l + 1) + a]).astype(np.float32)
                    hi = x.astype(np.float16)
                    lo = (x - hi.astype(np.float32)).astype(np.float32).astype(np.float16)
                    out[:, l * l + a, 0, g, jj] = hi.view(np.uint16)
                    out[:, l * l + a, 1, g, jj] = lo.view(np.uint16)
    return out


def _premix(h, g, in_scale):
    layer = _layer()
    layer._msg.tiles_per_block = 0
    with torch.no_grad():
        _, state = layer._msg.forward(h, g, layer.msg1, layer.msg2, in_scale, return_state=True)
    return state


def _regions(state, N):
    table, split, hmax = _layer()._msg.premix_regions(torch.device(DEV), state[1], N)
    return table, split, hmax


def _split_u16(split):
    return split.contiguous().cpu().numpy().view(np.uint16).reshape(-1, NC, 2, 4, 8)


@pytest.mark.parametrize("given", [True, False])
def test_split_rows_bit_for_bit(given):
    N = 37   # the last pre-mix tile is partial
    h = _rows_h(N, seed=3, ld=W + 32)
    assert h.stride(0) == W + 32
    g = _ring_graph(N, seed=1)
    sc = ops.pow2_scale([h], target_log2=6) if given else None
    state = _premix(h, g, sc)
    s = float((sc if given else ops.pow2_scale([h]))[0])
    table, split, hmax = _regions(state, N)
    assert split.shape == (N, NC * 32)
    got, want = _split_u16(split), _split_reference(h, s)
    lo = want[:, :, 1].view(np.float16)
    assert ((lo != 0) & (np.abs(lo) < 2.0 ** -14)).any(), "the inputs must produce subnormal lo halves"
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, (bad[:5], got[tuple(bad[0])] if bad.size else None, want[tuple(bad[0])] if bad.size else None)
    want_max = (h.abs() * np.float32(s)).amax(1)
    assert torch.equal(hmax, want_max)


def test_refresh_rows():
    N = 37
    h = _rows_h(N, seed=5, ld=W + 32)
    g = _ring_graph(N, seed=2)
    sc = ops.pow2_scale([h], target_log2=6)
    state = _premix(h, g, sc)
    before = [t.clone() for t in _regions(state, N)]
    rows = torch.tensor([0, 11, 18, 29, N - 1], device=DEV)
    h[rows] = torch.randn(5, W, device=DEV) * torch.tensor([3.0, 1e-3, 40.0, 0.2, 7.0], device=DEV)[:, None]
    top = _layer()._msg.refresh_row_max(state, h, rows, sc)
    table, split, hmax = _regions(state, N)
    fresh = _regions(_premix(h, g, sc), N)
    assert torch.equal(split[rows].view(torch.int32), fresh[1][rows].view(torch.int32))
    assert torch.equal(hmax[rows], fresh[2][rows])
    assert float(top) == float(fresh[2][rows].max())
    keep = torch.ones(N, dtype=torch.bool, device=DEV)
    keep[rows] = False
    assert torch.equal(split[keep].view(torch.int32), before[1][keep].view(torch.int32))
    assert torch.equal(hmax[keep], before[2][keep])
    assert torch.equal(table.view(torch.int32), before[0].view(torch.int32))   # table rows belong to dst nodes: untouched


# ---- tile-stream shapes -------------------------------------------------------------------------------------------
def _case(name):
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    scale = None
    if name in ("one edge", "17 edges"):
        N, E = 20, 1 if name == "one edge" else 17
        pos = torch.rand(N, 3, generator=gen)
        dst = torch.sort(torch.randint(0, N, (E,), generator=gen)).values
        src = (dst + 1 + torch.randint(0, N - 1, (E,), generator=gen)) % N
    elif name == "hub then singles":   # a run across 7 tiles, then two-run tiles of fewer than 16 edges
        N = 160
        pos = torch.rand(N, 3, generator=gen)
        dst = torch.cat([torch.full((100,), 5), torch.arange(6, 56)])
        src = torch.cat([torch.arange(60, 160), (torch.arange(6, 56) * 7 + 3) % N])
    elif name == "two sources":        # every gathered row is node 0 or node N - 1
        N = 17
        pos = torch.rand(N, 3, generator=gen)
        dst = torch.arange(1, N - 1).repeat_interleave(2)
        src = torch.tensor([0, N - 1]).repeat(N - 2)
    else:                              # ~2 000 edges at k ~ 14: 8 workgroups walk >= 10 tiles each
        N = 200   # (an open box loses ~30 % of the neighbours at its faces)
        pos = torch.rand(N, 3, generator=gen)
        g = radius_graph(pos.to(DEV), float((3 * 14.0 / (4 * np.pi * N)) ** (1 / 3)), [0, 0, 0], [1, 1, 1])
        assert 1600 <= g.num_edges <= 2600, g.num_edges
        if name == "mixed magnitudes":
            scale = 10.0 ** (torch.randint(0, 5, (N,), generator=gen).float() - 2.0)   # rows 1e-2 .. 1e2 in one tensor
        h = torch.randn(N, W, generator=gen) * (1.0 if scale is None else scale[:, None])
        return g, h.to(DEV)
    assert bool((src != dst).all())
    return _graph_of(pos, src, dst), torch.randn(N, W, generator=gen).to(DEV)


@pytest.mark.parametrize("name", ["one edge", "17 edges", "hub then singles", "two sources", "random k14", "mixed magnitudes"])
def test_tile_stream_shapes(name):
    g, h = _case(name)
    layer = _layer()
    Y, d, _ = ops.edge_geometry(g, lmax=LMAX)
    edges = (g.src.contiguous(), g.dst.contiguous())
    with torch.no_grad():
        for tp in (layer.msg1, layer.msg2):   # the unfused exact chain of tests/test_msg_fused_gpu.py
            if hasattr(tp, "exact"):
                tp.exact = True   # generic fp32 FMA kernel
            else:
                tp.kernel = 1
        m = ops.gather_concat(h, g, d)
        m = layer._gate(layer.msg1(m, Y))
        m = layer._gate(layer.msg2(m, Y))
        want = ops.segment_sum(m, g)
        top = float(want.abs().max())
        layer._msg.tiles_per_block = -4   # the one-wave-per-tile kernel
        other = layer._msg.forward(h, g, layer.msg1, layer.msg2, edges=edges).clone()
        for tpb in (1, 3, 0):
            layer._msg.tiles_per_block = tpb
            got = layer._msg.forward(h, g, layer.msg1, layer.msg2, edges=edges)
            err, err2 = float((got - want).abs().max()) / top, float((got - other).abs().max()) / top
            print(f"{name}: tiles_per_block {tpb}: vs exact chain {err:.2e}, vs one-wave-per-tile kernel {err2:.2e}")
            assert torch.isfinite(got).all()
            assert err < 3e-6, (name, tpb, err)
            assert err2 < 3e-6, (name, tpb, err2)
    layer._msg.tiles_per_block = 0


@pytest.mark.parametrize("N", [1, 16, 37])
def test_buffer_size(N):
    """e3_msg_premix_floats_per_node x N floats hold the table, the pre-split rows and the row maxima, and nothing is written
    behind them.  The C entries take no buffer size (the size is the caller's contract, include/e3gnn.h): a buffer one float
    short loses the last row maximum, which is what the arithmetic below pins."""
    from scalable_e3_gnn_amd import _lib
    layer = _layer()
    lib = _lib.load()
    dev = torch.device(DEV)
    hd = layer._msg._plans.handle(dev)
    per = int(lib.e3_msg_premix_floats_per_node(hd))
    buf = torch.full((per * N + 64,), -123.0, device=DEV)
    table, split, hmax = layer._msg.premix_regions(dev, buf[:per * N], N)
    ud = table.shape[1]
    assert ud * 4 % 128 == 0 and split.shape[1] == NC * 32 and per == ud + NC * 32 + 1
    assert table.numel() + split.numel() + hmax.numel() == per * N
    assert hmax.data_ptr() + 4 * N == buf.data_ptr() + 4 * per * N      # the last row maximum is the buffer's last float
    assert split.data_ptr() == buf.data_ptr() + 4 * ud * N
    h = torch.randn(N, W, device=DEV) + 0.5
    sc = ops.pow2_scale([h])
    with torch.cuda.device(dev):
        packed = layer._msg.packed(layer.msg1, layer.msg2, dev)
        _lib.check(lib.e3_msg_premix(hd, h.data_ptr(), h.stride(0), N, packed.data_ptr(), sc.data_ptr(), buf.data_ptr(),
                                     _lib.E3_F32, torch.cuda.current_stream(dev).cuda_stream), "e3_msg_premix")
    assert bool((buf[per * N:] == -123.0).all())
    assert bool((buf[:per * N] != -123.0).all())
    assert torch.equal(hmax, (h.abs() * sc[0]).amax(1))

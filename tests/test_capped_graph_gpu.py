"""Capped radius graph on the GPU (radius_graph(..., max_neighbors=k); include/e3gnn.h, "Capped rows"): every integer output
bit for bit against the numpy restatement (tests/nearest_reference.py) in the open box, periodic boxes and a skewed cell;
exact d2 ties; neighbourhoods that arrive in several candidate chunks; an uncapped edge count beyond int32; the SEGNN
consumers and the edge geometry (forward and backward) on the directed graph; the argument checks.

Tolerances are those of the tests these shapes come from: 1e-5 of the output scale for the SEGNN forward
(tests/test_parity_bench_mode_gpu.py), 1e-6 / 2e-5 for the open / periodic geometry and 2e-5 for its backward
(tests/test_forces_gpu.py, tests/test_periodic_gpu.py)."""
import ctypes
import time

import numpy as np
import pytest
import torch

import capped_cases as C
import nearest_reference as K
from oracle import graph_oracle as G
from oracle import segnn_oracle as S
from scalable_e3_gnn_amd import _lib, ops
from scalable_e3_gnn_amd.batched import batched_radius_graph
from scalable_e3_gnn_amd.radius_graph import grid_params, radius_graph
from scalable_e3_gnn_amd.segnn import SEGNN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _same(g, perm, pos4, rowptr, src, cut, full, k):
    assert np.array_equal(g.perm.cpu().numpy(), perm)
    assert np.array_equal(g.pos4.cpu().numpy(), pos4)
    assert np.array_equal(g.rowptr.cpu().numpy(), rowptr)
    assert g.num_edges == len(src) and np.array_equal(g.src.cpu().numpy(), src)
    assert (g.max_neighbors, g.truncated, g.full_edges) == (k, cut, full)


_GRAPHS = {}


def _gpu_graph(mode, k):
    """The capped graph of the uniform cloud, built once per (mode, k) and shared (read only) by the tests below."""
    if (mode, k) not in _GRAPHS:
        pos = torch.tensor(C.uniform_cloud()).to(DEV)
        _GRAPHS[(mode, k)] = radius_graph(pos, C.R_UNIFORM, max_neighbors=k, **C.graph_kwargs(mode))
    return _GRAPHS[(mode, k)]


# ---------------------------------------------------------------------------------------------------------------------
# 1. bit-exact against the reference, every mode
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 16, 32, 64])
@pytest.mark.parametrize("mode", C.MODES)
def test_capped_graph_bit_exact(mode, k):
    perm, pos4, rowptr_c, src_c, cut, full, deg = C.capped(mode, k)
    # from the reference alone: the rows the cap has to tell apart occur
    if k in (16, 32):
        assert (deg < k).any() and (deg == k).any() and (deg > k).any()
    if k == 1:
        assert (deg > 1).all()
    if k == 64 and mode != "cell":
        assert deg.max() <= 64 and cut == 0      # the capped graph IS the uncapped graph
        _, _, rowptr, src, _, _ = C.uncapped(mode)
        assert np.array_equal(rowptr_c, rowptr) and np.array_equal(src_c, src)
    if k == 64 and mode == "cell":
        assert (deg == 64).any() and (deg > 64).any()    # the denser cell cloud: a best-64 over all 64 lanes
    if mode != "open":   # 7 (cell: 6 / 5 / 5) grid cells per axis: cells that apply the image shift and cells that skip it
        n = _gpu_graph(mode, k).grid[0]
        assert all(5 <= na <= 7 for na in n)
    g = _gpu_graph(mode, k)
    _same(g, perm, pos4, rowptr_c, src_c, cut, full, k)
    if mode == "cell":
        assert g.cell is not None and g.box is None
    elif mode != "open":
        assert g.box == tuple(float(v) for v in C.uncapped(mode)[4])


def test_uncapped_call_is_unchanged_and_k64_equals_it():
    pos = torch.tensor(C.uniform_cloud()).to(DEV)
    a = radius_graph(pos, C.R_UNIFORM, C.LO, C.HI)
    b = radius_graph(pos, C.R_UNIFORM, C.LO, C.HI, max_neighbors=None)
    c = _gpu_graph("open", 64)
    for g in (b, c):
        for f in ("perm", "pos4", "rowptr", "src"):
            assert torch.equal(getattr(a, f), getattr(g, f))
    assert (a.max_neighbors, a.truncated, a.full_edges) == (None, 0, a.num_edges)
    assert (c.max_neighbors, c.truncated, c.full_edges) == (64, 0, a.num_edges)


def test_batched_graph_passes_the_cap_through():
    """Two copies of the cloud as two molecules: each gets its own k nearest (the lattice copy only translates them)."""
    pos = torch.tensor(C.uniform_cloud()[:600]).to(DEV)
    batch = torch.cat([torch.zeros(600), torch.ones(600)]).long().to(DEV)
    g, mol = batched_radius_graph(torch.cat([pos, pos]), batch, 0.2, max_neighbors=8)
    full, _ = batched_radius_graph(torch.cat([pos, pos]), batch, 0.2)
    deg = (g.rowptr[1:] - g.rowptr[:-1]).cpu().numpy()
    fdeg = (full.rowptr[1:] - full.rowptr[:-1]).cpu().numpy()
    assert np.array_equal(deg, np.minimum(fdeg, 8)) and g.max_neighbors == 8 and g.full_edges == full.num_edges
    assert g.truncated == int((fdeg > 8).sum()) > 0
    assert torch.equal(mol[g.src.long()], mol[g.dst.long()])


# ---------------------------------------------------------------------------------------------------------------------
# 2. ties
# ---------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lower_id():
    q = (np.arange(16) / 16).astype(np.float32)
    pos = np.stack(np.meshgrid(q, q, q, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    perm, rowptr, src = G.graph(pos, C.LO, C.HI, 0.09)
    deg = np.diff(rowptr)
    assert deg.max() == 18 and (deg == 18).sum() == 14 ** 3
    sp = pos[perm]
    d2, dst = K.edge_d2(sp, rowptr, src)
    interior = np.nonzero(deg == 18)[0][0]
    row = np.sort(d2[rowptr[interior]:rowptr[interior + 1]])
    assert (row[:6] == row[0]).all() and (row[6:] == row[6]).all() and row[6] > row[0]   # 6 + 12, exactly tied
    rowptr_c, src_c, cut, full = K.cap(sp, rowptr, src, 8)
    g = radius_graph(torch.as_tensor(pos).to(DEV), 0.09, C.LO, C.HI, max_neighbors=8)
    _same(g, perm, np.concatenate([sp, np.zeros((len(sp), 1), np.float32)], 1), rowptr_c, src_c, cut, full, 8)
    # the two members of the 12-fold tie group that an interior row keeps are its two lowest ids of that group
    lo, hi = rowptr[interior], rowptr[interior + 1]
    far = np.sort(src[lo:hi][d2[lo:hi] == row[6]])[:2]
    kept = g.src.cpu().numpy()[rowptr_c[interior]:rowptr_c[interior + 1]]
    assert set(far) <= set(kept) and len(kept) == 8


def test_coincident_points():
    g = radius_graph(torch.tensor([[0.5, 0.5, 0.5]] * 5, device=DEV), 0.1, C.LO, C.HI, max_neighbors=2)
    assert g.rowptr.tolist() == [0, 2, 4, 6, 8, 10]
    assert g.src.tolist() == [1, 2, 0, 2, 0, 1, 0, 1, 0, 1]
    assert (g.truncated, g.full_edges) == (5, 20)


# ---------------------------------------------------------------------------------------------------------------------
# 3. neighbourhoods of more than one candidate chunk
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blob():
    pos = C.blob_cloud()
    perm, rowptr, src = G.graph(pos, C.LO, C.HI, 0.1)
    deg = np.diff(rowptr)
    assert deg.max() > 1024 and (deg > 1024).sum() == 1536 and np.sort(deg)[:512].max() <= 32
    sp = pos[perm]
    d2, dst = K.edge_d2(sp, rowptr, src)
    order = np.lexsort((d2, dst))
    assert ((dst[order][1:] == dst[order][:-1]) & (d2[order][1:] == d2[order][:-1])).sum() > 0   # exact ties inside rows
    return pos, perm, np.concatenate([sp, np.zeros((len(sp), 1), np.float32)], 1), rowptr, src


@pytest.mark.parametrize("k", [8, 32, 64])
def test_chunked_neighbourhoods(blob, k):
    pos, perm, pos4, rowptr, src = blob
    rowptr_c, src_c, cut, full = K.cap(pos4, rowptr, src, k)
    assert cut == int((np.diff(rowptr) > k).sum()) >= 1536 and full == len(src)
    g = radius_graph(torch.as_tensor(pos).to(DEV), 0.1, C.LO, C.HI, max_neighbors=k)
    _same(g, perm, pos4, rowptr_c, src_c, cut, full, k)
    again = radius_graph(torch.as_tensor(pos).to(DEV), 0.1, C.LO, C.HI, max_neighbors=k)   # nothing is left over in a buffer
    assert torch.equal(g.src, again.src)


# ---------------------------------------------------------------------------------------------------------------------
# 4. an uncapped edge count beyond int32
# ---------------------------------------------------------------------------------------------------------------------
def test_cap_rowptr_on_a_wrapped_row_pointer():
    lib = _lib.load()
    full = torch.tensor([0, 2 ** 30, -2 ** 31, -2 ** 30], dtype=torch.int32, device=DEV)
    capped = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    stats = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    nbytes = lib.e3_rg_cap_workspace_bytes(5)
    assert 0 < lib.e3_rg_cap_workspace_bytes(3) <= nbytes
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    _lib.call("e3_rg_cap_rowptr", full.data_ptr(), 3, 8, capped.data_ptr(), stats.data_ptr(), ws.data_ptr(), nbytes, stream)
    assert capped.tolist() == [0, 8, 16, 24] and stats.tolist() == [3, 3 * 2 ** 30]
    assert full.tolist() == [0, 2 ** 30, -2 ** 31, -2 ** 30]
    # in place, and rows at and under the cap
    rp = torch.tensor([0, 3, 3, 11, 20, 84], dtype=torch.int32, device=DEV)
    _lib.call("e3_rg_cap_rowptr", rp.data_ptr(), 5, 8, rp.data_ptr(), stats.data_ptr(), ws.data_ptr(), nbytes, stream)
    assert rp.tolist() == [0, 3, 3, 11, 19, 27] and stats.tolist() == [2, 84]


def test_full_count_beyond_int32_builds_when_capped():
    """64 clusters of 5800 coincident points: 64 * 5800 * 5799 = 2 152 588 800 > 2^31 pairs inside r.  Every d2 is 0, so
    row i is the 16 lowest ids of its cluster other than i: an analytic expectation.  Timed: the end-to-end half of this
    test has 5 s on the device."""
    M, P = 64, 5800
    a = (torch.arange(4, dtype=torch.float32) + 0.5) / 4
    centres = torch.stack(torch.meshgrid(a, a, a, indexing="ij"), -1).reshape(M, 3)
    pos = centres.repeat_interleave(P, 0).to(DEV)
    with pytest.raises(RuntimeError, match="does not fit int32"):
        radius_graph(pos, 0.05)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g = radius_graph(pos, 0.05, max_neighbors=16)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    print(f"\ncapped build of {M} x {P} coincident points: {elapsed:.3f} s")
    assert (g.num_edges, g.truncated, g.full_edges) == (16 * M * P, M * P, M * P * (P - 1))
    assert torch.equal(g.rowptr, torch.arange(M * P + 1, dtype=torch.int32, device=DEV) * 16)
    # a cluster is one grid cell and the sort is stable: its new ids are contiguous, first id s
    same = (g.pos4[1:] == g.pos4[:-1]).all(1)
    head = torch.cat([torch.ones(1, dtype=torch.bool, device=DEV), ~same])
    assert int(head.sum()) == M
    i = torch.arange(M * P, device=DEV)
    s = torch.cummax(torch.where(head, i, torch.zeros_like(i)), 0).values
    assert torch.equal(s, (i // P) * P)
    j = torch.arange(16, device=DEV)[None, :]
    want = s[:, None] + j + (j >= (i - s)[:, None])
    assert torch.equal(g.src.view(M * P, 16).long(), want)
    assert elapsed < 5.0


# ---------------------------------------------------------------------------------------------------------------------
# 5. consumers on the directed graph
# ---------------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _min_image_geometry(monkeypatch, L):
    """The oracle's two geometry functions with the minimum image of a box of lengths L (the oracle itself knows open
    clouds only; the shift is a constant of the edge)."""
    def rel_of(pos, rowptr, src):
        dst = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
        rel = np.asarray(pos, np.float64)[src] - np.asarray(pos, np.float64)[dst]
        return rel - np.asarray(L, np.float64) * np.round(rel / np.asarray(L, np.float64)), dst

    def finish(Y, rel, dst, rowptr):
        N = len(rowptr) - 1
        A = np.zeros((N, Y.shape[1]))
        A[:, 0] = 1.0
        deg = np.diff(rowptr)
        np.add.at(A[:, 1:], dst, Y[:, 1:])
        A[deg > 0, 1:] /= deg[deg > 0, None]
        return Y, np.sqrt((rel * rel).sum(1)), A, dst

    def geo1(pos, rowptr, src):   # Y as in segnn_oracle.edge_geometry: (1, sqrt3 u), 0 for a zero vector
        rel, dst = rel_of(pos, rowptr, src)
        d = np.sqrt((rel * rel).sum(1))
        Y = np.zeros((len(src), 4))
        Y[:, 0] = 1.0
        Y[d > 0, 1:] = np.sqrt(3.0) * rel[d > 0] / d[d > 0, None]
        return finish(Y, rel, dst, rowptr)

    def geo2(pos, rowptr, src):
        from oracle import cg
        rel, dst = rel_of(pos, rowptr, src)
        return finish(cg.sh_component(2, rel), rel, dst, rowptr)

    monkeypatch.setattr(S, "edge_geometry", geo1)
    monkeypatch.setattr(S, "edge_geometry_l2", geo2)


@pytest.mark.parametrize("mode", ["open", "periodic"])
@pytest.mark.parametrize("lmax", [2, 1])
def test_segnn_on_the_capped_graph(monkeypatch, lmax, mode):
    """Hidden 32 at the bound of tests/test_parity_bench_mode_gpu.py (1e-5 of the output scale, its _rel): l_max = 2 runs the
    one-launch message kernel with owned sums, l_max = 1 its own fused kernel; then the per-product path on the same graph.
    One layer: the fp64 oracle costs about 5 s per layer on these 30 k edges, and a second layer sees the same graph."""
    H, L, k = 32, 1, 16
    perm, pos4, rowptr_c, src_c, _, _, _ = C.capped(mode, k)
    g = _gpu_graph(mode, k)
    assert np.array_equal(g.rowptr.cpu().numpy(), rowptr_c) and np.array_equal(g.src.cpu().numpy(), src_c)
    torch.manual_seed(5)
    model = SEGNN("1x0e+1x1o", H, "1x1o", L, lmax=lmax).to(DEV)
    xs = torch.randn(C.N_UNIFORM, 4, generator=torch.Generator().manual_seed(6))[torch.tensor(perm).long()]
    params = {n: v.detach().cpu().numpy() for n, v in model.state_dict().items()}
    if mode == "periodic":
        _min_image_geometry(monkeypatch, [1.0, 1.0, 1.0])
    fwd64 = S.forward_l2 if lmax == 2 else S.forward
    want = fwd64(params, H, L, "1x0e+1x1o", "1x1o", xs.double().numpy(), pos4[:, :3].astype(np.float64), rowptr_c, src_c)
    with torch.no_grad():
        assert all(l.fused and (l.fused_available() or l.fused_update_available()) for l in model.layers)
        got = model(xs.to(DEV), g).double().cpu().numpy()
        for l in model.layers:
            l.fuse_message = False
        per_product = model(xs.to(DEV), g).double().cpu().numpy()
    e_fast, e_tp = _rel(got, want), _rel(per_product, want)
    print(f"\ncapped k={k} {mode} l_max={lmax}: fused {e_fast:.2e} | per product {e_tp:.2e}")
    assert e_fast <= 1e-5, e_fast
    assert e_tp <= 1e-5, e_tp


@pytest.mark.parametrize("mode", ["open", "periodic"])
@pytest.mark.parametrize("lmax", [1, 2])
def test_edge_geometry_and_backward_on_the_directed_graph(lmax, mode):
    g = _gpu_graph(mode, 16)
    src, dst = g.src.long(), g.dst.long()
    pairs = set((dst * C.N_UNIFORM + src).tolist())
    assert any((s * C.N_UNIFORM + d) not in pairs for d, s in zip(dst[:4000].tolist(), src[:4000].tolist()))  # directed
    ny = (lmax + 1) ** 2
    pos = g.pos4[:, :3].clone().requires_grad_(True)
    Y, d, A = ops.edge_geometry(g, lmax=lmax, pos=pos)
    gen = torch.Generator(device=DEV).manual_seed(2)
    wY, wd, wA = (torch.randn(t.shape, device=DEV, generator=gen) for t in (Y, d, A))
    ((Y * wY).sum() + (d * wd).sum() + (A * wA).sum()).backward()
    p64 = g.pos4[:, :3].double().clone().requires_grad_(True)
    rel = p64[src] - p64[dst]
    if mode == "periodic":
        rel = rel - torch.round(rel.detach())   # L = 1 on every axis; the shift is a constant
    dd = rel.norm(dim=1)
    u = rel / dd[:, None]
    parts = [torch.ones_like(dd)[:, None], 3 ** 0.5 * u]
    if lmax == 2:
        x, y, z = u[:, 0], u[:, 1], u[:, 2]
        s3 = 3 ** 0.5
        parts.append(5 ** 0.5 * torch.stack([s3 * x * y, s3 * y * z, (2 * z * z - x * x - y * y) / 2, s3 * z * x,
                                             s3 / 2 * (x * x - y * y)], 1))
    Y64 = torch.cat(parts, 1)
    deg = (g.rowptr[1:] - g.rowptr[:-1]).double().clamp_min(1)
    A64 = torch.cat([torch.ones(len(deg), 1, device=DEV, dtype=torch.float64),
                     torch.zeros(len(deg), ny - 1, device=DEV, dtype=torch.float64).index_add(0, dst, Y64[:, 1:]) / deg[:, None]], 1)
    tol = 1e-6 if mode == "open" else 2e-5

    def rel_err(a, b):
        return float((a.detach() - b.detach()).abs().max() / b.detach().abs().max())

    assert rel_err(Y.double(), Y64) < tol and rel_err(A.double(), A64) < tol and rel_err(d.double(), dd) < tol
    ((Y64 * wY.double()).sum() + (dd * wd.double()).sum() + (A64 * wA.double()).sum()).backward()
    assert rel_err(pos.grad.double(), p64.grad) < 2e-5


# ---------------------------------------------------------------------------------------------------------------------
# 6. errors
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0, 65, 2.5, True])
def test_bad_cap_raises_before_any_launch(bad):
    pos = torch.tensor(C.uniform_cloud()).to(DEV)
    with pytest.raises(ValueError, match="max_neighbors"):
        radius_graph(pos, C.R_UNIFORM, C.LO, C.HI, max_neighbors=bad)
    with pytest.raises(ValueError, match="max_neighbors"):
        radius_graph(pos, C.R_UNIFORM, C.LO, C.HI, periodic=True, max_neighbors=bad)
    with pytest.raises(ValueError, match="max_neighbors"):
        radius_graph(pos, C.R_UNIFORM, cell=C.CELL.tolist(), max_neighbors=bad)


def test_abi_rejects_bad_cap_arguments_on_device_buffers():
    lib = _lib.load()
    g = _gpu_graph("open", 16)
    N = C.N_UNIFORM
    p = grid_params(C.LO, C.HI, C.R_UNIFORM)
    wbytes = lib.e3_rg_workspace_bytes(N, ctypes.byref(p))
    ws = torch.empty(wbytes, dtype=torch.uint8, device=DEV)
    cbytes = lib.e3_rg_cap_workspace_bytes(N)
    cws = torch.empty(cbytes, dtype=torch.uint8, device=DEV)
    stats = torch.zeros(2, dtype=torch.int64, device=DEV)
    rowptr, src = g.rowptr.clone(), g.src.clone()
    before = (rowptr.clone(), src.clone())
    for k in (0, 65):
        assert lib.e3_rg_cap_rowptr(rowptr.data_ptr(), N, k, rowptr.data_ptr(), stats.data_ptr(), cws.data_ptr(), cbytes,
                                    None) == 1
        assert lib.e3_rg_fill_nearest(N, ctypes.byref(p), g.pos4.data_ptr(), rowptr.data_ptr(), k, src.data_ptr(),
                                      ws.data_ptr(), wbytes, None) == 1
        assert lib.e3_rg_fill_nearest_pbc(N, ctypes.byref(p), 7, g.pos4.data_ptr(), rowptr.data_ptr(), k, src.data_ptr(),
                                          ws.data_ptr(), wbytes, None) == 1
    assert lib.e3_rg_cap_rowptr(None, N, 8, rowptr.data_ptr(), stats.data_ptr(), cws.data_ptr(), cbytes, None) == 1
    assert lib.e3_rg_cap_rowptr(rowptr.data_ptr(), N, 8, rowptr.data_ptr(), None, cws.data_ptr(), cbytes, None) == 1
    assert lib.e3_rg_fill_nearest(N, ctypes.byref(p), g.pos4.data_ptr(), rowptr.data_ptr(), 8, None, ws.data_ptr(), wbytes,
                                  None) == 1
    assert lib.e3_rg_fill_nearest(N, ctypes.byref(p), g.pos4.data_ptr(), rowptr.data_ptr(), 8, src.data_ptr(), ws.data_ptr(),
                                  wbytes - 1, None) == 1
    torch.cuda.synchronize()
    assert torch.equal(rowptr, before[0]) and torch.equal(src, before[1])

"""Helpers of tests/test_edge_table_gpu.py and tests/test_edge_cases_host.py: the graphs, the fp64 references and the per-block
error norm of the edge / node stage kernels (csrc/e3_edge_ops.hip, csrc/e3_edge_bwd.hip, csrc/e3_edge_geometry_bwd.hip).  TEST INFRASTRUCTURE ONLY; nothing
here touches the GPU at import time.

Graphs: A and B, positions(), BOX and CELL are those of tests/msg_cases.py (a row of 70 edges, degrees 1 .. 5 and 16, isolated
rows first, in the middle and last, a coincident pair joined both ways; every edge at least 1e-3 from a minimum-image tie).
W (open mode only) has more rows than one pass of the one-wave-per-row grid (4096 blocks x 4 waves = 16384): row i has source
(i + 1) % N, odd rows also (i + 4099) % N, rows 0 and N - 1 are isolated; positions are seeded uniform fp32 in the unit cube.
W cut to N = 4400 gives 1100 blocks, so the strained backward (S = 1) writes 1100 partials: one 1024-wide trip and both tail
trips of strain_partial_sum_kernel.

References: fp64, torch on the CPU (autograd for the gradients), returned as numpy."""
import functools

import numpy as np

import msg_cases as C
from msg_cases import BOX, CELL, edge_vectors, positions  # noqa: F401  (re-exported: one definition of each)
from oracle import segnn_oracle as S

MODES = C.PERIODICITY                            # open, box, cell
ROWS_PER_PASS = 16384                            # wave_grid: at most 4096 blocks of 4 waves
N_W, N_W_CUT = 16403, 4400
W_SEED = 77
LONG_ROW = 8                                     # the 70-edge row of graph A

# per block, against the fp64 reference.  Y, d, A, gate and the fp32 sum: the project's 1e-6 (tests/test_forces_gpu.py,
# tests/test_segnn_gpu.py); the periodic and strained forward at the same 1e-6: the fp32 restatement of the kernels' expressions
# (tests/test_edge_cases_host.py) stays below 5e-7 per block in every mode, unstrained (worst 3.1e-7) and strained.  Gradients:
# the project's 2e-5.
# "unwrapped" (Y and A of positions moved by up to two periods; d keeps 1e-6): coordinates of magnitude up to 4 carry an ulp of
# 2.4e-7 and the raw difference x_src - x_dst is rounded at that magnitude before the minimum image brings it back to the
# length of an edge, so the direction of a short edge is off by more than 1e-6 in fp32 whatever the kernel does.  The fp32
# restatement on these positions reads 1.40e-6 (box) and 2.11e-6 (cell) in its worst block (l = 2); the bound is twice that.
BOUND = {"Y": 1e-6, "d": 1e-6, "A": 1e-6, "strained": 1e-6, "unwrapped": 4.3e-6, "gate": 1e-6, "sum": 1e-6, "g_h": 1e-6,
         "g_pos": 2e-5, "g_strain": 2e-5}
RESTATEMENT_BOUND = 5e-7
RESTATEMENT_UNWRAPPED = 2.15e-6                  # worst block of the restatement on the unwrapped positions stays below this
BF16_REL, BF16_ABS = 2.0 ** -8, 1e-6             # |got - want| <= 2^-8 |want| + 1e-6 sum_e |m_e|: one output rounding + fp32 sums


# ---- graphs ----------------------------------------------------------------------------------------------------------
def wave_grid(n):
    """blocks of the one-wave-per-row kernels (4 waves per block), as csrc/e3_edge_ops.hip computes it"""
    return max(1, min((n + 3) // 4, 256 * 16))


@functools.lru_cache(maxsize=None)
def edges_w(n=N_W):
    """-> rowptr [n + 1], src [E], dst [E] (numpy int64) of graph W on n rows"""
    rows = []
    for i in range(n):
        if i == 0 or i == n - 1:
            rows.append([])
        elif i % 2:
            rows.append(sorted({(i + 1) % n, (i + 4099) % n}))
        else:
            rows.append([(i + 1) % n])
    deg = np.array([len(r) for r in rows], np.int64)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    src = np.array([s for r in rows for s in r], np.int64)
    return rowptr, src, np.repeat(np.arange(n), deg).astype(np.int64)


@functools.lru_cache(maxsize=None)
def positions_w(n=N_W):
    """[n, 3] fp32, uniform in the unit cube (the first n rows of the N_W cloud)"""
    return np.random.default_rng(W_SEED).random((N_W, 3)).astype(np.float32)[:n].copy()


def edges(name):
    """'A' / 'B' of msg_cases, 'W' and 'Wcut'"""
    if name == "W":
        return edges_w(N_W)
    if name == "Wcut":
        return edges_w(N_W_CUT)
    return C.edges(name)


def positions_of(name):
    return {"W": lambda: positions_w(N_W), "Wcut": lambda: positions_w(N_W_CUT)}.get(name, positions)()


def graph(name, mode="open", pos=None):
    """RadiusGraph on the device, built as tests/test_msg_table_gpu.py builds its graphs (msg_cases.graph_of)"""
    assert mode == "open" or name in ("A", "B"), "W is open mode only"
    rowptr, src, _ = edges(name)
    return C.graph_of(positions_of(name) if pos is None else pos, rowptr, src, mode)


def untouched_rows(name):
    """bool [N]: rows without an incoming edge that are nobody's source"""
    rowptr, src, _ = edges(name)
    free = np.diff(rowptr) == 0
    free[src] = False
    return free


def structure_s3():
    """[80] structure ids for S = 3 on graphs A / B: i % 3, with ids outside [0, 3) (-1 and 3) on some rows, the 70-edge row
    among them"""
    sid = np.arange(C.N, dtype=np.int64) % 3
    sid[[5, 20, 41]] = -1
    sid[[LONG_ROW, 13, 30]] = 3
    return sid


def strain_of(S_, seed=11):
    """[S, 3, 3] fp32, non-symmetric, entries uniform in [-0.05, 0.05]"""
    return ((np.random.default_rng(seed).random((S_, 3, 3)) - 0.5) * 0.1).astype(np.float32)


def lattice_shifted(mode, seed=5):
    """positions() moved by whole periods (box) or lattice vectors (cell), integers in -2 .. 2 per node, rounded to fp32 (the
    positions as stored: the reference starts from these); the coincident pair moves together"""
    k = np.random.default_rng(seed).integers(-2, 3, (C.N, 3)).astype(np.float64)
    k[C.PAIR[1]] = k[C.PAIR[0]]
    p = positions().astype(np.float64)
    p = p + (k * np.asarray(BOX, np.float64) if mode == "box" else k @ np.asarray(CELL, np.float64))
    return p.astype(np.float32)


# ---- blocks and the norm ---------------------------------------------------------------------------------------------
def sh_blocks(lmax):
    """columns of Y and A per degree l"""
    return [slice(l * l, (l + 1) * (l + 1)) for l in range(lmax + 1)]


def gate_out_blocks(ns, blocks):
    """columns of a gate output: the scalars, then each gated block (empty ones left out)"""
    out, c = [slice(0, ns)], ns
    for l, m in blocks:
        out.append(slice(c, c + m * (2 * l + 1)))
        c += m * (2 * l + 1)
    return [s for s in out if s.stop > s.start]


def gate_in_blocks(ns, blocks):
    """columns of a gate input (gradient): the scalars, the gates of each block, each gated block (empty ones left out)"""
    out, c = [slice(0, ns)], ns
    for _, m in blocks:
        out.append(slice(c, c + m))
        c += m
    for l, m in blocks:
        out.append(slice(c, c + m * (2 * l + 1)))
        c += m * (2 * l + 1)
    return [s for s in out if s.stop > s.start]


def f64(t):
    return np.asarray(t, np.float64) if isinstance(t, np.ndarray) else t.detach().float().double().cpu().numpy()


def block_errors(got, want, blocks=None):
    """per block of columns: max |got - want| / max |want| over the block and all rows (the norm of msg_cases.block_errors);
    ``blocks`` None: the whole array is one block (d, g_pos, sums)"""
    got, want = f64(got), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if blocks is None:
        got, want, blocks = got.reshape(len(got), -1), want.reshape(len(want), -1), [slice(None)]
    return [float(np.abs(got[:, s] - want[:, s]).max() / max(np.abs(want[:, s]).max(), 1e-300)) for s in blocks]


def structure_errors(got, want):
    """g_strain [S, 3, 3]: one block per structure"""
    got, want = f64(got).reshape(-1, 9), np.asarray(want, np.float64).reshape(-1, 9)
    return block_errors(got.T, want.T, [slice(s, s + 1) for s in range(len(want))])


# ---- geometry, fp64 --------------------------------------------------------------------------------------------------
def _sh_t(lmax, u):
    import torch
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    s3 = 3.0 ** 0.5
    parts = [torch.ones((len(u), 1), dtype=torch.float64), s3 * u]
    if lmax == 2:
        parts.append(5.0 ** 0.5 * torch.stack([s3 * x * y, s3 * y * z, (2 * z * z - x * x - y * y) / 2, s3 * z * x,
                                               s3 / 2 * (x * x - y * y)], 1))
    return torch.cat(parts, 1)


def _geometry_t(lmax, mode, pos_t, rowptr, src, dst, eps_t=None, structure=None):
    """torch fp64: Y [E, ny], d [E], A [N, ny] of positions pos_t [N, 3] (differentiable w.r.t. pos_t and eps_t).  The image
    of every edge is chosen from the positions as they stand (pbc_reference.min_image64 /
    triclinic_reference.min_image64_cell) and held fixed: the shift is piecewise constant."""
    import torch
    n = len(rowptr) - 1
    p = pos_t.detach().numpy()
    shift = torch.as_tensor(edge_vectors(p, src, dst, mode) - (p[src] - p[dst]))
    src_t, dst_t = torch.as_tensor(src), torch.as_tensor(dst)
    r = pos_t[src_t] - pos_t[dst_t] + shift
    if eps_t is not None:
        S_ = eps_t.shape[0]
        sid = np.zeros(n, np.int64) if structure is None else np.asarray(structure, np.int64)
        ok = (sid >= 0) & (sid < S_)                                   # ids outside [0, S): unstrained
        e = eps_t[torch.as_tensor(np.where(ok, sid, 0))[dst_t]] * torch.as_tensor(ok.astype(np.float64))[dst_t, None, None]
        r = r + torch.einsum("eab,eb->ea", e, r)
    r2 = (r * r).sum(1)
    nz = r2 > 0
    safe = torch.sqrt(torch.where(nz, r2, torch.ones_like(r2)))
    d = torch.where(nz, safe, torch.zeros_like(r2))
    u = torch.where(nz[:, None], r / safe[:, None], torch.zeros_like(r))   # u = 0 where d = 0, and so is its gradient
    Y = _sh_t(lmax, u)
    deg = torch.as_tensor(np.diff(rowptr).astype(np.float64))
    mean = torch.zeros((n, Y.shape[1] - 1), dtype=torch.float64).index_add(0, dst_t, Y[:, 1:]) / deg.clamp(min=1.0)[:, None]
    A = torch.cat([torch.ones((n, 1), dtype=torch.float64), mean], 1)      # [1, 0, ...] on an empty row
    return Y, d, A


def _as_t(a, grad=False):
    import torch
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


def geometry(lmax, mode, pos, rowptr, src, dst, strain=None, structure=None):
    """-> Y, d, A (numpy fp64) from the fp32 positions as stored; strain [S, 3, 3] applied in fp64 per dst-row structure"""
    import torch
    with torch.no_grad():
        out = _geometry_t(lmax, mode, _as_t(pos), rowptr, src, dst, None if strain is None else _as_t(strain), structure)
    return tuple(o.numpy() for o in out)


def geometry_grads(lmax, mode, pos, rowptr, src, dst, gY=None, gd=None, gA=None, strain=None, structure=None):
    """-> g_pos [N, 3], g_strain [S, 3, 3] | None: fp64 autograd of sum(Y gY) + sum(d gd) + sum(A gA)"""
    import torch
    pos_t = _as_t(pos, True)
    eps_t = None if strain is None else _as_t(strain, True)
    Y, d, A = _geometry_t(lmax, mode, pos_t, rowptr, src, dst, eps_t, structure)
    loss = pos_t.sum() * 0.0
    for out, g in ((Y, gY), (d, gd), (A, gA)):
        if g is not None:
            loss = loss + (out * _as_t(f64(g))).sum()
    grads = torch.autograd.grad(loss, [pos_t] + ([eps_t] if eps_t is not None else []), allow_unused=True)
    g_eps = None if eps_t is None else (grads[1] if grads[1] is not None else torch.zeros_like(eps_t)).numpy()
    return grads[0].numpy(), g_eps


# ---- fp32 restatement of the kernels' expressions (numpy float32, no fused multiply-add) ------------------------------
def geometry_fp32(lmax, mode, pos, src, dst, strain=None, structure=None):
    """-> Y [E, ny], d [E] in float32, in the expression order of csrc/e3_common.h (edge_rel, apply_strain) and of
    edge_geometry_kernel / edge_geometry_l2_kernel"""
    import triclinic_reference as TR
    f = np.float32
    p = np.asarray(pos, f)
    r = (p[src] - p[dst]).astype(f)
    if mode == "box":
        for a in range(3):
            L = f(BOX[a])
            inv = f(1.0) / L if L > 0 else f(0.0)
            r[:, a] = r[:, a] - L * np.rint(r[:, a] * inv)
    elif mode == "cell":
        cell = np.asarray(CELL, f)
        g, _, _ = TR.derive(cell)
        r = TR.shift(r, np.rint(TR.frac(r, g)), cell)
    if strain is not None:
        e = np.asarray(strain, f).reshape(-1, 9)
        sid = np.zeros(len(p), np.int64) if structure is None else np.asarray(structure, np.int64)
        ok = (sid >= 0) & (sid < len(e))
        e = (e[np.where(ok, sid, 0)] * ok[:, None].astype(f))[dst]
        x, y, z = r[:, 0].copy(), r[:, 1].copy(), r[:, 2].copy()
        r = np.stack([x + ((e[:, 0] * x + e[:, 1] * y) + e[:, 2] * z), y + ((e[:, 3] * x + e[:, 4] * y) + e[:, 5] * z),
                      z + ((e[:, 6] * x + e[:, 7] * y) + e[:, 8] * z)], 1).astype(f)
    d = np.sqrt((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]).astype(f)
    s3, s5 = f(1.7320508075688772), f(2.2360679774997896)
    with np.errstate(divide="ignore", invalid="ignore"):
        if lmax == 1:
            s = np.where(d > 0, s3 / d, f(0.0)).astype(f)
            Y = np.concatenate([np.ones((len(d), 1), f), s[:, None] * r], 1)
        else:
            inv = np.where(d > 0, f(1.0) / d, f(0.0)).astype(f)
            x, y, z = r[:, 0] * inv, r[:, 1] * inv, r[:, 2] * inv
            Y = np.stack([np.ones_like(x), s3 * x, s3 * y, s3 * z, (s5 * s3) * x * y, (s5 * s3) * y * z,
                          (s5 * f(0.5)) * ((f(2.0) * z * z - x * x) - y * y), (s5 * s3) * z * x,
                          (s5 * f(0.5) * s3) * (x * x - y * y)], 1)
    assert Y.dtype == f and d.dtype == f
    return Y, d


# ---- gather / segment-sum --------------------------------------------------------------------------------------------
def gather(h, src, dst, extra=None):
    h = f64(h)
    parts = [h[dst], h[src]] + ([f64(extra).reshape(len(src), -1)] if extra is not None else [])
    return np.concatenate(parts, 1)


def gather_grads(gm, D, src, dst, n):
    """-> g_h [n, D], g_extra [E, n_extra] of out = [h[dst] | h[src] | extra]"""
    gm = f64(gm)
    gh = np.zeros((n, D))
    np.add.at(gh, dst, gm[:, :D])
    np.add.at(gh, src, gm[:, D:2 * D])
    return gh, gm[:, 2 * D:]


def segment_sum(msg, dst, n):
    msg = f64(msg)
    out = np.zeros((n, msg.shape[1]))
    np.add.at(out, dst, msg)
    return out


def segment_abs_sum(msg, dst, n):
    return segment_sum(np.abs(f64(msg)), dst, n)


# ---- gates -----------------------------------------------------------------------------------------------------------
gate = S.gate
gate_blocks = S.gate_blocks


def _gate_blocks_t(x, ns, blocks):
    """oracle/segnn_oracle.gate_blocks in torch (tests/test_edge_cases_host.py holds the two together)"""
    import torch
    ng = sum(m for _, m in blocks)
    out = [x[:, :ns] * torch.sigmoid(x[:, :ns])]
    g0, c0 = ns, ns + ng
    for l, m in blocks:
        w = 2 * l + 1
        blk = x[:, c0:c0 + m * w].reshape(len(x), m, w)
        out.append((torch.sigmoid(x[:, g0:g0 + m])[:, :, None] * blk).reshape(len(x), m * w))
        g0 += m
        c0 += m * w
    return torch.cat(out, 1)


def gate_blocks_grad(x, go, ns, blocks):
    """-> g_x [B, ns + gates + wide]: fp64 autograd of sum(gate_blocks(x) go)"""
    import torch
    x_t = _as_t(f64(x), True)
    (g,) = torch.autograd.grad((_gate_blocks_t(x_t, ns, blocks) * _as_t(f64(go))).sum(), x_t)
    return g.numpy()


def layer_gate_shape(H, lmax):
    """(ns, blocks) of the gate a SEGNNLayer(H, lmax) applies, read from the layer: its ``_gate`` is called on a placeholder
    while ops.gate / ops.gate_blocks are replaced by recorders (nothing runs)"""
    from scalable_e3_gnn_amd import ops
    from scalable_e3_gnn_amd.segnn import SEGNNLayer
    seen = []
    keep = ops.gate, ops.gate_blocks
    ops.gate = lambda t, ns, nv: seen.append((int(ns), ((1, int(nv)),)))
    ops.gate_blocks = lambda t, ns, blocks: seen.append((int(ns), tuple((int(l), int(m)) for l, m in blocks)))
    try:
        SEGNNLayer(H, lmax)._gate(None)
    finally:
        ops.gate, ops.gate_blocks = keep
    assert len(seen) == 1, seen
    return seen[0]


def gate_width(ns, blocks):
    """(input width, output width)"""
    wide = sum(m * (2 * l + 1) for l, m in blocks)
    return ns + sum(m for _, m in blocks) + wide, ns + wide

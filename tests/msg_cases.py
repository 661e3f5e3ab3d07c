"""Helpers of tests/test_msg_table_gpu.py and tests/test_msg_cases_host.py: the table of message-kernel instantiations, the
literal support tables, two hand-made graphs with positions that are safe for the minimum image, the fp64 reference of one
case (oracle/segnn_oracle.message_sums on the storage-rounded inputs) and the per-block error norm.
TEST INFRASTRUCTURE ONLY.

The graphs are built by hand (80 nodes, dst-sorted edges with prescribed in-degrees, sources drawn without repetition): isolated
nodes at row 0, in the middle and at the last four rows (the ghosts of the accumulating case: sources only); degree 1; a run of
exactly 16 edges that starts on edge 16; a run of 70 edges; E = 314 (no multiple of 16); nodes 1 and 2 coincide and are joined
in both directions (d = 0: the harmonics of degree > 0 vanish).  The second graph has E = 12 < 16.  80 nodes and not 48 as in
tests/test_msg_owned_sums_gpu.py: a run of 70 edges without a repeated edge needs 70 other nodes."""
import functools

import numpy as np

import pbc_reference as P
import triclinic_reference as TR
from oracle import segnn_oracle as S

DEV = "cuda:0"
LMAX = (1, 2)
HIDDEN = (16, 32, 64)
STORAGE = ("fp32", "bf16")
PERIODICITY = ("open", "box", "cell")
NAT = ("l0e", "l1o", "l2e")                      # the class of output degree l
BOUND = {"fp32": 1e-5, "bf16": 2e-2}             # per block, against message_sums on the storage-rounded inputs

# ---- what the library answers, as literals ----
SUPPORTS_BF16 = {(1, 16): False, (1, 32): True, (1, 64): True, (2, 16): False, (2, 32): True, (2, 64): True}
# e3_msg_owned_workspace_bytes >= 0 (the weights-stationary kernel exists), per (l_max, hidden, storage)
OWNED = {(1, 16, "fp32"): False, (1, 32, "fp32"): False, (1, 64, "fp32"): False,
         (2, 16, "fp32"): False, (2, 32, "fp32"): True, (2, 64, "fp32"): False,
         (1, 32, "bf16"): False, (1, 64, "bf16"): False, (2, 32, "bf16"): True, (2, 64, "bf16"): False}
SHAPES = [(l, H) for l in LMAX for H in HIDDEN]
TABLE = [(l, H, st, per) for (l, H) in SHAPES for st in STORAGE if st == "fp32" or SUPPORTS_BF16[(l, H)]
         for per in PERIODICITY]                 # 30 instantiations of the edge kernel (+ 6 of the weights-stationary one)


def tiles_per_block_of(lmax, H):
    """every way the library runs a shape: 0 = default, < 0 = the one-wave-per-tile kernel, > 0 = chunks of the
    weights-stationary kernel where it exists"""
    return (0, -1, 1, 2, -4) if (lmax, H) == (2, 32) else (0, -1)


def width(lmax, H):
    return H * (lmax + 1) ** 2


# ---- periodicity ----
BOX = (1.0, 1.0, 0.0)                            # L per axis, 0 = open
CELL = TR.T                                      # rows = lattice vectors; dyadic entries, exact in fp32

# ---- graphs ----
N = 80
GHOSTS = 4                                       # the last rows: degree 0 in both graphs
PAIR = (1, 2)                                    # coincident nodes, joined in both directions
DEG_A = ([0,          # 0: isolated, row 0
          5,          # 1: [0, 5)
          11,         # 2: [5, 16)    ends on a tile boundary
          16,         # 3: [16, 32)   exactly one tile, starting on a multiple of 16
          1,          # 4: [32, 33)   degree 1
          15,         # 5: [33, 48)
          0,          # 6: isolated between a run that ends on edge 48 and one that starts there
          2,          # 7: [48, 50)
          70,         # 8: [50, 120)  five tiles and more
          0, 0,       # 9, 10: two isolated nodes in a row
          8,          # 11: [120, 128)
          0,          # 12: isolated
          3]          # 13: [128, 131)
         + [(i % 5) + 1 for i in range(N - GHOSTS - 14)]
         + [0] * GHOSTS)
DEG_B = [0] * N
DEG_B[3], DEG_B[4], DEG_B[20] = 4, 1, 7          # E = 12: less than one tile
DEGREES = {"A": DEG_A, "B": DEG_B}
POS_SEED = 34


@functools.lru_cache(maxsize=None)
def edges(name):
    """-> rowptr [N + 1], src [E], dst [E] (numpy int64): dst-sorted, src ascending inside a run, no self edge, no edge twice"""
    deg = DEGREES[name]
    rng = np.random.default_rng({"A": 3, "B": 4}[name])
    src = []
    for i, d in enumerate(deg):
        others = np.array([n for n in range(N) if n != i])
        s = rng.choice(others, d, replace=False)
        if name == "A" and i in PAIR:
            mate = PAIR[1 - PAIR.index(i)]
            if mate not in s:
                s[0] = mate
        src.append(np.sort(s))
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    return rowptr, np.concatenate(src).astype(np.int64), np.repeat(np.arange(N), deg).astype(np.int64)


@functools.lru_cache(maxsize=None)
def positions():
    """[N, 3] fp32, uniform in the unit cube; the seed is one at which no edge of either graph comes within 1e-3 of a
    minimum-image tie in BOX or CELL (tests/test_msg_cases_host.py asserts it)"""
    pos = np.random.default_rng(POS_SEED).random((N, 3)).astype(np.float32)
    pos[PAIR[1]] = pos[PAIR[0]]
    return pos


def fractional(rel, per):
    """displacements in units of the periods, periodic axes only: [E, 2] (box) or [E, 3] (cell)"""
    rel = np.asarray(rel, np.float64)
    if per == "box":
        ax = [a for a in range(3) if BOX[a] > 0]
        return rel[:, ax] / np.array([BOX[a] for a in ax])
    return rel @ np.linalg.inv(CELL)


def tie_distance(rel, per):
    """smallest distance of a fractional displacement from a half-integer (where rint changes the image)"""
    f = fractional(rel, per)
    return float(np.abs(f - np.floor(f) - 0.5).min())


def edge_vectors(pos, src, dst, per):
    """fp64 edge vectors of the periodicity, from the positions as stored"""
    p = np.asarray(pos, np.float64)
    rel = p[src] - p[dst]
    if per == "box":
        return P.min_image64(rel, BOX)
    if per == "cell":
        return TR.min_image64_cell(rel, CELL)
    return rel


def blocks(lmax, H):
    return [slice(H * l * l, H * (l + 1) * (l + 1)) for l in range(lmax + 1)]


def block_errors(got, want, lmax, H):
    """per output degree l: max |got_l - want_l| / max |want_l| over the columns [H l^2, H (l + 1)^2) and all rows"""
    got = np.asarray(got, np.float64) if isinstance(got, np.ndarray) else got.detach().double().cpu().numpy()
    assert got.shape == want.shape, (got.shape, want.shape)
    return [float(np.abs(got[:, s] - want[:, s]).max() / max(np.abs(want[:, s]).max(), 1e-300)) for s in blocks(lmax, H)]


def random_weights(lmax, H, rng, uneven=False):
    """(W, norms) pairs of the two message products with random weights and the default norms (numpy, host tests)"""
    from oracle import tp_oracle as T
    hid, gated = S.hidden_irreps(H, lmax)
    out = []
    for in1 in (f"{hid}+{hid}+1x0e", hid):
        sh = T.shapes(in1, gated, lmax)
        W = {c: rng.standard_normal(sh[c]) for c in T.CLASSES if sh[c]}
        out.append((W, {c: v.astype(np.float64) for c, v in T.default_norms(in1, gated, lmax).items()}))
    if uneven:
        out[1][1][NAT[lmax]] = out[1][1][NAT[lmax]] * 2.0 ** -7
    return out


# ---- device side ----
def torch_dtype(storage):
    import torch
    return {"fp32": torch.float32, "bf16": torch.bfloat16}[storage]


def make_layer(lmax, H, storage, uneven=False, seed=0):
    """A SEGNNLayer of the storage type.  ``uneven``: msg2's norm buffer of degree l_max times 2^-7 (exact in fp32 and in
    bf16): the last block of the sums then lies two orders of magnitude below the others."""
    import torch
    from scalable_e3_gnn_amd.segnn import SEGNNLayer
    torch.manual_seed(100 + 10 * H + lmax + 1000 * seed)
    layer = SEGNNLayer(H, lmax).to(torch_dtype(storage)).to(DEV)
    if uneven:
        with torch.no_grad():
            getattr(layer.msg2, "norm_" + NAT[lmax]).mul_(2.0 ** -7)
    return layer


layer = functools.lru_cache(maxsize=None)(make_layer)   # shared: tests must not change its tensors


@functools.lru_cache(maxsize=None)
def features(lmax, H, storage, seed=5):
    import torch
    return torch.randn(N, width(lmax, H), generator=torch.Generator().manual_seed(seed)).to(torch_dtype(storage)).to(DEV)


def graph_of(pos, rowptr, src, per):
    import torch
    from scalable_e3_gnn_amd.radius_graph import RadiusGraph
    n = pos.shape[0]
    pos4 = torch.zeros(n, 4)
    pos4[:, :3] = torch.as_tensor(np.asarray(pos, np.float32))
    return RadiusGraph(perm=torch.arange(n, dtype=torch.int32, device=DEV), pos4=pos4.to(DEV),
                       rowptr=torch.as_tensor(rowptr).int().to(DEV), src=torch.as_tensor(src).int().to(DEV).contiguous(),
                       num_edges=int(len(src)), grid=(1, 1, 1), box=BOX if per == "box" else None,
                       cell=tuple(float(v) for v in CELL.reshape(9)) if per == "cell" else None)


@functools.lru_cache(maxsize=None)
def graph(name, per):
    rowptr, src, _ = edges(name)
    return graph_of(positions(), rowptr, src, per)


def f64(t):
    return t.detach().float().double().cpu().numpy()


def weights_norms(layer_):
    """the (W, norms) pairs of msg1 / msg2 as stored (bf16 storage: the bf16 values), fp64"""
    from r16_cases import weights_norms as wn
    return wn(layer_.msg1), wn(layer_.msg2)


def oracle(layer_, h, lmax, H, rel, src, dst, n_nodes):
    wn1, wn2 = weights_norms(layer_)
    return S.message_sums(lmax, H, wn1, wn2, f64(h), rel, src, dst, n_nodes)


@functools.lru_cache(maxsize=None)
def reference(lmax, H, storage, per, name, uneven=False):
    """message_sums of the shared layer and features on graph ``name``, once per case; callers must not write to it"""
    _, src, dst = edges(name)
    want = oracle(layer(lmax, H, storage, uneven), features(lmax, H, storage), lmax, H,
                  edge_vectors(positions(), src, dst, per), src, dst, N)
    want.setflags(write=False)
    return want

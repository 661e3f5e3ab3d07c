"""The cases and the reference of tests/test_msg_table_gpu.py checked on the host: the hand-made graphs hold the runs they are
meant to hold, the positions keep every edge away from a minimum-image tie, the literal support tables are what the library
answers (host-only entries), and oracle/segnn_oracle.message_sums agrees with the reference-pinned closed form at l_max = 1,
is equivariant and does not see a node move by a lattice vector -- so that the reference is not wrong along with the kernels."""
import ctypes

import numpy as np
import pytest

import msg_cases as C
from oracle import cg
from oracle import l1tp_oracle as O
from oracle import segnn_oracle as S


def _rel_err(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("name", ["A", "B"])
def test_graphs_have_the_cases(name):
    rowptr, src, dst = C.edges(name)
    deg = np.diff(rowptr)
    E = len(src)
    assert len(deg) == C.N and list(deg) == C.DEGREES[name]
    assert not (src == dst).any(), "self edge"
    assert len(set(zip(src.tolist(), dst.tolist()))) == E, "an edge twice"
    assert (np.diff(dst) >= 0).all() and all((np.diff(src[rowptr[i]:rowptr[i + 1]]) > 0).all() for i in range(C.N))
    assert (deg[-C.GHOSTS:] == 0).all()
    if name == "B":
        assert 0 < E < 16
        return
    assert E == 314 and E % 16 != 0
    assert deg[0] == 0 and deg[C.N - 1] == 0 and deg[6] == 0 and deg[9] == 0 and deg[10] == 0   # row 0, row N - 1, middle
    assert deg[4] == 1
    assert deg[3] == 16 and rowptr[3] % 16 == 0                     # exactly one tile, from a multiple of 16
    assert deg[8] == 70
    a, b = C.PAIR                                                   # coincident, joined in both directions
    assert a in src[rowptr[b]:rowptr[b + 1]] and b in src[rowptr[a]:rowptr[a + 1]]
    assert (C.positions()[a] == C.positions()[b]).all()
    ghost = src >= C.N - C.GHOSTS                                   # the accumulating case needs both kinds of edges
    assert 0 < ghost.sum() < E and len(set(dst[ghost].tolist())) > 1


@pytest.mark.parametrize("per", ["box", "cell"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_positions_are_safe_for_the_minimum_image(name, per):
    _, src, dst = C.edges(name)
    pos = C.positions()
    assert pos.dtype == np.float32 and pos.min() >= 0 and pos.max() < 1
    raw = pos.astype(np.float64)[src] - pos.astype(np.float64)[dst]
    rel = C.edge_vectors(pos, src, dst, per)
    share = float((np.abs(rel - raw).max(1) > 0).mean())
    tie = C.tie_distance(raw, per)
    print(f"graph {name}, {per}: {share:.0%} of the edges wrapped, nearest tie {tie:.2e}")
    assert share >= 0.25
    assert tie >= 1e-3     # fp32 rintf and the fp64 reference pick the same image
    assert (np.asarray(C.CELL, np.float32).astype(np.float64) == C.CELL).all() and all(float(np.float32(v)) == v for v in C.BOX)
    assert sum(v > 0 for v in C.BOX) == 2                           # one open axis


def test_support_tables_match_the_library():
    from scalable_e3_gnn_amd import _lib
    lib = _lib.load()
    assert sorted(C.SUPPORTS_BF16) == sorted(C.SHAPES)
    assert {k for k, v in C.SUPPORTS_BF16.items() if not v} == {(l, 16) for l in C.LMAX}
    assert {k for k, v in C.OWNED.items() if v} == {(2, 32, "fp32"), (2, 32, "bf16")}
    assert sorted(C.OWNED) == sorted({(l, H, st) for (l, H, st, _) in C.TABLE})
    assert len(C.TABLE) == 30
    code = {"fp32": _lib.E3_F32, "bf16": _lib.E3_BF16}
    for (lmax, H) in C.SHAPES:
        h = ctypes.c_void_p()
        assert lib.e3_msg_plan_create(lmax, H, ctypes.byref(h)) == 0
        try:
            assert lib.e3_msg_supports(h, _lib.E3_F32) == 1
            assert bool(lib.e3_msg_supports(h, _lib.E3_BF16)) == C.SUPPORTS_BF16[(lmax, H)], (lmax, H)
            assert lib.e3_msg_supports(h, _lib.E3_F64) == 0
            for st in C.STORAGE:
                owned = C.OWNED.get((lmax, H, st), False)
                for E in (0, 12, 314, 100000):
                    for tpb in (0, 1, 2, 16):
                        b = int(lib.e3_msg_owned_workspace_bytes(h, E, code[st], tpb))
                        assert (b >= 0) == owned and (owned or b == -1), (lmax, H, st, E, tpb, b)
                    for tpb in (-1, -4):
                        assert int(lib.e3_msg_owned_workspace_bytes(h, E, code[st], tpb)) == -1, (lmax, H, st, E, tpb)
        finally:
            assert lib.e3_msg_plan_destroy(h) == 0


def test_block_errors_and_the_uneven_case():
    lmax, H = 2, 16
    want = np.random.default_rng(0).standard_normal((7, C.width(lmax, H)))
    got = want.copy()
    got[3, H * 4 + 5] += 1e-3 * np.abs(want[:, H * 4:]).max()
    assert C.block_errors(got, want, lmax, H)[:2] == [0.0, 0.0]
    assert abs(C.block_errors(got, want, lmax, H)[2] - 1e-3) < 1e-12
    # the uneven case: the last block two orders of magnitude below the others
    _, src, dst = C.edges("A")
    rng = np.random.default_rng(1)
    h = rng.standard_normal((C.N, C.width(lmax, H)))
    rel = C.edge_vectors(C.positions(), src, dst, "open")
    even = S.message_sums(lmax, H, *C.random_weights(lmax, H, np.random.default_rng(2)), h, rel, src, dst, C.N)
    uneven = S.message_sums(lmax, H, *C.random_weights(lmax, H, np.random.default_rng(2), uneven=True), h, rel, src, dst, C.N)
    tops = [float(np.abs(uneven[:, s]).max()) for s in C.blocks(lmax, H)]
    assert tops[2] < 0.02 * min(tops[:2])
    assert np.array_equal(uneven[:, :4 * H], even[:, :4 * H]) and _rel_err(uneven[:, 4 * H:] * 2.0 ** 7, even[:, 4 * H:]) < 1e-14


def _closed_form_chain(H, wn1, wn2, h, rel, src, dst, n_nodes):
    """the l_max = 1 message function on l1tp_oracle.forward_closed_form, as segnn_oracle.forward builds it"""
    hid, gated = f"{H}x0e+{H}x1o", f"{H}x0e+{H}x0e+{H}x1o"
    d = np.sqrt((rel * rel).sum(1))
    Y = np.zeros((len(src), 4))
    Y[:, 0] = 1.0
    nz = d > 0
    Y[nz, 1:] = np.sqrt(3.0) * rel[nz] / d[nz, None]

    def tp(wn, in1, ii):
        W = {c: wn[0][c] for c in O.CLASSES if c in wn[0]}
        return O.forward_closed_form(O.make_layout(ii, gated), in1, Y, W, {c: wn[1][c] for c in O.CLASSES})

    m = np.concatenate([h[dst], h[src], d[:, None]], 1)
    m = S.gate(tp(wn1, m, f"{hid}+{hid}+1x0e"), H, H)
    m = S.gate(tp(wn2, m, hid), H, H)
    a = np.zeros((n_nodes, h.shape[1]))
    np.add.at(a, dst, m)
    return a


@pytest.mark.parametrize("per", C.PERIODICITY)
@pytest.mark.parametrize("H", [16, 32])
def test_lmax1_agrees_with_the_closed_form(H, per):
    _, src, dst = C.edges("A")
    rng = np.random.default_rng(10 + H)
    wn1, wn2 = C.random_weights(1, H, rng)
    h = rng.standard_normal((C.N, 4 * H))
    rel = C.edge_vectors(C.positions(), src, dst, per)
    got, m = S.message_sums(1, H, wn1, wn2, h, rel, src, dst, C.N, return_messages=True)
    want = _closed_form_chain(H, wn1, wn2, h, rel, src, dst, C.N)
    assert m.shape == (len(src), 4 * H) and got.shape == (C.N, 4 * H)
    assert _rel_err(got, want) < 1e-12
    assert (got[np.diff(C.edges("A")[0]) == 0] == 0).all()


def _rotate_rows(x, lmax, H, R):
    """rows [.., (l_max + 1)^2 H] (per degree: H channels x (2 l + 1) components) under the rotation R"""
    out = x.copy()
    for l, s in enumerate(C.blocks(lmax, H)):
        D = cg.rotation_matrices(l, R)
        out[:, s] = (x[:, s].reshape(len(x), H, 2 * l + 1) @ D.T).reshape(len(x), -1)
    return out


@pytest.mark.parametrize("lmax", C.LMAX)
def test_message_sums_are_equivariant(lmax):
    H = 16
    _, src, dst = C.edges("A")
    rng = np.random.default_rng(20 + lmax)
    wn1, wn2 = C.random_weights(lmax, H, rng)
    h = rng.standard_normal((C.N, C.width(lmax, H)))
    R = cg.random_rotation(rng)
    pos = C.positions().astype(np.float64)
    a = S.message_sums(lmax, H, wn1, wn2, h, pos[src] - pos[dst], src, dst, C.N)
    pr = pos @ R.T
    b = S.message_sums(lmax, H, wn1, wn2, _rotate_rows(h, lmax, H, R), pr[src] - pr[dst], src, dst, C.N)
    want = _rotate_rows(a, lmax, H, R)
    assert _rel_err(want, a) > 0.1          # the rotation does something
    for s in C.blocks(lmax, H):
        assert _rel_err(b[:, s], want[:, s]) < 1e-11


@pytest.mark.parametrize("per", ["box", "cell"])
@pytest.mark.parametrize("lmax", C.LMAX)
def test_a_lattice_vector_changes_nothing(lmax, per):
    H = 16
    _, src, dst = C.edges("A")
    rng = np.random.default_rng(30 + lmax)
    wn1, wn2 = C.random_weights(lmax, H, rng)
    h = rng.standard_normal((C.N, C.width(lmax, H)))
    pos = C.positions().astype(np.float64)
    a = S.message_sums(lmax, H, wn1, wn2, h, C.edge_vectors(pos, src, dst, per), src, dst, C.N)
    moved = pos.copy()
    node = 8                                # the hub: 70 incoming edges, and a source of others
    assert (src == node).any()
    moved[node] += np.array([1.0, -1.0, 0.0]) * np.array(C.BOX) if per == "box" else np.array([1.0, -2.0, 1.0]) @ C.CELL
    rel = C.edge_vectors(moved, src, dst, per)
    raw = moved[src] - moved[dst]
    assert np.abs(raw - (pos[src] - pos[dst])).max() >= 1.0
    b = S.message_sums(lmax, H, wn1, wn2, h, rel, src, dst, C.N)
    for s in C.blocks(lmax, H):
        assert _rel_err(b[:, s], a[:, s]) < 1e-11

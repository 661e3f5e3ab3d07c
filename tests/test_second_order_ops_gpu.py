"""Second derivatives, op by op: the backward of every first-order backward of the differentiable chain against fp64 torch
autograd of the same op written in torch.

Tensor products (composition of the existing entries, no new kernel), the second-order gate (e3_gate_blocks_backward2), the
tangent of the edge geometry (e3_edge_geometry_jvp, open / box / cell) and the second derivative of the envelope
(e3_cutoff_envelope_backward2) with the weighted segment sum.  Norm: max |got - want| / max |want| per tensor.  Bounds: the
fp64 cases 1e-10 (fp64 rounding through sums of a few hundred terms is ~1e-13), the fp32 cases 2e-5, the project's bound
for derivatives of fp32 kernels."""
import functools

import numpy as np
import pytest
import torch

import models  # noqa: F401
import msg_cases as MC
from envelope_reference import envelope64
from models.segnn.l1_tensor_prod import L1TensorProduct
from oracle import tp_oracle as T
from scalable_e3_gnn_amd import ops
from scalable_e3_gnn_amd.tensor_product import _BWD_GEMM_MIN_ROWS, SHTensorProduct

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = {torch.float32: 2e-5, torch.float64: 1e-10}

HID = "16x0e+16x1o+16x2e"
GATED = "16x0e+32x0e+16x1o+16x2e"
PRODUCTS = {   # name -> (in1 irreps, out irreps, lmax_sh, class)
    "msg1": (f"{HID}+{HID}+1x0e", GATED, 2, SHTensorProduct),
    "upd2": (HID, HID, 2, SHTensorProduct),
    "readout": (HID, "1x0e", 2, SHTensorProduct),
    "l1tp": ("16x0e+16x1o", "16x0e+16x0e+16x1o", 1, L1TensorProduct),
}


def rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))


def _make(name, dtype):
    ii, oi, lsh, cls = PRODUCTS[name]
    torch.manual_seed(3)
    mod = cls(ii, oi) if cls is L1TensorProduct else cls(ii, oi, lmax_sh=lsh)
    return mod.to(DEV).to(dtype)


def _double_backward(forward, x, y, ws, g, c1, c2, cws, need_y=True):
    """grad of s = <c1, g_x> + <c2, g_y> + sum <cW, g_W>, (g_x, g_y, g_W) = grad(<g, out>, create_graph), w.r.t. x, y, W, g"""
    firsts = [x] + ([y] if need_y else []) + list(ws)
    gr = torch.autograd.grad((g * forward(x, y)).sum(), firsts, create_graph=True)
    cs = [c1] + ([c2] if need_y else []) + list(cws)
    s = sum((c * t).sum() for c, t in zip(cs, gr))
    return firsts + [g], torch.autograd.grad(s, firsts + [g])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("B,only_in1", [(37, False), (600, False), (600, True)], ids=["B37", "B600", "B600-in1-W"])
@pytest.mark.parametrize("name", list(PRODUCTS))
def test_tensor_product_double_backward(name, B, only_in1, dtype):
    assert 37 < _BWD_GEMM_MIN_ROWS <= 600
    ii, oi, lsh, _ = PRODUCTS[name]
    mod = _make(name, dtype)
    names = [n for n, _ in mod.named_parameters()]
    gen = torch.Generator().manual_seed(11)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    x, y = rnd(B, mod.in1_dim), rnd(B, mod.in2_dim)
    g = rnd(B, mod.iro.dim)
    c1, c2 = rnd(B, mod.in1_dim), rnd(B, mod.in2_dim)
    cws = [rnd(*p.shape) for p in mod.parameters()]
    need_y = not only_in1
    dev = lambda t, grad=True: t.to(dtype).to(DEV).requires_grad_(grad)
    xg, yg = dev(x), dev(y, need_y)
    with torch.no_grad():
        before = mod(xg, yg).clone()
    _, got = _double_backward(mod, xg, yg, list(mod.parameters()), dev(g), dev(c1, False), dev(c2, False),
                              [dev(c, False) for c in cws], need_y)
    # the same product in fp64 torch on the CPU
    W = {n[len("weights_"):]: p.detach().double().cpu().requires_grad_(True) for n, p in mod.named_parameters()}
    norms = {c: getattr(mod, "norm_" + c).double().cpu() if hasattr(mod, "norm_" + c) else torch.ones(0, dtype=torch.float64)
             for c in T.CLASSES}
    fwd = lambda a, b: T.forward_torch_cpu(ii, oi, lsh, a, b, W, norms)
    x64, y64 = x.clone().requires_grad_(True), y.clone().requires_grad_(need_y)
    _, want = _double_backward(fwd, x64, y64, [W[n[len("weights_"):]] for n in names], g.clone().requires_grad_(True),
                               c1, c2, cws, need_y)
    labels = ["x"] + (["y"] if need_y else []) + names + ["g"]
    errs = {k: rel(a, b) for k, a, b in zip(labels, got, want)}
    print(f"\n{name} B={B} {dtype}: " + " ".join(f"{k}={v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) < BOUND[dtype], errs
    # the packed-weight cache of the module's own weights was not disturbed: the next plain forward is bit-equal
    with torch.no_grad():
        assert torch.equal(mod(xg, yg), before)


def test_broadcast_in2_is_refused_not_summed_wrongly():
    mod = _make("upd2", torch.float32)
    x = torch.randn(40, mod.in1_dim, device=DEV, requires_grad=True)
    y = torch.randn(1, mod.in2_dim, device=DEV, requires_grad=True)
    (gx,) = torch.autograd.grad(mod(x, y).sum(), [x], create_graph=True)
    with pytest.raises(NotImplementedError, match="broadcast"):
        gx.square().sum().backward()


def test_third_derivative_raises():
    mod = _make("readout", torch.float32)
    x = torch.randn(20, mod.in1_dim, device=DEV, requires_grad=True)
    y = torch.randn(20, mod.in2_dim, device=DEV, requires_grad=True)
    (gx,) = torch.autograd.grad(mod(x, y).sum(), [x], create_graph=True)
    (gy,) = torch.autograd.grad(gx.square().sum(), [y], create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|differentiable twice"):
        gy.square().sum().backward()


# ---------------------------------------------------------------------------------------------------------------------
# gate
# ---------------------------------------------------------------------------------------------------------------------
def _gate64(x, ns, blocks):
    ng = sum(m for _, m in blocks)
    out, g0, c0 = [torch.nn.functional.silu(x[:, :ns])], ns, ns + ng
    for l, m in blocks:
        w = 2 * l + 1
        out.append((torch.sigmoid(x[:, g0:g0 + m])[:, :, None] * x[:, c0:c0 + m * w].reshape(-1, m, w)).reshape(-1, m * w))
        g0, c0 = g0 + m, c0 + m * w
    return torch.cat(out, 1)


def _gate_inputs(B, ns, blocks, seed=5):
    ng, wide = sum(m for _, m in blocks), sum(m * (2 * l + 1) for l, m in blocks)
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(B, ns + ng + wide, generator=gen, dtype=torch.float64) * 1.5,
            torch.randn(B, ns + wide, generator=gen, dtype=torch.float64),
            torch.randn(B, ns + ng + wide, generator=gen, dtype=torch.float64))


@pytest.mark.parametrize("B,ns,blocks,entry", [(70, 4, ((1, 2), (2, 2)), "gate_blocks"), (70, 16, ((1, 16), (2, 16)), "gate_blocks"),
                                               (70, 16, ((1, 16),), "gate")], ids=["small", "H16-l2", "H16-l1"])
def test_gate_double_backward(B, ns, blocks, entry):
    x, go, c = _gate_inputs(B, ns, blocks)

    def run(fwd, x, go, c):
        (gi,) = torch.autograd.grad(fwd(x), [x], go, create_graph=True)
        return torch.autograd.grad((c * gi).sum(), [x, go])

    dev = lambda t: t.float().to(DEV).requires_grad_(True)
    hip = (lambda t: ops.gate(t, ns, blocks[0][1])) if entry == "gate" else (lambda t: ops.gate_blocks(t, ns, blocks))
    got = run(hip, dev(x), dev(go), c.float().to(DEV))
    want = run(lambda t: _gate64(t, ns, blocks), x.clone().requires_grad_(True), go.clone().requires_grad_(True), c)
    errs = [rel(a, b) for a, b in zip(got, want)]
    print(f"\ngate {entry} ns={ns} blocks={blocks}: cot(x) {errs[0]:.1e} cot(go) {errs[1]:.1e}")
    assert max(errs) < 2e-5, errs


def test_gate_backward2_row_strides_and_nan_padding():
    ns, blocks = 4, ((1, 2), (2, 2))
    x, go, c = (t.float().to(DEV) for t in _gate_inputs(70, ns, blocks, seed=6))
    want = ops._gate_blocks_backward2_raw(x, go, c, ns, blocks)

    def padded(t, pad):
        buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), device=DEV)
        buf[:, :t.shape[1]] = t
        return buf[:, :t.shape[1]]

    xs, gs, cs = padded(x, 3), padded(go, 5), padded(c, 7)
    assert xs.stride(0) > xs.shape[1] and not xs.is_contiguous()
    got = ops._gate_blocks_backward2_raw(xs, gs, cs, ns, blocks)
    for a, b in zip(got, want):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    # one output alone
    only_go, none = ops._gate_blocks_backward2_raw(xs, gs, cs, ns, blocks, want_go=True, want_x=False)
    assert none is None and torch.equal(only_go, want[0])


# ---------------------------------------------------------------------------------------------------------------------
# geometry tangent
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tangent_reference(per, lmax):
    """fp64: (dY [E, ny], dd [E], dA [N, ny]) along the field V on graph A, zeros at d = 0 and in empty rows"""
    rowptr, src, dst = MC.edges("A")
    relv = MC.edge_vectors(MC.positions(), src, dst, per)
    V = _field()
    nz = np.linalg.norm(relv, axis=1) > 0
    from oracle.segnn_oracle import sh_component_torch
    r = torch.as_tensor(relv[nz])
    t = torch.as_tensor(V[src] - V[dst])[nz]
    _, (dYn, ddn) = torch.autograd.functional.jvp(lambda q: sh_component_torch(lmax, q), (r,), (t,))
    ny = (lmax + 1) ** 2
    dY = torch.zeros(len(src), ny, dtype=torch.float64)
    dd = torch.zeros(len(src), dtype=torch.float64)
    dY[torch.as_tensor(nz)], dd[torch.as_tensor(nz)] = dYn, ddn
    deg = torch.as_tensor(np.diff(rowptr)).double().clamp_min(1)
    dA = torch.zeros(MC.N, ny, dtype=torch.float64).index_add(0, torch.as_tensor(dst), dY) / deg[:, None]
    return dY, dd, dA


def _field():
    return np.random.default_rng(8).standard_normal((MC.N, 3))


@pytest.mark.parametrize("per", MC.PERIODICITY)
@pytest.mark.parametrize("lmax", [1, 2])
def test_edge_geometry_tangent(lmax, per):
    g = MC.graph("A", per)
    rowptr, src, dst = MC.edges("A")
    dY64, dd64, dA64 = _tangent_reference(per, lmax)
    v = torch.as_tensor(_field()).float().to(DEV)
    dY, dd, dA = ops._edge_geometry_jvp_raw(g.pos4, g, lmax, v)
    errs = (rel(dY, dY64), rel(dd, dd64), rel(dA, dA64))
    print(f"\ntangent l_max={lmax} {per}: dY {errs[0]:.1e} dd {errs[1]:.1e} dA {errs[2]:.1e}")
    assert max(errs) < 2e-5, errs
    # column 0 (Y_0 = 1, A_0 = 1), the coincident pair and the rows without edges: exact zeros
    zero_d = torch.as_tensor(np.linalg.norm(MC.edge_vectors(MC.positions(), src, dst, per), axis=1) == 0).to(DEV)
    assert int(zero_d.sum()) == 2
    empty = torch.as_tensor(np.diff(rowptr) == 0).to(DEV)
    assert int(empty.sum()) >= 7 and np.diff(rowptr).max() == 70
    assert not dY[:, 0].any() and not dA[:, 0].any() and not dY[zero_d].any() and not dd[zero_d].any() and not dA[empty].any()
    # each output alone (NULL for the others) is the same bits; dA is bit-equal on a second run
    assert torch.equal(ops._edge_geometry_jvp_raw(g.pos4, g, lmax, v, True, False, False)[0], dY)
    assert torch.equal(ops._edge_geometry_jvp_raw(g.pos4, g, lmax, v, False, True, False)[1], dd)
    alone = ops._edge_geometry_jvp_raw(g.pos4, g, lmax, v, False, False, True)
    assert alone[0] is None and alone[1] is None and torch.equal(alone[2], dA)
    # through autograd: the backward of the geometry's backward w.r.t. the three output gradients is this tangent
    pos = g.pos4[:, :3].clone().requires_grad_(True)
    outs = ops.edge_geometry(g, lmax=lmax, pos=pos)
    seeds = [torch.randn_like(o).requires_grad_(True) for o in outs]
    (gpos,) = torch.autograd.grad(outs, [pos], seeds, create_graph=True)
    cots = torch.autograd.grad((gpos * v).sum(), seeds)
    assert all(torch.equal(a, b) for a, b in zip(cots, (dY, dd, dA)))


def test_edge_geometry_tangent_without_edges():
    g = MC.graph_of(MC.positions(), np.zeros(MC.N + 1, np.int64), np.zeros(0, np.int64), "open")
    dY, dd, dA = ops._edge_geometry_jvp_raw(g.pos4, g, 2, torch.randn(MC.N, 3, device=DEV))
    assert dY.shape == (0, 9) and dd.shape == (0,) and dA.shape == (MC.N, 9) and not dA.any()
    pos = g.pos4[:, :3].clone().requires_grad_(True)
    A = ops.edge_geometry(g, lmax=2, pos=pos)[2]
    seed = torch.randn_like(A).requires_grad_(True)
    (gpos,) = torch.autograd.grad(A, [pos], seed, create_graph=True)
    (cot,) = torch.autograd.grad(gpos.sum(), [seed])
    assert not cot.any()


# ---------------------------------------------------------------------------------------------------------------------
# envelope and weighted sum
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [2, 6])
def test_envelope_and_weighted_sum_double_backward(p):
    g = MC.graph("A", "open")
    rowptr, src, dst = MC.edges("A")
    E, D, r_c = len(src), 20, 0.75
    gen = torch.Generator().manual_seed(9)
    d = (torch.rand(E, generator=gen, dtype=torch.float64) * 0.9).float().double()   # fp32-exact values, some beyond r_c
    d[0], d[1], d[2], d[3], d[4], d[5] = 0.0, r_c, r_c * (1 - 2.0 ** -20), float(np.nextafter(np.float32(r_c), np.float32(0))), 0.8, 2.0
    msg = torch.randn(E, D, generator=gen, dtype=torch.float64)
    ga = torch.randn(MC.N, D, generator=gen, dtype=torch.float64)
    cm, cd = torch.randn(E, D, generator=gen, dtype=torch.float64), torch.randn(E, generator=gen, dtype=torch.float64)
    outside = d >= float(np.float32(r_c))
    assert int(outside.sum()) > 10 and int((~outside).sum()) > 100

    def run(agg_of, msg, d, ga, cm, cd):
        gm, gd = torch.autograd.grad(agg_of(msg, d), [msg, d], ga, create_graph=True)
        return torch.autograd.grad((cm * gm).sum() + (cd * gd).sum(), [msg, d, ga])

    dev = lambda t, grad=True: t.float().to(DEV).requires_grad_(grad)
    got = run(lambda m, dd: ops.segment_sum(m, g, weight=ops.cutoff_envelope(dd, r_c, p)), dev(msg), dev(d), dev(ga),
              dev(cm, False), dev(cd, False))
    dst_t = torch.as_tensor(dst)
    rc32 = float(np.float32(r_c))
    want = run(lambda m, dd: torch.zeros(MC.N, D, dtype=torch.float64).index_add(0, dst_t, envelope64(dd, rc32, p)[:, None] * m),
               msg.clone().requires_grad_(True), d.clone().requires_grad_(True), ga.clone().requires_grad_(True), cm, cd)
    errs = [rel(a, b) for a, b in zip(got, want)]
    print(f"\nenvelope p={p} + weighted sum: cot(msg) {errs[0]:.1e} cot(d) {errs[1]:.1e} cot(ga) {errs[2]:.1e}")
    assert max(errs) < 2e-5, errs
    out = outside.to(DEV)
    assert not got[1][out].any() and not got[0][out].any()      # exact zeros at and beyond the cutoff
    assert float(want[1][outside].abs().max()) == 0.0

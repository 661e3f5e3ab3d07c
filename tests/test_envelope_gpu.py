"""The cutoff envelope on the GPU (include/e3gnn.h: e3_cutoff_envelope, e3_segment_sum_weighted and their backward;
ops.cutoff_envelope / segment_sum(weight=) / enveloped_node_attr; SEGNN(envelope=), the energy models' skin=).

The kernels against fp64 formulas with bounds from the number formats, their bit-level contracts (exact zeros beyond the
cutoff, run-to-run equality, weight 1 = the plain sum), the models against the fp64 restatement
(tests/envelope_reference.py) with the tolerances of tests/test_stress_gpu.py, and the skin invariance of the models."""
import contextlib
import warnings

import numpy as np
import pytest
import torch

import envelope_reference as ER
import triclinic_reference as TR
from scalable_e3_gnn_amd import ops
from scalable_e3_gnn_amd.batched import BatchedEnergyModel, PeriodicEnergyModel, batched_radius_graph
from scalable_e3_gnn_amd.radius_graph import RadiusGraph, radius_graph
from scalable_e3_gnn_amd.segnn import SEGNN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS32 = 2.0 ** -23
R, SKIN, P_ENV = 0.2, 0.05, 6
BOX = ([0, 0, 0], [1, 1, 1])


def rel(a, b):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _dyadic(n, seed):
    return (np.random.default_rng(seed).integers(0, 1 << 16, size=(n, 3)) / float(1 << 16)).astype(np.float32)


@contextlib.contextmanager
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # "the unfused differentiable chain runs": what is used here
        yield


# ---------------------------------------------------------------------------------------------------------------------
# 1: the envelope kernels
# ---------------------------------------------------------------------------------------------------------------------
def _envelope_inputs(r_c):
    rc32 = np.float32(r_c)
    special = np.array([0.0, rc32, np.nextafter(rc32, np.float32(np.inf)), np.nextafter(rc32, np.float32(0)),
                        np.float32(2) * rc32, np.float32(1e-30), np.float32(0.5) * rc32], np.float32)
    rnd = (np.random.default_rng(0).random(5000) * 1.3 * float(rc32)).astype(np.float32)
    return torch.as_tensor(np.concatenate([special, rnd])).to(DEV), float(rc32)


@pytest.mark.parametrize("p", [2, 6, 16])
def test_envelope_forward_and_backward_vs_fp64(p):
    d, rc = _envelope_inputs(R)
    d.requires_grad_(True)
    w = ops.cutoff_envelope(d, rc, p)
    gw = torch.randn(d.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    (gd,) = torch.autograd.grad(w, [d], gw)
    d64 = d.detach().double()
    w64 = ER.envelope64(d64, rc, p)
    err = float((w.detach().double() - w64).abs().max())
    print(f"p={p}: max |dw| = {err:.3e}")
    assert err <= 2e-6, err
    beyond = d.detach() >= rc
    assert int(beyond.sum()) >= 3
    assert torch.all(w.detach()[beyond] == 0.0) and torch.all(gd[beyond] == 0.0)
    assert float(w.detach()[0]) == 1.0 and float(gd[0]) == 0.0  # d = 0
    # backward: du/dd(x) / r_c with x = fl(d fl(1 / r_c)) off by at most 2^-22 (two roundings of a number <= 1), which moves
    # u' by max |u''| 2^-22; the p + 4 operations of the product each add a relative 2^-24 of at most max |u'|
    xs = torch.linspace(0, 1, 20001, dtype=torch.float64, requires_grad=True)
    u1 = ER.envelope_derivative64(xs, 1.0, p)
    (u2,) = torch.autograd.grad(u1.sum(), [xs])
    bound = gw.double().abs() / rc * (float(u2.abs().max()) * 2.0 ** -22 + (p + 4) * 2.0 ** -23 * float(u1.detach().abs().max()))
    gd64 = gw.double() * ER.envelope_derivative64(d64, rc, p)
    gd64[beyond] = 0.0
    excess = float(((gd.double() - gd64).abs() - bound).max())
    print(f"p={p}: max |dg_d| / bound = {float(((gd.double() - gd64).abs() / bound.clamp_min(1e-300)).max()):.3f}")
    assert excess <= 0.0, excess
    assert float(gd.abs().max()) > 0.1
    # without grad: the same forward kernel, bit for bit
    with torch.no_grad():
        assert torch.equal(ops.cutoff_envelope(d.detach(), rc, p), w.detach())


# ---------------------------------------------------------------------------------------------------------------------
# 2-3: the weighted segment sum and its backward
# ---------------------------------------------------------------------------------------------------------------------
N_ROWS = 300


def _csr_graph():
    """300 rows; degrees 0 (first, last and some others), 1, 64, 65, 70, 129 and small random ones."""
    rng = np.random.default_rng(2)
    deg = rng.integers(0, 12, N_ROWS)
    deg[[0, 7, N_ROWS - 1]] = 0
    deg[[1, 8]] = 1
    deg[2], deg[3], deg[4], deg[5], deg[6] = 70, 129, 64, 65, 3
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    E = int(rowptr[-1])
    g = RadiusGraph(perm=torch.arange(N_ROWS, dtype=torch.int32, device=DEV), pos4=torch.zeros(N_ROWS, 4, device=DEV),
                    rowptr=torch.as_tensor(rowptr).to(DEV), src=torch.zeros(E, dtype=torch.int32, device=DEV),
                    num_edges=E, grid=None)
    return g, torch.as_tensor(deg).to(DEV), E


def _operands(D, layout, seed):
    """msg [E, D] in one of three layouts: contiguous, a row stride above D (ld_msg > D), and a column slice that starts one
    element into a wider buffer (base pointer 4 bytes off a 16-byte boundary: the 4-byte path)."""
    g, deg, E = _csr_graph()
    gen = torch.Generator(device=DEV).manual_seed(seed)
    if layout == "contiguous":
        msg = torch.randn(E, D, device=DEV, generator=gen)
    elif layout == "padded":
        msg = torch.randn(E, D + 8, device=DEV, generator=gen)[:, :D]
    else:
        msg = torch.randn(E, D + 4, device=DEV, generator=gen)[:, 1:D + 1]
        assert msg.data_ptr() % 16 == 4
    w = torch.rand(E, device=DEV, generator=gen) * 1.5
    return g, deg, msg, w


CASES = [(D, "contiguous") for D in (1, 4, 9, 63, 64, 65, 144, 288)] + [(288, "padded"), (144, "slice"), (288, "slice")]


@pytest.mark.parametrize("D,layout", CASES)
def test_weighted_segment_sum(D, layout):
    g, deg, msg, w = _operands(D, layout, 3)
    dst = g.dst.long()
    agg = ops.segment_sum(msg, g, weight=w)
    assert agg.shape == (N_ROWS, D)
    wm = w.double()[:, None] * msg.double()
    want = torch.zeros(N_ROWS, D, dtype=torch.float64, device=DEV).index_add(0, dst, wm)
    mag = torch.zeros(N_ROWS, D, dtype=torch.float64, device=DEV).index_add(0, dst, wm.abs())
    # deg fmafs into one accumulator: each rounds a partial sum that is at most the row's sum of |w m|
    bound = deg.double()[:, None] * EPS32 * mag
    assert torch.all((agg.double() - want).abs() <= bound), float(((agg.double() - want).abs() - bound).max())
    assert torch.all(agg[deg == 0] == 0.0)
    assert torch.equal(agg, ops.segment_sum(msg, g, weight=w))  # bit-equal run to run
    # weight 1: the plain sum, bit for bit
    assert torch.equal(ops.segment_sum(msg, g, weight=torch.ones_like(w)), ops.segment_sum(msg, g))


@pytest.mark.parametrize("D,layout", CASES)
def test_weighted_segment_sum_backward(D, layout):
    g, deg, msg, w = _operands(D, layout, 4)
    dst = g.dst.long()
    gen = torch.Generator(device=DEV).manual_seed(5)
    ga = torch.randn(N_ROWS, D, device=DEV, generator=gen)
    runs = []
    for _ in range(2):
        m, ww = msg.detach().requires_grad_(True), w.detach().requires_grad_(True)
        runs.append(torch.autograd.grad(ops.segment_sum(m, g, weight=ww), [m, ww], ga))
    gm, gwt = runs[0]
    assert torch.equal(gm, w[:, None] * ga[dst])  # one rounding per element
    prod = msg.double() * ga.double()[dst]
    bound = D * EPS32 * prod.abs().sum(1)
    assert torch.all((gwt.double() - prod.sum(1)).abs() <= bound)
    assert float(gwt.abs().max()) > 0
    assert torch.equal(runs[1][0], gm) and torch.equal(runs[1][1], gwt)  # bit-equal run to run
    # only msg needs a gradient: g_w = NULL, the same g_msg
    m = msg.detach().requires_grad_(True)
    (gm_only,) = torch.autograd.grad(ops.segment_sum(m, g, weight=w), [m], ga)
    assert torch.equal(gm_only, gm)


def test_weighted_segment_sum_autograd_vs_fp64_dense():
    """ops.segment_sum(weight=) through torch autograd with a non-linear loss, against fp64 autograd of the dense expression."""
    D = 36
    g, deg, msg, w = _operands(D, "contiguous", 6)
    dst = g.dst.long()
    m, ww = msg.detach().requires_grad_(True), w.detach().requires_grad_(True)
    c = torch.randn(N_ROWS, D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
    gm, gwt = torch.autograd.grad((torch.tanh(ops.segment_sum(m, g, weight=ww)) * c).sum(), [m, ww])
    m64, w64 = msg.double().requires_grad_(True), w.double().requires_grad_(True)
    dense = torch.zeros(N_ROWS, D, dtype=torch.float64, device=DEV).index_add(0, dst, w64[:, None] * m64)
    gm64, gw64 = torch.autograd.grad((torch.tanh(dense) * c.double()).sum(), [m64, w64])
    # fp32 chain of ~deg + D roundings against fp64: 1e-5 of the output scale leaves two orders over (129 + 36) 2^-24
    assert rel(gm, gm64) < 1e-5 and rel(gwt, gw64) < 1e-5, (rel(gm, gm64), rel(gwt, gw64))


def test_enveloped_node_attr():
    g, deg, Y, w = _operands(9, "contiguous", 8)
    Y[:, 0] = 1.0
    A = ops.enveloped_node_attr(Y, w, g)
    dst = g.dst.long()
    S = torch.zeros(N_ROWS, 9, dtype=torch.float64, device=DEV).index_add(0, dst, w.double()[:, None] * Y.double())
    want = torch.cat([torch.ones(N_ROWS, 1, dtype=torch.float64, device=DEV), S[:, 1:] / (1 + S[:, :1])], 1)
    assert rel(A, want) < 1e-5
    iso = torch.zeros(9, device=DEV)
    iso[0] = 1.0
    assert torch.all(A[deg == 0] == iso)


# ---------------------------------------------------------------------------------------------------------------------
# 4-6: the models against the fp64 restatement
# ---------------------------------------------------------------------------------------------------------------------
def _params(model):
    return {k[len("net."):]: v.detach().cpu().numpy() for k, v in model.state_dict().items()}


def _reference(model, g, x, pos, lmax, H, layers, **kw):
    """e, forces (caller order), dE/deps of the enveloped restatement on the graph g (built at any radius >= R)."""
    perm = g.perm.cpu().numpy()
    r_c = float(np.float32(kw.pop("r", R)))  # the radius the library sees
    e, f, dE = ER.energy_forces_strain(_params(model), H, layers, lmax, "1x0e+1x1o", x[perm].astype(np.float64),
                                       pos[perm].astype(np.float64), g.rowptr.cpu().numpy(), g.src.cpu().numpy(),
                                       r_c, P_ENV, **kw)
    f_want = np.empty_like(f)
    f_want[perm] = f
    return e, f_want, dE


def _periodic_case(lmax, seed, M=200, H=16, layers=2):
    rng = np.random.default_rng(seed)
    pos = _dyadic(M, seed)
    unwrapped = (pos + rng.integers(-2, 3, size=pos.shape)).astype(np.float32)  # whole periods, exact
    x = rng.standard_normal((M, 4)).astype(np.float32)
    torch.manual_seed(seed + 1)
    model = PeriodicEnergyModel("1x0e+1x1o", H, layers, lmax=lmax, envelope=P_ENV).to(DEV).eval()
    return model, x, unwrapped


_CACHE = {}


def _periodic_run(lmax):
    """One model, its outputs at skin = 0 and skin = SKIN, and the one reference (on the graph at R): shared by the tests."""
    if lmax not in _CACHE:
        model, x, pos = _periodic_case(lmax, 30 + lmax)
        xd, pd = torch.as_tensor(x).to(DEV), torch.as_tensor(pos).to(DEV)
        with _quiet():
            out0 = model(xd, pd, R, *BOX, forces=True, virial=True, stress=True)
            outs = model(xd, pd, R, *BOX, forces=True, virial=True, stress=True, skin=SKIN)
        with torch.no_grad():
            e_only = model(xd, pd, R, *BOX)
        g = radius_graph(pd, R, *BOX, periodic=True)
        ref = _reference(model, g, x, pos, lmax, 16, 2, L=g.box)
        _CACHE[lmax] = (model, x, pos, out0, outs, e_only, ref)
    return _CACHE[lmax]


def _check_outputs(out, ref, vol):
    e, f, W, sigma = out
    e_ref, f_ref, dE = ref
    assert abs(float(e) - e_ref) < 1e-5 * max(1.0, abs(e_ref)), (float(e), e_ref)
    assert rel(f, f_ref) < 2e-5, rel(f, f_ref)
    assert rel(W, -dE[0]) < 2e-5, rel(W, -dE[0])
    assert rel(sigma, dE[0] / vol) < 2e-5, rel(sigma, dE[0] / vol)


@pytest.mark.parametrize("lmax", [1, 2])
def test_periodic_model_vs_reference(lmax):
    model, x, pos, out0, _, e_only, ref = _periodic_run(lmax)
    assert out0[0].dim() == 0 and out0[1].shape == (200, 3) and out0[2].shape == (3, 3) and out0[3].shape == (3, 3)
    _check_outputs(out0, ref, 1.0)
    assert abs(float(e_only) - ref[0]) < 1e-5 * max(1.0, abs(ref[0]))  # the no-grad route
    assert float(out0[1].abs().max()) > 0 and float(out0[3].abs().max()) > 0


@pytest.mark.parametrize("lmax", [1, 2])
def test_skin_invariance_of_the_periodic_model(lmax):
    model, x, pos, out0, outs, _, ref = _periodic_run(lmax)
    pd = torch.as_tensor(pos).to(DEV)
    # the shell (R, R + SKIN] holds edges: the graph with the skin is a different graph
    g0, g1 = radius_graph(pd, R, *BOX, periodic=True), radius_graph(pd, R + SKIN, *BOX, periodic=True)
    assert g1.num_edges - g0.num_edges >= 200, (g0.num_edges, g1.num_edges)
    _, d1, _ = ops.edge_geometry(g1, lmax=1)
    assert int(((d1 > R) & (d1 <= R + SKIN)).sum()) >= 200
    # each within the tolerances of the one reference, and of each other
    _check_outputs(outs, ref, 1.0)
    e0, f0, W0, s0 = out0
    e1, f1, W1, s1 = outs
    assert abs(float(e1) - float(e0)) < 2e-5 * max(1.0, abs(float(e0)))
    assert rel(f1, f0) < 2e-5 and rel(s1, s0) < 2e-5 and rel(W1, W0) < 2e-5, (rel(f1, f0), rel(s1, s0))
    # the reference on the skin graph is the reference (fp64: to rounding)
    ref1 = _reference(model, g1, x, pos, lmax, 16, 2, L=g1.box)
    assert abs(ref1[0] - ref[0]) <= 1e-12 * max(1.0, abs(ref[0]))


def test_skin_changes_a_model_without_the_envelope():
    """The same comparison on the plain model's chain: the shell's edges move the energy by far more than the tolerance --
    the invariance above is the envelope's doing."""
    lmax = 1
    model, x, pos, out0, _, _, _ = _periodic_run(lmax)
    xd, pd = torch.as_tensor(x).to(DEV), torch.as_tensor(pos).to(DEV)
    plain = PeriodicEnergyModel("1x0e+1x1o", 16, 2, lmax=lmax).to(DEV).eval()
    plain.load_state_dict(model.state_dict())  # the envelope adds no parameter or buffer
    with _quiet():
        e_r = plain(xd, pd, R, *BOX, forces=True)[0]
        e_rs = plain(xd, pd, R + SKIN, *BOX, forces=True)[0]
    assert abs(float(e_rs) - float(e_r)) > 1e-3 * max(1.0, abs(float(e_r)))
    assert abs(float(e_r) - float(out0[0])) > 1e-3 * max(1.0, abs(float(e_r)))  # and the envelope is not a no-op


@pytest.mark.parametrize("lmax", [1, 2])
def test_cell_model_vs_reference(lmax):
    T = TR.T
    rng = np.random.default_rng(40 + lmax)
    s = rng.integers(0, 1 << 16, size=(200, 3)) / float(1 << 16)
    pos = ((s + rng.integers(-2, 3, size=s.shape)) @ T).astype(np.float32)  # dyadic cell: exact
    x = rng.standard_normal((200, 4)).astype(np.float32)
    torch.manual_seed(41)
    model = PeriodicEnergyModel("1x0e+1x1o", 16, 2, lmax=lmax, envelope=P_ENV).to(DEV).eval()
    xd, pd = torch.as_tensor(x).to(DEV), torch.as_tensor(pos).to(DEV)
    with _quiet():
        out = model(xd, pd, R, cell=T.tolist(), forces=True, virial=True, stress=True)
    g = radius_graph(pd, R, cell=T.tolist())
    ref = _reference(model, g, x, pos, lmax, 16, 2, cell=T)
    _check_outputs(out, ref, abs(np.linalg.det(T)))


def test_batched_model_with_per_molecule_virials():
    rng = np.random.default_rng(5)
    sizes = rng.integers(3, 30, 64)
    pos = np.concatenate([rng.normal(size=(n, 3)) * 1.5 + rng.uniform(-40, 40, 3) for n in sizes]).astype(np.float32)
    batch = np.concatenate([np.full(n, i) for i, n in enumerate(sizes)])
    order = rng.permutation(len(batch))
    pos, batch = pos[order], batch[order]
    r, H, layers, lmax, n_mol = 5.0, 16, 2, 2, len(sizes)
    torch.manual_seed(6)
    model = BatchedEnergyModel("1x0e+1x1o", H, layers, lmax=lmax, envelope=P_ENV).to(DEV).eval()
    x = torch.randn(len(batch), 4, generator=torch.Generator().manual_seed(7))
    xd, pd, bd = x.to(DEV), torch.from_numpy(pos).to(DEV), torch.from_numpy(batch).to(DEV)
    with _quiet():
        e, f, W = model(xd, pd, bd, r, forces=True, virial=True)
        e_s, f_s, W_s = model(xd, pd, bd, r, forces=True, virial=True, skin=1.0)
    with torch.no_grad():
        e_only = model(xd, pd, bd, r)
    assert W.shape == (n_mol, 3, 3) and e.shape == (n_mol,)
    g, mol = batched_radius_graph(pd, bd, r)
    e_ref, f_ref, dE = _reference(model, g, x.numpy(), pos, lmax, H, layers, r=r, structure=mol.cpu().numpy(), S=n_mol,
                                  per_structure=True)
    assert rel(e, e_ref) < 1e-5 and rel(e_only, e_ref) < 1e-5, (rel(e, e_ref), rel(e_only, e_ref))
    assert rel(f, f_ref) < 2e-5, rel(f, f_ref)
    assert rel(W, -dE) < 2e-5, rel(W, -dE)
    assert rel(e_s, e_ref) < 1e-5 and rel(f_s, f_ref) < 2e-5 and rel(W_s, -dE) < 2e-5


def test_inference_route_on_the_fused_products():
    """H = 32, l_max = 2: under no_grad the messages come from the per-product fused MFMA kernels, then the weighted sum."""
    lmax, H, layers = 2, 32, 1
    model, x, pos = _periodic_case(lmax, 50, H=H, layers=layers)
    assert model.net.layers[0].fused_available()
    xd, pd = torch.as_tensor(x).to(DEV), torch.as_tensor(pos).to(DEV)
    with torch.no_grad():
        e_inf = model(xd, pd, R, *BOX)
    with _quiet():
        e_grad = model(xd, pd, R, *BOX, forces=True)[0]
    g = radius_graph(pd, R, *BOX, periodic=True)
    e_ref = _reference(model, g, x, pos, lmax, H, layers, L=g.box)[0]
    tol = 1e-5 * max(1.0, abs(e_ref))
    assert abs(float(e_inf) - e_ref) < tol and abs(float(e_grad) - e_ref) < tol, (float(e_inf), float(e_grad), e_ref)
    assert abs(float(e_inf) - float(e_grad)) < tol


# ---------------------------------------------------------------------------------------------------------------------
# 7: nothing moved without the envelope; error paths
# ---------------------------------------------------------------------------------------------------------------------
def test_without_the_envelope_nothing_moved():
    pos = torch.as_tensor(_dyadic(500, 60)).to(DEV)
    g = radius_graph(pos, 0.15, *BOX, periodic=True)
    x = torch.randn(500, 4, device=DEV, generator=torch.Generator(device=DEV).manual_seed(61))
    torch.manual_seed(62)
    a = SEGNN("1x0e+1x1o", 16, "1x0e", 2, lmax=2).to(DEV).eval()
    torch.manual_seed(62)
    b = SEGNN("1x0e+1x1o", 16, "1x0e", 2, lmax=2, envelope=None).to(DEV).eval()
    b.load_state_dict(a.state_dict())
    with torch.no_grad():
        assert torch.equal(a(x, g), b(x, g, cutoff=None))
    env = SEGNN("1x0e+1x1o", 16, "1x0e", 2, lmax=2, envelope=P_ENV).to(DEV).eval()
    env.load_state_dict(a.state_dict())
    with torch.no_grad():
        assert not torch.equal(env(x, g, cutoff=0.15), a(x, g))


def test_error_paths():
    pos = torch.as_tensor(_dyadic(50, 70)).to(DEV)
    g = radius_graph(pos, R, *BOX, periodic=True)
    go = radius_graph(pos, R, *BOX)
    x = torch.randn(50, 4, device=DEV)
    for p in (1, 17):
        with pytest.raises(ValueError):
            SEGNN("1x0e+1x1o", 8, "1x0e", 1, lmax=1, envelope=p)
        with pytest.raises(ValueError):
            ops.cutoff_envelope(torch.rand(10, device=DEV), R, p)
    env = SEGNN("1x0e+1x1o", 8, "1x0e", 1, lmax=2, envelope=P_ENV).to(DEV).eval()
    plain = SEGNN("1x0e+1x1o", 8, "1x0e", 1, lmax=2).to(DEV).eval()
    with torch.no_grad():
        with pytest.raises(ValueError):
            env(x, g)
        with pytest.raises(ValueError):
            plain(x, g, cutoff=R)
        with pytest.raises(RuntimeError):
            env.to(torch.bfloat16)(x.bfloat16(), g, cutoff=R)
        env = env.float()
        for kw in ({"halo": object()}, {"split": object()}):
            with pytest.raises(NotImplementedError):
                env(x, go, cutoff=R, **kw)
        Y, d, A = ops.edge_geometry(go, lmax=2)
        w = ops.cutoff_envelope(d, R, P_ENV)
        h = torch.randn(50, 72, device=DEV)  # 8x0e + 8x1o + 8x2e
        with pytest.raises(NotImplementedError):
            env.layers[0](h, go, Y, d, A, halo=object(), w=w)
        with pytest.raises(RuntimeError):
            env.layers[0](h.bfloat16(), go, Y, d, A, w=w)
        with pytest.raises(RuntimeError):
            ops.segment_sum(torch.randn(go.num_edges, 8, device=DEV).bfloat16(), go, weight=w)
        with pytest.raises(ValueError):
            ops.segment_sum(torch.randn(go.num_edges, 8, device=DEV), go, weight=w[:-1])
    model = PeriodicEnergyModel("1x0e+1x1o", 8, 1, lmax=1).to(DEV).eval()
    with pytest.raises(ValueError):
        model(x, pos, R, *BOX, skin=SKIN)
    envm = PeriodicEnergyModel("1x0e+1x1o", 8, 1, lmax=1, envelope=P_ENV).to(DEV).eval()
    with pytest.raises(ValueError):  # the periodic cutoff check applies to r + skin: 2 (0.2 + 0.3) >= 1
        envm(x, pos, R, *BOX, skin=0.3)

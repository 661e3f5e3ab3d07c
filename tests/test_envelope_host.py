"""The cutoff envelope without a GPU: the closed forms of include/e3gnn.h against each other, the skin invariance of the
fp64 restatement (tests/envelope_reference.py) -- the property the envelope exists for -- next to the same comparison without
the envelope (which must fail by orders of magnitude), and the host side of the new entries: C ABI argument checks, the
bindings, and the Python argument checks that run before any device call."""
import ctypes

import numpy as np
import pytest
import torch

import envelope_reference as ER
import pbc_reference as P
import virial_reference as V
from scalable_e3_gnn_amd import _lib

NEW_ENTRIES = ["e3_cutoff_envelope", "e3_cutoff_envelope_backward", "e3_segment_sum_weighted",
               "e3_segment_sum_weighted_backward"]
H, LAYERS = 8, 2
R, SKIN = 0.2, 0.05


@pytest.mark.parametrize("p", [2, 6, 16])
def test_closed_forms_and_derivative_agree(p):
    r_c = 0.7
    d = torch.cat([torch.linspace(0.0, r_c, 2001, dtype=torch.float64),
                   torch.tensor([r_c * (1 - 1e-9), r_c, r_c * (1 + 1e-9), 2 * r_c], dtype=torch.float64)])
    d.requires_grad_(True)
    u = ER.envelope64(d, r_c, p)
    # the expanded form cancels: its error is a few roundings of its largest terms
    bound = 4 * (1 + (p + 1) * (p + 2) / 2 + p * (p + 2) + p * (p + 1) / 2) * 2.0 ** -53
    assert float((u - ER.envelope_expanded64(d, r_c, p)).detach().abs().max()) <= bound
    (du,) = torch.autograd.grad(u.sum(), [d])
    want = ER.envelope_derivative64(d.detach(), r_c, p)
    assert float((du - want).abs().max()) <= 1e-13 * float(want.abs().max())
    # the properties of the header
    assert float(u[0].detach()) == 1.0 and float(du[0]) == 0.0
    assert torch.all(u[d.detach() >= r_c] == 0.0) and torch.all(du[d.detach() >= r_c] == 0.0)
    assert torch.all(u.detach()[:-3] >= 0.0) and torch.all(want <= 0.0)
    # u'' -> 0 at the cutoff: u' = O((1 - x)^2)
    assert abs(float(want[-4])) <= (p * (p + 1) * (p + 2) / 2) * 1.01e-18 / r_c


def _shell_case(lmax, seed=0, M=200):
    """200 points on the 2^-16 grid of the periodic unit box and the graphs at r and r + skin (2 (r + skin) = 0.5 < L)."""
    from scalable_e3_gnn_amd.segnn import SEGNN
    rng = np.random.default_rng(seed)
    pos = (rng.integers(0, 1 << 16, size=(M, 3)) / float(1 << 16)).astype(np.float32)
    x = rng.standard_normal((M, 4))
    torch.manual_seed(seed + 1)
    params = {k: v.detach().double().numpy()
              for k, v in SEGNN("1x0e+1x1o", H, "1x0e", LAYERS, lmax=lmax).state_dict().items()}
    L = P.box_lengths([0, 0, 0], [1, 1, 1], True)
    graphs = [P.graph_pbc(pos, [0, 0, 0], [1, 1, 1], r, True) for r in (R, R + SKIN)]
    # the shell (r, r + skin] must hold edges for the comparison to mean anything (expected: density * shell volume
    # * M = 200 * 4/3 pi (0.25^3 - 0.2^3) * 200 ~ 1280 directed edges)
    perm, pos4, rowptr, src = graphs[1]
    dst = np.repeat(np.arange(M), np.diff(rowptr))
    dist = np.linalg.norm(P.min_image64(pos4[src, :3].astype(np.float64) - pos4[dst, :3].astype(np.float64), L), axis=1)
    shell = int(((dist > R) & (dist <= R + SKIN)).sum())
    assert shell >= 200, shell
    assert len(graphs[1][3]) - len(graphs[0][3]) == shell
    return params, x, L, graphs


def _caller_order(perm, f):
    out = np.empty_like(f)
    out[perm] = f
    return out


@pytest.mark.parametrize("lmax", [1, 2])
def test_reference_skin_invariance_and_its_failure_without_the_envelope(lmax):
    params, x, L, graphs = _shell_case(lmax)
    with_env, without = [], []
    for perm, pos4, rowptr, src in graphs:
        sp = pos4[:, :3].astype(np.float64)
        e, f, dE = ER.energy_forces_strain(params, H, LAYERS, lmax, "1x0e+1x1o", x[perm], sp, rowptr, src, R, 6, L=L)
        with_env.append((e, _caller_order(perm, f), dE[0]))
        e, f, dE = V.energy_forces_strain(params, H, LAYERS, lmax, "1x0e+1x1o", x[perm], sp, rowptr, src, L)
        without.append((e, _caller_order(perm, f), dE[0]))
    (e0, f0, s0), (e1, f1, s1) = with_env
    assert abs(e1 - e0) <= 1e-12 * max(1.0, abs(e0)), (e0, e1)
    assert np.abs(f1 - f0).max() <= 1e-12 * max(1.0, np.abs(f0).max())
    assert np.abs(s1 - s0).max() <= 1e-12 * max(1.0, np.abs(s0).max())
    assert np.abs(f0).max() > 1e-6 and np.abs(s0).max() > 1e-6  # not a trivially constant model
    # the same two graphs without the envelope: the shell's edges change the energy -- the case can fail
    (e0, f0, _), (e1, f1, _) = without
    assert abs(e1 - e0) > 1e-6 * max(1.0, abs(e0)), (e0, e1)
    assert np.abs(f1 - f0).max() > 1e-6 * max(1.0, np.abs(f0).max())


def test_enveloped_forces_are_the_derivative_where_a_pair_crosses_the_cutoff():
    """Two points pushed across the cutoff by +-delta: the central difference of the enveloped energy is the reported force
    (the envelope is C^2: the error is O(delta^2)); the plain energy jumps, so its difference quotient is off by ~ 1 / delta."""
    lmax, delta = 1, 1e-6
    params, x, _, _ = _shell_case(lmax)
    pos = np.array([[0.1, 0.1, 0.1], [0.1 + R, 0.1, 0.1], [0.15, 0.2, 0.1]])
    runs = []
    for shift in (-delta, +delta):
        p2 = pos.copy()
        p2[1, 0] += shift
        rel = p2[None, :, :] - p2[:, None, :]
        adj = (np.linalg.norm(rel, axis=2) <= R) & ~np.eye(3, dtype=bool)
        dst, src = np.nonzero(adj)
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=3))])
        e_env, f_env, _ = ER.energy_forces_strain(params, H, LAYERS, lmax, "1x0e+1x1o", x[:3], p2, rowptr, src, R, 6)
        e_raw, f_raw, _ = V.energy_forces_strain(params, H, LAYERS, lmax, "1x0e+1x1o", x[:3], p2, rowptr, src)
        runs.append((len(src), e_env, f_env[1, 0], e_raw, f_raw[1, 0]))
    (n_in, env_in, fe_in, raw_in, fr_in), (n_out, env_out, fe_out, raw_out, fr_out) = runs
    assert n_in == n_out + 2  # the pair left the graph
    fd_env, f_env = -(env_out - env_in) / (2 * delta), 0.5 * (fe_in + fe_out)
    assert abs(fd_env - f_env) <= 1e-6 * max(1.0, abs(f_env)), (fd_env, f_env)
    fd_raw, f_raw = -(raw_out - raw_in) / (2 * delta), 0.5 * (fr_in + fr_out)
    assert abs(fd_raw - f_raw) > 1e2 * max(1.0, abs(f_raw)), (fd_raw, f_raw)


def test_new_entries_are_declared_and_bound():
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name), name
    assert lib.e3_abi_version() == 3


def test_invalid_arguments_return_before_any_launch():
    """E3_ERR_INVALID_ARG (1) with nothing launched and no pointer dereferenced; empty problems are E3_OK (0)."""
    lib = _lib.load()
    fake = ctypes.c_void_p(16)
    for r_c, p, E in [(1.0, 1, 10), (1.0, 17, 10), (1.0, -3, 10), (0.0, 6, 10), (-1.0, 6, 10), (float("inf"), 6, 10),
                      (float("nan"), 6, 10), (1e-45, 6, 10), (1.0, 6, -1)]:
        assert lib.e3_cutoff_envelope(fake, E, r_c, p, fake, None) == 1, (r_c, p, E)
        assert lib.e3_cutoff_envelope_backward(fake, fake, E, r_c, p, fake, None) == 1, (r_c, p, E)
    assert lib.e3_cutoff_envelope(None, 0, 1.0, 6, None, None) == 0
    assert lib.e3_cutoff_envelope_backward(None, None, 0, 1.0, 2, None, None) == 0
    assert lib.e3_cutoff_envelope(None, 0, 1.0, 1, None, None) == 1  # a bad p is an error even when E = 0
    for N, D, ld_m, ld_a in [(-1, 8, 8, 8), (10, 0, 8, 8), (10, -4, 8, 8), (10, 8, 7, 8), (10, 8, 8, 7)]:
        assert lib.e3_segment_sum_weighted(fake, ld_m, fake, fake, N, D, fake, ld_a, None) == 1
        assert lib.e3_segment_sum_weighted_backward(fake, ld_a, fake, ld_m, fake, fake, N, D, fake, ld_a, fake, None) == 1
    assert lib.e3_segment_sum_weighted_backward(fake, 8, fake, 8, fake, fake, 10, 8, fake, 7, None, None) == 1
    assert lib.e3_segment_sum_weighted(None, 8, None, None, 0, 8, None, 8, None) == 0
    assert lib.e3_segment_sum_weighted_backward(None, 8, None, 8, None, None, 0, 8, None, 8, None, None) == 0
    for null in range(4):  # a NULL pointer with N > 0
        args = [fake, 8, fake, fake, 10, 8, fake, 8, None]
        args[[0, 2, 3, 6][null]] = None
        assert lib.e3_segment_sum_weighted(*args) == 1


def _cpu_graph(N=5):
    from scalable_e3_gnn_amd.radius_graph import RadiusGraph
    return RadiusGraph(perm=torch.arange(N, dtype=torch.int32), pos4=torch.zeros(N, 4),
                       rowptr=torch.zeros(N + 1, dtype=torch.int32), src=torch.zeros(0, dtype=torch.int32), num_edges=0,
                       grid=None)


def test_python_argument_checks_before_the_device():
    from scalable_e3_gnn_amd import ops
    from scalable_e3_gnn_amd.batched import BatchedEnergyModel, PeriodicEnergyModel
    from scalable_e3_gnn_amd.segnn import SEGNN
    for p in (1, 17, 0, -6, 2.5, True):
        with pytest.raises(ValueError):
            SEGNN("1x0e+1x1o", 8, "1x0e", 1, lmax=1, envelope=p)
        with pytest.raises(ValueError):
            ops.cutoff_envelope(torch.zeros(3), 1.0, p)
    for r_c in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            ops.cutoff_envelope(torch.zeros(3), r_c, 6)
    with pytest.raises(RuntimeError):  # CPU tensors: no CPU path
        ops.cutoff_envelope(torch.zeros(3), 1.0, 6)
    g = _cpu_graph()
    x = torch.zeros(5, 4)
    with pytest.raises(ValueError):  # cutoff missing
        SEGNN("1x0e+1x1o", 8, "1x0e", 1, lmax=1, envelope=6)(x, g)
    with pytest.raises(ValueError):  # cutoff superfluous
        SEGNN("1x0e+1x1o", 8, "1x0e", 1, lmax=1)(x, g, cutoff=0.2)
    for halo_kw in ({"halo": object()}, {"split": object()}):
        with pytest.raises(NotImplementedError):
            SEGNN("1x0e+1x1o", 8, "1x0e", 1, lmax=1, envelope=6)(x, g, cutoff=0.2, **halo_kw)
    with pytest.raises(RuntimeError):  # bf16 storage
        SEGNN("1x0e+1x1o", 8, "1x0e", 1, lmax=2, envelope=6)(x.bfloat16(), g, cutoff=0.2)
    # skin without an envelope would change the energy
    with pytest.raises(ValueError):
        PeriodicEnergyModel("1x0e+1x1o", 8, 1, lmax=1)(x, torch.zeros(5, 3), 0.2, [0, 0, 0], [1, 1, 1], skin=0.05)
    with pytest.raises(ValueError):
        BatchedEnergyModel("1x0e+1x1o", 8, 1, lmax=1)(x, torch.zeros(5, 3), torch.zeros(5, dtype=torch.long), 0.2, skin=0.05)
    with pytest.raises(ValueError):
        PeriodicEnergyModel("1x0e+1x1o", 8, 1, lmax=1, envelope=6)(x, torch.zeros(5, 3), 0.2, [0, 0, 0], [1, 1, 1],
                                                                   skin=-0.05)


def test_envelope_adds_no_parameters_or_buffers():
    from scalable_e3_gnn_amd.segnn import SEGNN
    torch.manual_seed(0)
    plain = SEGNN("1x0e+1x1o", 8, "1x0e", 2, lmax=2)
    env = SEGNN("1x0e+1x1o", 8, "1x0e", 2, lmax=2, envelope=6)
    sd = plain.state_dict()
    assert list(sd) == list(env.state_dict())
    env.load_state_dict(sd)  # strict
    assert all(torch.equal(a, b) for a, b in zip(sd.values(), env.state_dict().values()))
    assert env.envelope == 6 and plain.envelope is None

"""Strain, virial and stress without a GPU: self-checks of the fp64 restatement (tests/virial_reference.py) and the
C ABI / binding of the strained geometry entries.  The strain derivative is checked against central finite differences
of the restatement's own energy, the unstrained energy and forces against tests/pbc_reference.py, the symmetry of the
virial (scalar inputs: the energy is invariant under a rotation of every edge vector) and the per-structure split."""
import numpy as np
import pytest
import torch

import pbc_reference as P
import virial_reference as V
from scalable_e3_gnn_amd import _lib

NEW_ENTRIES = ["e3_edge_geometry_strained", "e3_edge_geometry_backward_strained",
               "e3_edge_geometry_backward_strained_workspace_bytes"]
H, LAYERS = 8, 2


def _case(lmax, periodic, seed=0, M=60):
    from scalable_e3_gnn_amd.segnn import SEGNN
    rng = np.random.default_rng(seed)
    pos = rng.random((M, 3)).astype(np.float32)
    r = 0.36
    perm, pos4, rowptr, src = P.graph_pbc(pos, [0, 0, 0], [1, 1, 1], r, periodic)
    L = P.box_lengths([0, 0, 0], [1, 1, 1], periodic)
    x = np.zeros((M, 4))
    x[:, 0] = rng.standard_normal(M)  # scalar inputs only: a rotation of every edge vector leaves the energy unchanged
    torch.manual_seed(seed + 1)
    params = {k: v.detach().double().numpy()
              for k, v in SEGNN("1x0e+1x1o", H, "1x0e", LAYERS, lmax=lmax).state_dict().items()}
    sp = pos4[:, :3].astype(np.float64)
    return params, x[perm], sp, rowptr, src, L


CASES = [(1, True), (2, True), (1, False), (2, False)]


@pytest.mark.parametrize("lmax,periodic", CASES)
def test_strain_derivative_matches_central_differences(lmax, periodic):
    params, x, sp, rowptr, src, L = _case(lmax, periodic)
    assert len(src) > 4 * len(sp)
    e0, _, dE = V.energy_forces_strain(params, H, LAYERS, lmax, "1x0e+1x1o", x, sp, rowptr, src, L)
    delta = 1e-6
    fd = np.zeros((3, 3))
    for a in range(3):
        for b in range(3):
            ep = np.zeros((1, 3, 3))
            ep[0, a, b] = delta
            e_p, _, _ = V.energy_forces_strain(params, H, LAYERS, lmax, "1x0e+1x1o", x, sp, rowptr, src, L, eps=ep)
            e_m, _, _ = V.energy_forces_strain(params, H, LAYERS, lmax, "1x0e+1x1o", x, sp, rowptr, src, L, eps=-ep)
            fd[a, b] = (e_p - e_m) / (2 * delta)
    assert np.abs(dE[0] - fd).max() <= 1e-6 * np.abs(dE[0]).max(), (dE[0], fd)
    assert np.abs(dE[0]).max() > 1e-6 * max(1.0, abs(e0))


@pytest.mark.parametrize("lmax,periodic", CASES)
def test_unstrained_equals_pbc_reference_and_virial_is_symmetric(lmax, periodic):
    params, x, sp, rowptr, src, L = _case(lmax, periodic, seed=1)
    # positions shifted by whole periods on the periodic axes: the minimum image sees the same edge vectors
    shifts = np.random.default_rng(2).integers(-2, 3, size=sp.shape) * (np.asarray(L) > 0)
    up = sp + shifts
    e, f, dE = V.energy_forces_strain(params, H, LAYERS, lmax, "1x0e+1x1o", x, up, rowptr, src, L)
    e_ref, f_ref = P.energy_forces_pbc(params, H, LAYERS, lmax, "1x0e+1x1o", x, up, rowptr, src, L)
    assert abs(e - e_ref) <= 1e-12 * max(1.0, abs(e_ref))
    assert np.abs(f - f_ref).max() <= 1e-12 * max(1.0, np.abs(f_ref).max())
    W = -dE[0]
    assert np.abs(W - W.T).max() <= 1e-10 * np.abs(W).max(), W


@pytest.mark.parametrize("lmax,periodic", [(1, True), (2, False)])
def test_per_structure_virials_sum_to_the_one_structure_virial(lmax, periodic):
    params, x, sp, rowptr, src, L = _case(lmax, periodic, seed=3)
    S = 4
    sid = np.random.default_rng(4).integers(0, S, len(sp))
    e1, f1, dE1 = V.energy_forces_strain(params, H, LAYERS, lmax, "1x0e+1x1o", x, sp, rowptr, src, L)
    eS, fS, dES = V.energy_forces_strain(params, H, LAYERS, lmax, "1x0e+1x1o", x, sp, rowptr, src, L, structure=sid, S=S,
                                         per_structure=True)
    assert dES.shape == (S, 3, 3)
    assert np.abs(dES.sum(0) - dE1[0]).max() <= 1e-12 * np.abs(dE1[0]).max()
    assert abs(eS.sum() - e1) <= 1e-12 * max(1.0, abs(e1))
    assert np.abs(fS - f1).max() <= 1e-12 * np.abs(f1).max()
    # a strain of one structure moves only the edges whose dst row belongs to it
    ep = np.zeros((S, 3, 3))
    ep[2] = 1e-3 * np.random.default_rng(5).standard_normal((3, 3))
    eS2, _, _ = V.energy_forces_strain(params, H, LAYERS, lmax, "1x0e+1x1o", x, sp, rowptr, src, L, structure=sid, S=S,
                                       eps=ep, per_structure=True)
    assert abs(eS2.sum() - e1) > 1e-9 * max(1.0, abs(e1))


def test_new_entries_are_declared_and_bound():
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name), name
    assert lib.e3_abi_version() == 3


def test_invalid_arguments_return_before_any_launch():
    """Host-side argument checks: E3_ERR_INVALID_ARG (1) with nothing launched (every pointer here is a dummy)."""
    import ctypes
    lib = _lib.load()
    fake = ctypes.c_void_p(16)  # never dereferenced: the call must fail in its argument check
    good = _lib.Float3(1.0, 1.0, 1.0)
    bad_box = _lib.Float3(1.0, -1.0, 1.0)
    for lmax, box, strain, S in [(1, None, fake, 0), (2, None, None, 1), (3, None, fake, 1), (1, bad_box, fake, 1),
                                 (2, good, fake, -2)]:
        assert lib.e3_edge_geometry_strained(fake, fake, fake, 10, lmax, box, strain, None, S, fake, fake, fake,
                                             None) == 1
        assert lib.e3_edge_geometry_backward_strained(fake, fake, fake, 10, lmax, box, strain, None, S, fake, fake, fake,
                                                      fake, fake, fake, 1 << 20, None) == 1
    # g_strain NULL, and a workspace that is too small for S = 1
    assert lib.e3_edge_geometry_backward_strained(fake, fake, fake, 10, 1, None, fake, None, 1, fake, fake, fake, fake,
                                                  None, fake, 1 << 20, None) == 1
    need = lib.e3_edge_geometry_backward_strained_workspace_bytes(10)
    assert need >= 36 and lib.e3_edge_geometry_backward_strained_workspace_bytes(1 << 20) <= 4096 * 36
    assert lib.e3_edge_geometry_backward_strained(fake, fake, fake, 10, 1, None, fake, None, 1, fake, fake, fake, fake,
                                                  fake, fake, need - 1, None) == 1
    assert lib.e3_edge_geometry_backward_strained_workspace_bytes(-1) < 0


def test_edge_geometry_rejects_wrong_strain_shapes_before_the_device():
    """ValueError for the shapes, whatever the device (checked before any tensor is touched)."""
    from scalable_e3_gnn_amd import ops
    from scalable_e3_gnn_amd.radius_graph import RadiusGraph
    N = 5
    g = RadiusGraph(perm=torch.arange(N, dtype=torch.int32), pos4=torch.zeros(N, 4),
                    rowptr=torch.zeros(N + 1, dtype=torch.int32), src=torch.zeros(0, dtype=torch.int32), num_edges=0,
                    grid=None)
    for bad in (torch.zeros(3), torch.zeros(2, 3), torch.zeros(4, 3, 2), torch.zeros(0, 3, 3), torch.zeros(1, 1, 3, 3)):
        with pytest.raises(ValueError):
            ops._strain_args(bad, None, g)
    for bad in (torch.zeros(N + 1, dtype=torch.int32), torch.zeros(N, 1, dtype=torch.int32), torch.zeros(N)):
        with pytest.raises(ValueError):
            ops._strain_args(torch.zeros(3, 3), bad, g)
    with pytest.raises(RuntimeError):  # CPU tensors: no CPU path
        ops._strain_args(torch.zeros(2, 3, 3), None, g)

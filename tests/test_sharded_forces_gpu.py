"""``ShardedEnergyModel``: energy, forces, virial, stress and parameter gradients through the differentiable ghost refresh,
with the real kernels.  Small clouds (M = 200-300 dyadic particles in the unit box, r = 1 / (layers + 2.2), 2 layers, fp32):

  * world 1, periodic self-halo (all 26 entries served by local copies) against ``PeriodicEnergyModel`` with the same state
    dict on the same cloud, some positions outside the box.  Both sides are the same fp32 chain in a different summation
    order; tests/test_forces_gpu.py bounds each against fp64 truth at 1e-5 (energy) and 2e-5 (forces), so the two may differ
    by the sum: 2e-5 for the energy, 4e-5 for forces, virial and stress, relative to the largest magnitude.
  * two ranks sharing cuda:0 over gloo, ``GridHalo((2, 1, 1))``: open box against the fp64 autograd oracle of the whole cloud
    (energy 1e-5, forces and all-reduced parameter gradients 2e-5: the bounds of tests/test_forces_gpu.py); periodic box
    against ``PeriodicEnergyModel`` on rank 0 with the bounds of the world-1 case.
  * the API: ``stress=True`` needs a fully periodic ``GridHalo``; a ``PeriodicEnergyModel`` state dict loads; the fused
    inference path (no grad, nothing requested) returns the energy of the gradient path within 1e-5."""
import numpy as np
import pytest
import torch

import gloo_ranks
import models  # noqa: F401  (registers scalable_e3_gnn_amd -- also in the spawned ranks, which import this module)
from scalable_e3_gnn_amd import ShardedEnergyModel
from scalable_e3_gnn_amd.batched import PeriodicEnergyModel
from scalable_e3_gnn_amd.sharding import GridHalo, MortonHalo, MortonPartition, all_reduce_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYERS = 2
R = 1.0 / (LAYERS + 2.2)
IN = "1x0e+1x1o"
LO, HI = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]


def _cloud(M, seed):
    rng = np.random.default_rng(seed)
    pos = (rng.integers(0, 1 << 16, size=(M, 3)) / float(1 << 16)).astype(np.float32)
    return torch.as_tensor(pos), torch.as_tensor(rng.standard_normal((M, 4)).astype(np.float32))


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max())


def _pair(H, lmax, seed):
    """A ``PeriodicEnergyModel`` and a ``ShardedEnergyModel`` that loaded its state dict."""
    torch.manual_seed(seed)
    ref = PeriodicEnergyModel(IN, H, LAYERS, lmax=lmax).to(DEV)
    sh = ShardedEnergyModel(IN, H, LAYERS, lmax).to(DEV)
    sh.load_state_dict(ref.state_dict())
    return ref.eval(), sh.eval()


@pytest.mark.parametrize("H,lmax", [(8, 1), (32, 1), (8, 2), (32, 2)])
def test_world1_self_halo_equals_periodic_model(H, lmax):
    pos, x = _cloud(250, 51)
    pos[:20] += 1.0                                            # outside the box on every axis: wrapped by the halo
    pos[20:30, 1] -= 1.0
    ref, sh = _pair(H, lmax, 52)
    pd, xd = pos.to(DEV), x.to(DEV)
    halo = GridHalo((1, 1, 1), LO, HI, periodic=True)
    got = sh(xd, pd, R, halo, forces=True, virial=True, stress=True)
    want = ref(xd, pd, R, LO, HI, periodic=True, forces=True, virial=True, stress=True)
    red_ptr = halo._maps()[1]
    assert int((red_ptr[1:] - red_ptr[:-1]).max()) >= 3        # precondition: some owned row is sent for >= 3 entries
    assert got[1].shape == pd.shape and got[2].shape == (3, 3) and got[3].shape == (3, 3)
    errs = [_rel(a, b) for a, b in zip(got, want)]
    print(f"\nworld-1 self-halo vs PeriodicEnergyModel, H={H} l_max={lmax}, ghosts/owned {halo.ghost_fraction():.2f}: "
          f"energy {errs[0]:.2e}, forces {errs[1]:.2e}, virial {errs[2]:.2e}, stress {errs[3]:.2e}")
    assert errs[0] < 2e-5 and max(errs[1:]) < 4e-5, errs


def _param_grads(model):
    return {k[len("net."):]: p.grad.detach().double().cpu().numpy() for k, p in model.named_parameters()}


def _worker(rank, world, periodic, H, lmax, q):
    """One rank; a failure is reported on the queue at once (as many items as the rank owes), so the parent never waits
    for its timeout because of a plain exception."""
    import traceback
    try:
        _rank_body(rank, world, periodic, H, lmax, q)
    except Exception:
        for _ in range(2 if rank == 0 else 1):
            q.put(("error", rank, traceback.format_exc()))


def _rank_body(rank, world, periodic, H, lmax, q):
    import torch.distributed as dist
    from oracle import segnn_oracle as S
    from scalable_e3_gnn_amd.radius_graph import radius_graph

    pos, x = _cloud(300, 61)
    ref, model = _pair(H, lmax, 62)
    halo = GridHalo((2, 1, 1), LO, HI, periodic=periodic)
    own = (halo.owner_of(pos) == rank).nonzero().flatten()
    xd, pd = x[own].to(DEV), pos[own].to(DEV)
    with torch.no_grad():                                      # forces switch grad on themselves
        e, f = model(xd, pd, R, halo, forces=True)
    assert f.shape == pd.shape
    model.train()
    model.zero_grad()
    e_train = model(xd, pd, R, halo)                           # E_local + (E_total - E_local).detach()
    e_train.backward()                                         # every rank, once: the refreshes exchange gradients
    all_reduce_grads(model, halo.group)
    assert abs(float(e_train.detach()) - float(e)) <= 1e-5 * abs(float(e))
    q.put(("part", own.numpy(), float(e), f.double().cpu().numpy(), _param_grads(model) if rank == 0 else None))
    if rank == 0 and not periodic:
        g = radius_graph(pos.to(DEV), R, LO, HI)
        perm = g.perm.cpu().numpy()
        params = {k[len("net."):]: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
        E64, F64, gW = S.energy_forces_torch(params, H, LAYERS, lmax, IN, x.double().numpy()[perm],
                                             pos.double().numpy()[perm], g.rowptr.cpu().numpy(), g.src.cpu().numpy(),
                                             np.zeros(len(perm), np.int64), 1)
        F = np.empty_like(F64)
        F[perm] = F64
        q.put(("ref", None, float(E64[0]), F, gW))
    elif rank == 0:
        with torch.no_grad():
            e_ref, f_ref = ref(x.to(DEV), pos.to(DEV), R, LO, HI, periodic=True, forces=True)
        ref.train()
        ref.zero_grad()
        ref(x.to(DEV), pos.to(DEV), R, LO, HI, periodic=True).backward()
        q.put(("ref", None, float(e_ref), f_ref.double().cpu().numpy(), _param_grads(ref)))
    dist.barrier()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("periodic", [False, True])
def test_two_ranks_on_one_gpu(periodic):
    H, lmax = 32, 2
    got = gloo_ranks.run(_worker, 2, (periodic, H, lmax), 3, 240)
    assert not [g for g in got if g[0] == "error"], "\n".join(g[2] for g in got if g[0] == "error")
    _, _, E_ref, F_ref, gW_ref = [g for g in got if g[0] == "ref"][0]
    parts = [g for g in got if g[0] == "part"]
    F = np.full_like(F_ref, np.nan)
    for _, own, e, f, _ in parts:
        F[own] = f
        assert e == parts[0][2]                                # the all-reduced energy is the same number on both ranks
    assert not np.isnan(F).any(), "every particle must be owned by exactly one rank"
    gW = [p[4] for p in parts if p[4] is not None][0]
    e_err = abs(parts[0][2] - E_ref) / abs(E_ref)
    f_err = float(np.abs(F - F_ref).max() / np.abs(F_ref).max())
    w_err = {k: float(np.abs(gW[k] - v).max() / max(np.abs(v).max(), 1e-12)) for k, v in gW_ref.items()}
    assert set(w_err) == set(gW)
    worst = max(w_err, key=w_err.get)
    print(f"\ntwo ranks, GridHalo((2, 1, 1)), periodic={periodic}, vs {'PeriodicEnergyModel' if periodic else 'fp64 oracle'}: "
          f"energy {e_err:.2e}, forces {f_err:.2e}, worst parameter gradient {w_err[worst]:.2e} ({worst})")
    e_tol, g_tol = (2e-5, 4e-5) if periodic else (1e-5, 2e-5)
    assert e_err < e_tol and f_err < g_tol and w_err[worst] < g_tol, (e_err, f_err, worst, w_err[worst])


def test_api_errors_state_dict_and_inference_path():
    pos, x = _cloud(200, 71)
    pd, xd = pos.to(DEV), x.to(DEV)
    ref, sh = _pair(8, 2, 72)                                  # _pair loads a PeriodicEnergyModel state dict
    assert [k for k, _ in sh.state_dict().items()] == [k for k, _ in ref.state_dict().items()]
    for halo in (GridHalo((1, 1, 1), LO, HI), GridHalo((1, 1, 1), LO, HI, periodic=(True, True, False)),
                 MortonHalo(MortonPartition(LO, HI, R, 1).fit(pd))):
        with pytest.raises(ValueError, match="stress"):
            sh(xd, pd, R, halo, stress=True)
    halo = GridHalo((1, 1, 1), LO, HI, periodic=True)
    with torch.no_grad():
        e_fast = sh(xd, pd, R, halo)                           # nothing requested, no grad: the fused inference path
        e_grad, w = sh(xd, pd, R, halo, virial=True)
    assert e_fast.dim() == 0 and w.shape == (3, 3)
    assert abs(float(e_fast) - float(e_grad)) < 1e-5 * abs(float(e_grad)), (float(e_fast), float(e_grad))
    # an open box on one rank (no entry, no ghost: every exchange is empty): the open PeriodicEnergyModel's energy and forces
    e_1, f_1 = sh(xd, pd, R, GridHalo((1, 1, 1), LO, HI), forces=True)
    e_o, f_o = ref(xd, pd, R, LO, HI, periodic=False, forces=True)
    assert _rel(e_1, e_o) < 2e-5 and _rel(f_1, f_o) < 4e-5

#!/usr/bin/env python3
"""Hessian-vector product timings (development / profiles tool) on the configuration of tools/train_step_bench.py case (a):
128 synthetic QM9-shaped molecules (2 059 atoms, r = 5 A), l_max = 2, 4 layers, H = 32, frozen model in eval().

  forces       : one plain ``forward(..., forces=True)`` (forward + first backward of the differentiable chain)
  hvp K = 1    : one ``hessian_vector_product`` with one vector (forward + first backward with create_graph + one second
                 backward)
  hvp K = 8    : the same with eight vectors; (K8 - K1) / 7 is the marginal cost of a further vector

HIP-event times, ms per call after a warm-up, medians of REPEATS alternating measurements of ITERS calls each, as
tools/train_step_bench.py does.  A first measurement: no threshold.

``--strain``: the strained second derivatives on the same atoms and net, wrapped periodic -- the 2 059 atoms uniformly in a
periodic cube of edge 41.6 A (about 15 neighbours per atom within r = 5 A, as in the molecules), a frozen
``PeriodicEnergyModel`` of the same shape:

  forces          : one ``forward(..., forces=True)``
  hvp K = 1       : one ``hessian_vector_product`` (the unstrained kernels)
  strain hvp K = 1: one ``strain_hessian_vector_product`` with one (v, Xi) pair (the strained kernels)
  elastic tensor  : one ``elastic_tensor`` (one forward, one first backward, nine second backwards)

and, beside them, ``hvp K = 1`` of the molecules above: the number to hold against the parent commit's (the unstrained path
launches nothing new).  No thresholds: a first measurement.

usage: hvp_bench.py [--strain] [OUT.json]      (profiles/hvp_step.json, profiles/elastic_step.json)"""
import json, os, statistics, sys, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import models  # noqa
from train_step_bench import dev, iters, molecules, repeats, timed


BOX_EDGE = 41.6


def measure(calls):
    every = {k: [] for k in calls}
    for _ in range(repeats):   # alternating, so that a drift of the clocks reaches all alike
        for k, fn in calls.items():
            every[k].append(timed(fn))
    return every


def strain(argv):
    from scalable_e3_gnn_amd.batched import PeriodicEnergyModel
    mol, _, x, mol_pos, batch, N = molecules()
    mol.requires_grad_(False).eval()
    g = torch.Generator().manual_seed(6)
    pos = (torch.rand(N, 3, generator=g) * BOX_EDGE).to(dev)
    v, xi = torch.randn(1, N, 3, generator=g).to(dev), torch.randn(1, 3, 3, generator=g).to(dev)
    torch.manual_seed(0)
    model = PeriodicEnergyModel("1x0e+1x1o", 32, 4, lmax=2).to(dev).requires_grad_(False).eval()
    box = ([0.0] * 3, [BOX_EDGE] * 3)
    calls = {"forces_ms": lambda: model(x, pos, 5.0, *box, forces=True),
             "hvp_k1_ms": lambda: model.hessian_vector_product(x, pos, 5.0, *box, v=v),
             "strain_hvp_k1_ms": lambda: model.strain_hessian_vector_product(x, pos, 5.0, *box, v=v, strain_v=xi),
             "elastic_tensor_ms": lambda: model.elastic_tensor(x, pos, 5.0, *box),
             "molecules_hvp_k1_ms": lambda: mol.hessian_vector_product(x, mol_pos, batch, 5.0, v)}
    every = measure(calls)
    from scalable_e3_gnn_amd.radius_graph import radius_graph
    out = {"atoms": N, "edges": radius_graph(pos, 5.0, *box, periodic=True).num_edges,
           **{k: statistics.median(t) for k, t in every.items()}}
    out["strain_hvp_k1_over_hvp_k1"] = out["strain_hvp_k1_ms"] / out["hvp_k1_ms"]
    out["elastic_tensor_over_forces"] = out["elastic_tensor_ms"] / out["forces_ms"]
    out.update({k + "_all": t for k, t in every.items()})
    out["steps_per_value"] = iters
    out["note"] = ("same run, frozen models in eval() (l_max = 2, 4 layers, H = 32): 2 059 atoms uniform in a periodic cube of edge "
                   "41.6, r = 5, graph build included in every call, medians of alternating measurements; molecules_hvp_k1 = "
                   "hvp K = 1 of the 128 molecules of the plain run of this tool")
    print(json.dumps(out), flush=True)
    files = [a for a in argv if not a.startswith("--")]
    if files:
        with open(files[0], "w") as fh:
            json.dump({"periodic_2059_lmax2_elastic": out}, fh, indent=1)
            fh.write("\n")


def main(argv):
    warnings.simplefilter("ignore", RuntimeWarning)   # "the unfused differentiable chain runs": what is measured here
    if "--strain" in argv:
        return strain(argv)
    model, _, x, pos, batch, N = molecules()
    model.requires_grad_(False).eval()
    g = torch.Generator().manual_seed(5)
    v8 = torch.randn(8, N, 3, generator=g).to(dev)
    calls = {"forces_ms": lambda: model(x, pos, batch, 5.0, forces=True),
             "hvp_k1_ms": lambda: model.hessian_vector_product(x, pos, batch, 5.0, v8[:1]),
             "hvp_k8_ms": lambda: model.hessian_vector_product(x, pos, batch, 5.0, v8)}
    every = measure(calls)
    out = {"atoms": N, **{k: statistics.median(t) for k, t in every.items()}}
    out["hvp_marginal_ms_per_vector"] = (out["hvp_k8_ms"] - out["hvp_k1_ms"]) / 7
    out["hvp_k1_over_forces"] = out["hvp_k1_ms"] / out["forces_ms"]
    out.update({k + "_all": t for k, t in every.items()})
    out["steps_per_value"] = iters
    out["note"] = ("same run, same frozen model in eval() (128 molecules, l_max = 2, 4 layers, H = 32), graph build included in "
                   "every call, medians of alternating measurements; forces = forward + first backward; hvp = forward + first "
                   "backward with create_graph + one second backward per vector")
    print(json.dumps(out), flush=True)
    files = [a for a in argv if not a.startswith("--")]
    if files:
        with open(files[0], "w") as fh:
            json.dump({"qm9_128mol_lmax2_hvp": out}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])

#!/usr/bin/env python3
"""Hessian-vector product timings (development / profiles tool) on the configuration of tools/train_step_bench.py case (a):
128 synthetic QM9-shaped molecules (2 059 atoms, r = 5 A), l_max = 2, 4 layers, H = 32, frozen model in eval().

  forces       : one plain ``forward(..., forces=True)`` (forward + first backward of the differentiable chain)
  hvp K = 1    : one ``hessian_vector_product`` with one vector (forward + first backward with create_graph + one second
                 backward)
  hvp K = 8    : the same with eight vectors; (K8 - K1) / 7 is the marginal cost of a further vector

HIP-event times, ms per call after a warm-up, medians of REPEATS alternating measurements of ITERS calls each, as
tools/train_step_bench.py does.  A first measurement: no threshold.

usage: hvp_bench.py [OUT.json]      (profiles/hvp_step.json)"""
import json, os, statistics, sys, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import models  # noqa
from train_step_bench import dev, iters, molecules, repeats, timed


def main(argv):
    warnings.simplefilter("ignore", RuntimeWarning)   # "the unfused differentiable chain runs": what is measured here
    model, _, x, pos, batch, N = molecules()
    model.requires_grad_(False).eval()
    g = torch.Generator().manual_seed(5)
    v8 = torch.randn(8, N, 3, generator=g).to(dev)
    calls = {"forces_ms": lambda: model(x, pos, batch, 5.0, forces=True),
             "hvp_k1_ms": lambda: model.hessian_vector_product(x, pos, batch, 5.0, v8[:1]),
             "hvp_k8_ms": lambda: model.hessian_vector_product(x, pos, batch, 5.0, v8)}
    every = {k: [] for k in calls}
    for _ in range(repeats):   # alternating, so that a drift of the clocks reaches all alike
        for k, fn in calls.items():
            every[k].append(timed(fn))
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

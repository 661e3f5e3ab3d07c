"""Clouds and reference graphs shared by tests/test_capped_graph_host.py and tests/test_capped_graph_gpu.py: each uncapped
reference is computed once per process and never modified.  TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np
import torch

import nearest_reference as K
import pbc_reference as P
import triclinic_reference as R
from oracle import graph_oracle as G

N_UNIFORM = 2000
R_UNIFORM = float((3 * 24.0 / (4 * np.pi * N_UNIFORM)) ** (1 / 3))   # ~ 0.142: 7 cells per axis in [0, 1)^3
LO, HI = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
MODES = ("open", "periodic", "mixed", "cell")
PERIODIC = {"periodic": True, "mixed": (True, False, True)}
# the skewed cell of the triclinic tests: heights 0.93, 0.83, 0.75 > 2 r, 6 / 5 / 5 grid cells.  Its volume is 0.66, so the
# cloud wrapped into it is denser: full degrees 7 .. 73, and even k = 64 cuts rows there (45 of them)
CELL = R.T


@functools.lru_cache(maxsize=None)
def uniform_cloud():
    pos = torch.rand(N_UNIFORM, 3, generator=torch.Generator().manual_seed(3), dtype=torch.float32).numpy()
    pos.setflags(write=False)
    return pos


def graph_kwargs(mode):
    """The arguments of radius_graph (after pos, r) of a mode."""
    if mode == "open":
        return dict(lo=LO, hi=HI)
    if mode == "cell":
        return dict(cell=CELL.tolist())
    return dict(lo=LO, hi=HI, periodic=PERIODIC[mode])


@functools.lru_cache(maxsize=None)
def uncapped(mode):
    """-> perm, pos4 [N,4], rowptr, src, box | None, cell | None of the uniform cloud in ``mode`` (read-only arrays)."""
    pos = uniform_cloud()
    box = cell = None
    if mode == "open":
        perm, rowptr, src = G.graph(pos, LO, HI, R_UNIFORM)
        pos4 = np.concatenate([pos[perm], np.zeros((len(pos), 1), np.float32)], 1)
    elif mode == "cell":
        perm, pos4, rowptr, src = R.graph_cell(pos, CELL, R_UNIFORM)
        cell = CELL
    else:
        perm, pos4, rowptr, src = P.graph_pbc(pos, LO, HI, R_UNIFORM, PERIODIC[mode])
        box = P.box_lengths(LO, HI, PERIODIC[mode])
    for a in (perm, pos4, rowptr, src):
        a.setflags(write=False)
    return perm, pos4, rowptr, src, box, cell


@functools.lru_cache(maxsize=None)
def capped(mode, k):
    """-> perm, pos4, rowptr_capped, src_capped, truncated, full_edges, full degrees."""
    perm, pos4, rowptr, src, box, cell = uncapped(mode)
    rowptr_c, src_c, cut, full = K.cap(pos4, rowptr, src, k, box=box, cell=cell)
    rowptr_c.setflags(write=False)
    src_c.setflags(write=False)
    return perm, pos4, rowptr_c, src_c, cut, full, np.diff(rowptr)


def blob_cloud():
    """1536 points 0.5 + 0.01 randn plus 512 uniform points (seed 5), clamped into [0, 1): every blob row has more than 1024
    neighbours inside r = 0.1, so its candidates arrive in at least two chunks."""
    g = torch.Generator().manual_seed(5)
    blob = 0.5 + 0.01 * torch.randn(1536, 3, generator=g)
    back = torch.rand(512, 3, generator=g)
    return torch.cat([blob, back]).clamp(0, 0.999999).float().numpy()

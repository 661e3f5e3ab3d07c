"""The Morton-range halo kernels (csrc/e3_morton_halo.hip) against their torch restatements, bit for bit: ``e3_morton_keys``
== ``morton_keys_torch`` and ``e3_morton_select_count`` / ``_fill`` == ``select_morton_torch`` (``idx`` and ``counts``), over
uniform and clustered clouds, the dyadic cell-face cloud, the block tail and every rank count the 64-bit mask allows."""
import numpy as np
import pytest
import torch

import models  # noqa: F401
from scalable_e3_gnn_amd import _lib
from scalable_e3_gnn_amd.sharding import (MortonPartition, morton_keys, morton_keys_torch, select_morton,
                                          select_morton_torch)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOX = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def _uniform(n, seed=5):
    return torch.rand(n, 3, generator=torch.Generator().manual_seed(seed))


def _clustered(n, seed=6):
    g = torch.Generator().manual_seed(seed)
    pos = torch.rand(n, 3, generator=g)
    blob = torch.rand(n, generator=g) < 0.6
    c = torch.tensor([0.3, 0.65, 0.6])
    return torch.where(blob[:, None], c + 0.15 * torch.randn(n, 3, generator=g), pos).clamp_(0.0, 1.0 - 2.0 ** -20)


def _faces():
    rng = np.random.default_rng(17)
    pos = rng.integers(0, 256, size=(1500, 3)) / 256.0
    v = [0.25 - 0.125, 0.25, 0.25 + 0.125, 0.5, 0.75 - 0.125, 0.75]
    return torch.as_tensor(np.concatenate([pos, [[a, b, c] for a in v for b in v for c in v]])).float()


def _check(pos, r, world, ranks=None, max_bits=6, workspace=None):
    """Fit on the whole cloud, then for each rank compare the HIP selection of its owned particles with the restatement."""
    part = MortonPartition(*BOX, r, world, max_bits=max_bits).fit(pos)
    d = pos.to(DEV)
    keys = morton_keys(d, part.lo, part.hi, part.grid)
    assert keys.is_cuda and torch.equal(keys.cpu(), morton_keys_torch(pos, part.lo, part.hi, part.grid))
    owner = part.owner_of(pos)
    sent = 0
    for me in (range(world) if ranks is None else ranks):
        own = pos[owner == me]
        idx, cnt = select_morton(own.to(DEV), part.lo, part.hi, part.grid, r, part.splitters, me, workspace=workspace)
        widx, wcnt = select_morton_torch(own, part.lo, part.hi, part.grid, r, part.splitters, me)
        assert cnt == wcnt and cnt[me] == 0 and len(cnt) == world
        assert idx.dtype == torch.long and torch.equal(idx.cpu(), widx)
        gidx, gcnt = select_morton_torch(own.to(DEV), part.lo, part.hi, part.grid, r, part.splitters, me)   # on the GPU too
        assert gcnt == wcnt and torch.equal(gidx.cpu(), widx)
        sent += sum(cnt)
    return sent


@pytest.mark.parametrize("cloud", ["uniform", "clustered"])
@pytest.mark.parametrize("world", [1, 2, 8, 13, 64])
def test_select_equals_restatement_large(cloud, world):
    pos = (_uniform if cloud == "uniform" else _clustered)(1 << 17)
    sent = _check(pos, 0.02, world, ranks=sorted({0, world // 2, world - 1}))
    assert (sent > 0) == (world > 1)


def test_every_self_rank_world8():
    assert _check(_clustered(1 << 17), 0.02, 8) > 0


@pytest.mark.parametrize("world", [2, 5, 8])
def test_face_cloud(world):
    assert _check(_faces(), 0.125, world, max_bits=2) > 0       # cells 1/4 wide: particles on faces and at faces +- r
    assert _check(_faces(), 0.125, world) > 0                   # cells 1/8 = r wide


@pytest.mark.parametrize("n", [0, 1, 257])
def test_small_and_block_tail(n):
    pos = _clustered(4096)
    part = MortonPartition(*BOX, 0.1, 8).fit(pos)
    sub = pos[:n]
    for me in range(8):
        idx, cnt = select_morton(sub.to(DEV), part.lo, part.hi, part.grid, 0.1, part.splitters, me)
        widx, wcnt = select_morton_torch(sub, part.lo, part.hi, part.grid, 0.1, part.splitters, me)
        assert cnt == wcnt and torch.equal(idx.cpu(), widx)
    assert torch.equal(morton_keys(sub.to(DEV), part.lo, part.hi, part.grid).cpu(),
                       morton_keys_torch(sub, part.lo, part.hi, part.grid))


def test_workspace_reused_for_two_clouds():
    lib = _lib.load()
    ws = torch.empty(int(lib.e3_morton_select_workspace_bytes(1 << 17, 8)), dtype=torch.uint8, device=DEV)
    assert _check(_clustered(1 << 17), 0.02, 8, ranks=[3], workspace=ws) > 0
    assert _check(_uniform(100_000, seed=9), 0.03, 8, ranks=[3], workspace=ws) > 0
    assert _check(_clustered(1 << 17), 0.02, 8, ranks=[3], workspace=ws) > 0


def test_fit_on_device_equals_fit_on_host():
    pos = _clustered(1 << 17)
    a = MortonPartition(*BOX, 0.02, 8).fit(pos)
    b = MortonPartition(*BOX, 0.02, 8).fit(pos.to(DEV))
    assert a.splitters == b.splitters and a.counts == b.counts and a.hist_max == b.hist_max
    assert all(abs(c - pos.shape[0] / 8) < a.hist_max for c in a.counts)

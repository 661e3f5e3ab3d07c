"""The host side of particle migration, on CPU tensors (no GPU): ``pack_rows`` / ``unpack_rows`` bit for bit,
``migrate_rows_torch`` (the CPU twin of csrc/e3_migrate.hip) against a loop over the rows, and ``Halo.migrate`` at world 1."""
import numpy as np
import pytest
import torch

import models  # noqa: F401  (registers scalable_e3_gnn_amd)
from scalable_e3_gnn_amd import pack_rows, unpack_rows
from scalable_e3_gnn_amd.sharding import GridHalo, migrate_rows_torch

LO, HI = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def test_pack_rows_round_trip_is_bit_exact():
    n = 37
    g = torch.Generator().manual_seed(1)
    pos = torch.randn(n, 3, generator=g)
    x = torch.randn(n, 4, generator=g)
    x[0, 0], x[1, 1], x[2, 2] = float("nan"), float("-inf"), -0.0        # bits, not values
    ids = torch.randint(-2 ** 62, 2 ** 62, (n,), generator=g)
    d = torch.randn(n, 3, generator=g, dtype=torch.float64)
    h = torch.randn(n, 2, generator=g).bfloat16()
    table, layout = pack_rows(pos, x, ids, d, h)
    assert table.dtype == torch.int32 and table.shape == (n, 3 + 4 + 2 + 6 + 1) and table.is_contiguous()
    assert torch.equal(table[:, :3], pos.view(torch.int32))               # positions first
    back = unpack_rows(table, layout)
    for a, b in zip((pos, x, ids, d, h), back):
        assert a.dtype == b.dtype and a.shape == b.shape and b.is_contiguous() and torch.equal(_bits(a), _bits(b))
    assert back[0].data_ptr() != pos.data_ptr()
    # no rows at all, and a lone position tensor
    t0, l0 = pack_rows(pos[:0], ids[:0])
    assert t0.shape == (0, 5) and [t.shape for t in unpack_rows(t0, l0)] == [(0, 3), (0,)]
    t1, l1 = pack_rows(pos)
    assert torch.equal(_bits(unpack_rows(t1, l1)[0]), _bits(pos))
    # one row (a column slice of it is contiguous where it lies), taken from the middle of narrow-dtype storage
    one = (pos[5:6], ids[5:6], h[5:6], d[5:6])
    for a, b in zip(one, unpack_rows(*pack_rows(*one))):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def test_pack_rows_refusals_name_the_tensor():
    pos = torch.zeros(5, 3)
    with pytest.raises(ValueError, match=r"tensor 2 .*bfloat16"):
        pack_rows(pos, torch.zeros(5, 4), torch.zeros(5, 3).bfloat16())
    with pytest.raises(ValueError, match=r"tensor 1 .*requires grad"):
        pack_rows(pos, torch.zeros(5, 4, requires_grad=True))
    with pytest.raises(ValueError, match="tensor 0"):
        pack_rows(pos.requires_grad_(True))
    pos = torch.zeros(5, 3)
    with pytest.raises(ValueError, match="tensor 1"):
        pack_rows(pos, torch.zeros(4, 4))                                 # another row count
    with pytest.raises(ValueError, match="tensor 1"):
        pack_rows(pos, torch.zeros(5, 8)[:, ::2])                         # not contiguous
    with pytest.raises(ValueError, match=r"tensor 1 .*uint8"):
        pack_rows(pos, torch.zeros(5, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        unpack_rows(torch.zeros(5, 4, dtype=torch.int32), pack_rows(pos)[1])


def _by_rows(table, owner, rank, world):
    """The contract, one row at a time."""
    stay = [i for i, o in enumerate(owner) if o == rank]
    send = [i for q in range(world) if q != rank for i, o in enumerate(owner) if o == q]
    counts = [sum(1 for o in owner if o == q) for q in range(world)]
    return table[stay], table[send], counts, sum(1 for o in owner if not 0 <= o < world)


CASES = {
    "empty": (0, 4, 1, lambda n, w, r: []),
    "all stay": (41, 4, 2, lambda n, w, r: [r] * n),
    "all to one rank": (41, 4, 2, lambda n, w, r: [3] * n),
    "round robin": (41, 4, 2, lambda n, w, r: [(r + 1 + i % (w - 1)) % w for i in range(n)]),
    "self first": (41, 4, 0, lambda n, w, r: [(7 * i) % w for i in range(n)]),
    "self last": (41, 4, 3, lambda n, w, r: [(7 * i) % w for i in range(n)]),
    "world 1": (9, 1, 0, lambda n, w, r: [0] * n),
    "invalid": (41, 4, 1, lambda n, w, r: [(-1, w, 0, 1, 2, 3, w + 5, -7)[i % 8] for i in range(n)]),
}


@pytest.mark.parametrize("case", list(CASES))
def test_migrate_rows_torch_order_and_counts(case):
    n, world, rank, make = CASES[case]
    owner = make(n, world, rank)
    table = torch.arange(n * 5, dtype=torch.int32).reshape(n, 5)
    stay, send, counts, n_invalid = migrate_rows_torch(table, torch.tensor(owner, dtype=torch.int32), rank, world)
    w_stay, w_send, w_counts, w_invalid = _by_rows(table, owner, rank, world)
    assert stay.dtype == send.dtype == torch.int32 and counts.dtype == torch.int64
    assert stay.shape == w_stay.shape and torch.equal(stay, w_stay)
    assert send.shape == w_send.shape and torch.equal(send, w_send)
    assert counts.tolist() == w_counts and n_invalid == w_invalid and counts[rank] == stay.shape[0]
    assert stay.shape[0] + send.shape[0] + n_invalid == n
    if case == "round robin":
        assert stay.shape[0] == 0 and min(w_counts[q] for q in range(world) if q != rank) > 0
    if case == "all to one rank":
        assert w_counts == [0, 0, 0, n] and torch.equal(send, table)
    if case == "invalid":
        assert n_invalid == 21 and send.shape[0] > 0 and stay.shape[0] > 0
    # int64 owners (what owner_of returns) give the same answer
    again = migrate_rows_torch(table, torch.tensor(owner, dtype=torch.int64), rank, world)
    assert torch.equal(again[0], stay) and torch.equal(again[1], send) and again[3] == n_invalid


def test_world1_migrate_returns_the_inputs():
    halo = GridHalo((1, 1, 1), LO, HI, periodic=True)
    rng = np.random.default_rng(3)
    pos = torch.as_tensor((rng.random((50, 3)) * 5 - 2).astype(np.float32))      # up to two box lengths outside
    x, ids = torch.randn(50, 4), torch.arange(50)
    halo.setup(pos, x, 0.2)
    gen = halo.generation
    out = halo.migrate(pos, x, ids)
    assert len(out) == 3 and out[0] is pos and out[1] is x and out[2] is ids
    assert halo.generation == gen and halo.migrated == 0 and halo.migrated_out == [0] and halo.migrated_in == [0]
    halo.update_positions(pos, x)                                     # the setup state is still there
    # a position that is not finite has no owner
    bad = pos.clone()
    bad[7, 1] = float("nan")
    with pytest.raises(ValueError, match="no owner"):
        halo.migrate(bad, x, ids)
    assert halo.generation == gen
    with pytest.raises(ValueError, match="tensor 2"):
        halo.migrate(pos, x, torch.zeros(50, 3).half())
    # before any setup the exchange along stored entries names what is missing
    with pytest.raises(RuntimeError, match="setup"):
        GridHalo((1, 1, 1), LO, HI, periodic=True).update_positions(pos, x)

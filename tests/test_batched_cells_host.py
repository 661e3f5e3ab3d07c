"""Batches of periodic cells, the parts that need no GPU: the exported symbols, ``e3_cell_images_plan_batch`` against
``e3_cell_images_plan`` per structure, the argument checks of the batched entries that return before any HIP call, the refusals
of ``BatchedCellImages`` / ``BatchedPeriodicEnergyModel`` that need no device, the shared base class, and the batched twin
(tests/batched_cells_reference.py) on the standard batch: the cases of ``cell_images_reference`` scaled to one cutoff keep
their recorded shells, image counts and edge counts.

Without the feature every test here fails: the names do not exist."""
import ctypes

import numpy as np
import pytest
import torch

import batched_cells_reference as BR
import cell_images_reference as R
import models  # noqa: F401
import scalable_e3_gnn_amd as pkg
from scalable_e3_gnn_amd import _lib
from scalable_e3_gnn_amd import cell_images as CI
from scalable_e3_gnn_amd.batched import BatchedPeriodicEnergyModel, PeriodicEnergyModel

ORIGIN = [0.375, -1.25, 2.5]
EYE = [[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]


def _floats(values):
    flat = [float(v) for v in np.asarray(values, np.float32).reshape(-1)]
    return (ctypes.c_float * max(len(flat), 1))(*flat)


def _plan_batch(cells, origins, r):
    """the C entry on its own -> (status, shells [B][3], rho [B], the table's bytes)"""
    lib = _lib.load()
    B = len(cells)
    rec = lib.e3_cell_images_record_bytes()
    shells, rho = (ctypes.c_int32 * (3 * max(B, 1)))(), (ctypes.c_float * max(B, 1))()
    owner, table = CI._aligned_host(rec * max(B, 1))
    c, o = _floats(cells), _floats(origins)
    st = lib.e3_cell_images_plan_batch(ctypes.addressof(c), ctypes.addressof(o), B, float(r), ctypes.addressof(shells),
                                       ctypes.addressof(rho), table)
    return st, [list(shells[3 * b:3 * b + 3]) for b in range(B)], list(rho)[:B], ctypes.string_at(table, rec * B)


def test_symbols_are_exported_with_the_declared_argument_types():
    lib = _lib.load()
    for name in ("e3_cell_images_record_bytes", "e3_cell_images_plan_batch", "e3_cell_images_count_batch",
                 "e3_cell_images_fill_batch"):
        fn = getattr(lib, name)                                   # AttributeError: the symbol is not exported
        res, args = _lib.SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    rec = lib.e3_cell_images_record_bytes()
    assert rec > 0 and rec % 16 == 0
    for name in ("BatchedCellImages", "batched_cell_image_graph", "BatchedPeriodicEnergyModel"):
        assert name in pkg.__all__ and hasattr(pkg, name)


def test_plan_batch_equals_the_single_plan_bit_for_bit():
    """all seven cases as one batch at each case's own r in turn: shells and rho are those of e3_cell_images_plan on every
    structure, and of the numpy twin wherever the twin accepts the structure (it raises above 7 shells)"""
    lib = _lib.load()
    cells = [R.case(name)[0] for name in R.ALL]
    for origins in ([[0.0] * 3] * len(cells), [BR.origin_of(b) for b in range(len(cells))]):
        for r in sorted({R.case(name)[2] for name in R.ALL}):
            st, shells, rho, _ = _plan_batch(cells, origins, r)
            assert st == _lib.E3_OK
            for b, (cell, origin) in enumerate(zip(cells, origins)):
                m, one = _lib.Int3(), ctypes.c_float()
                assert lib.e3_cell_images_plan(_lib.Float9(*np.asarray(cell, np.float32).reshape(9).tolist()),
                                               _lib.Float3(*origin), r, m, ctypes.byref(one)) == _lib.E3_OK
                assert shells[b] == list(m), (b, r)
                assert np.float32(rho[b]).view(np.uint32) == np.float32(one.value).view(np.uint32), (b, r)
                if max(m) <= R.MAX_SHELLS:
                    tm, trho = R.plan(cell, origin, r)
                    assert shells[b] == tm and np.float32(rho[b]) == trho
    # every case at its own r: the recorded shells
    for b, name in enumerate(R.CASES):
        st, shells, _, _ = _plan_batch([cells[b]], [[0.0] * 3], R.case(name)[2])
        assert st == _lib.E3_OK and tuple(shells[0]) == R.CASES[name]["shells"]


def test_plan_batch_reports_shells_as_they_are_and_refuses_what_the_single_plan_refuses():
    lib = _lib.load()
    st, shells, _, table = _plan_batch([EYE, [[10.0, 0, 0], [0, 10.0, 0], [0, 0, 10.0]]], [[0.0] * 3] * 2, 7.5)
    assert st == _lib.E3_OK and shells == [[8, 8, 8], [1, 1, 1]] and len(table) == 2 * lib.e3_cell_images_record_bytes()
    assert _plan_batch([], [], 1.0)[0] == _lib.E3_OK                                   # B = 0 is valid
    assert _plan_batch([EYE, np.zeros((3, 3))], [[0.0] * 3] * 2, 1.0)[0] == 1         # a singular cell
    assert _plan_batch([EYE], [[float("inf"), 0.0, 0.0]], 1.0)[0] == 1                # a non-finite origin
    assert _plan_batch([EYE], [[0.0] * 3], 0.0)[0] == 1 and _plan_batch([EYE], [[0.0] * 3], float("nan"))[0] == 1
    c, o = _floats(EYE), _floats([0.0] * 3)
    m, rho = (ctypes.c_int32 * 3)(), (ctypes.c_float * 1)()
    owner, table = CI._aligned_host(lib.e3_cell_images_record_bytes())
    args = [ctypes.addressof(c), ctypes.addressof(o), 1, 1.0, ctypes.addressof(m), ctypes.addressof(rho), table]
    assert lib.e3_cell_images_plan_batch(*args) == _lib.E3_OK
    for k in (0, 1, 4, 5, 6):                                                          # every pointer is needed
        assert lib.e3_cell_images_plan_batch(*[None if i == k else a for i, a in enumerate(args)]) == 1
    assert lib.e3_cell_images_plan_batch(*args[:2], -1, *args[3:]) == 1
    assert lib.e3_cell_images_plan_batch(*args[:6], table + 4) == 1                    # the table is read in 16-byte groups


def test_count_and_fill_batch_argument_checks_return_before_any_launch():
    """the checks of the single entries, per structure: shells, the int32 bound with each structure's own shells, counts that
    sum to N.  Every call here passes NULL device pointers with N = 0 or is refused: nothing is launched"""
    lib = _lib.load()
    ok = _plan_batch([EYE, EYE], [[0.0] * 3] * 2, 6.9)                                # 7 shells: the limit
    bad = _plan_batch([EYE, EYE], [[0.0] * 3] * 2, 7.5)                               # 8 shells
    assert ok[1] == [[7, 7, 7]] * 2 and bad[1] == [[8, 8, 8]] * 2

    def tables(planned):
        owner, host = CI._aligned_host(len(planned[3]))
        ctypes.memmove(host, planned[3], len(planned[3]))
        return owner, host
    keep_ok, host_ok = tables(ok)
    keep_bad, host_bad = tables(bad)
    zero = (ctypes.c_int64 * 2)(0, 0)
    count = lambda host, counts, N, B=2: lib.e3_cell_images_count_batch(None, None, N, None, host, ctypes.addressof(counts), B,
                                                                        None, None, None, 0, None)
    fill = lambda host, counts, N, G=0, B=2: lib.e3_cell_images_fill_batch(None, None, N, None, host, ctypes.addressof(counts),
                                                                           B, None, G, None, None, None, None)
    assert fill(host_ok, zero, 0) == _lib.E3_OK                                       # N = 0: valid, nothing to do
    assert fill(host_bad, zero, 0) == 1 and count(host_bad, zero, 0) == 1            # 8 shells in a structure
    assert count(host_ok, zero, 0) == 1                                               # NULL offsets / workspace
    assert fill(host_ok, (ctypes.c_int64 * 2)(1, 0), 0) == 1                          # counts do not sum to N
    assert fill(host_ok, (ctypes.c_int64 * 2)(-1, 1), 0) == 1                         # a negative count
    assert fill(host_ok, zero, 0, G=-1) == 1 and fill(host_ok, zero, 0, B=-1) == 1
    # 15^3 = 3375 rows per particle at 7 shells: 636291 particles stay below 2^31 - 1 rows, 636292 do not
    big = (ctypes.c_int64 * 2)(636291, 0)
    assert 636291 * 3375 < 2 ** 31 - 1 <= 636292 * 3375
    assert fill(host_ok, big, 636291) == _lib.E3_OK                                   # G = 0: returns before a launch
    assert fill(host_ok, (ctypes.c_int64 * 2)(636291, 1), 636292) == 1
    assert fill(host_ok, (ctypes.c_int64 * 2)(318146, 318146), 636292) == 1           # the sum over structures counts
    assert fill(None, zero, 0) == 1                                                   # B > 0 needs the host table


def test_the_shared_base_class_keeps_the_public_attributes():
    one, many = CI.CellImages(EYE, ORIGIN), CI.BatchedCellImages([EYE, [[2.0, 0, 0], [0.5, 2.0, 0], [0, 0, 3.0]]])
    assert isinstance(one, CI.ImageRows) and isinstance(many, CI.ImageRows)
    for name in ("renumber", "split_graph", "exchange", "start", "finish", "refresh", "ghost_rows", "extend", "reduce", "setup"):
        assert callable(getattr(one, name)) and callable(getattr(many, name)), name
        if name != "setup":                                       # one copy: the methods are the base class'
            assert getattr(type(one), name) is getattr(type(many), name) is getattr(CI.ImageRows, name), name
    for obj in (one, many):
        assert obj.anchor is None and obj.overflow is None and obj.map is None and obj.n_owned == 0 and obj.n_ghost == 0
    assert one.cell == tuple(float(v) for row in EYE for v in row) and one.origin == tuple(ORIGIN) and one.volume == 1.0
    assert one.heights == (1.0, 1.0, 1.0) and one.needs_images(0.5)
    assert many.n_structures == 2 and many.volumes == [1.0, 12.0] and len(many.cells) == 2 and many.origins == [(0.0,) * 3] * 2
    # the batched map carries no cell, so a translated expand is refused with the existing message
    source = torch.tensor([0, 1, 0, 1], dtype=torch.int32)
    many.n_owned = 2
    many._selected(2, torch.tensor([0, 1], dtype=torch.int32), torch.tensor([[1, 0, 0], [0, -1, 0]], dtype=torch.int32))
    assert torch.equal(many.map.source, source) and many.map.cell is None and many.map.shift is not None
    with pytest.raises(ValueError, match="translate=True needs a map built with shift= and cell="):
        many.extend(torch.zeros(2, 3, dtype=torch.float64), translate=True)
    assert torch.equal(many.extend(torch.tensor([[1.0], [2.0]])), torch.tensor([[1.0], [2.0], [1.0], [2.0]]))
    assert torch.equal(many.reduce(torch.tensor([[1.0], [2.0], [4.0], [8.0]])), torch.tensor([[5.0], [10.0]]))
    one._selected(2, torch.tensor([0, 1], dtype=torch.int32), torch.tensor([[1, 0, 0], [0, -1, 0]], dtype=torch.int32))
    assert one.map.cell == one.cell                               # CellImages keeps its translation


def test_refusals_need_no_device():
    cells = [EYE, [[2.0, 0, 0], [0.5, 2.0, 0], [0, 0, 3.0]]]
    pos, x = torch.rand(3, 3), torch.randn(3, 4)
    with pytest.raises(ValueError, match=r"structure 0: r = 7.5 needs \(8, 8, 8\) image shells, more than 7 image shells"):
        CI.BatchedCellImages(cells).setup(pos, x, torch.tensor([0, 1, 1]), 7.5)
    with pytest.raises(ValueError, match=r"structure 1: .* needs \(8, 8, 8\) image shells"):
        CI.BatchedCellImages([cells[1], EYE]).setup(pos, x, torch.tensor([0, 1, 1]), 7.5)
    for bad in ([0, 1, 2], [0, -1, 1]):
        with pytest.raises(ValueError, match=r"1 structure ids outside \[0, 2\)"):
            CI.BatchedCellImages(cells).setup(pos, x, torch.tensor(bad), 0.75)
    with pytest.raises(ValueError, match="integer dtype"):
        CI.BatchedCellImages(cells).setup(pos, x, torch.tensor([0.0, 1.0, 1.0]), 0.75)
    with pytest.raises(ValueError, match="non-finite"):
        CI.BatchedCellImages(cells).setup(torch.tensor([[0.0, float("nan"), 0.0]] * 3), x, torch.tensor([0, 1, 1]), 0.75)
    for r in (0.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="finite r > 0"):
            CI.BatchedCellImages(cells).setup(pos, x, torch.tensor([0, 1, 1]), r)
    with pytest.raises(ValueError, match="singular or not finite"):
        CI.BatchedCellImages([EYE, np.zeros((3, 3)).tolist()])
    with pytest.raises(ValueError, match="singular or not finite"):
        CI.BatchedCellImages(cells, [[0.0] * 3, [float("inf"), 0.0, 0.0]])
    with pytest.raises(ValueError, match="one origin per cell"):
        CI.BatchedCellImages(cells, [[0.0] * 3])
    with pytest.raises(RuntimeError, match="ROCm tensors only"):
        CI.BatchedCellImages(cells).setup(pos, x, torch.tensor([0, 1, 1]), 0.75)
    assert CI.BatchedCellImages(torch.tensor(cells)).volumes == [1.0, 12.0]          # a CPU tensor of cells

    torch.manual_seed(0)
    model = BatchedPeriodicEnergyModel("1x0e+1x1o", 8, 1, lmax=1)
    batch = torch.tensor([0, 1, 1])
    with pytest.raises(NotImplementedError, match="create_graph=True with virial= / stress="):
        model(x, pos, batch, 0.75, cells, forces=True, stress=True, create_graph=True)
    with pytest.raises(NotImplementedError, match="create_graph=True with virial= / stress="):
        model(x, pos, batch, 0.75, cells, forces=True, virial=True, create_graph=True)
    with pytest.raises(NotImplementedError, match="create_graph=True with bf16 storage"):
        model(x.bfloat16(), pos, batch, 0.75, cells, forces=True, create_graph=True)
    with pytest.raises(ValueError, match="needs forces=True"):
        model(x, pos, batch, 0.75, cells, create_graph=True)
    with pytest.raises(ValueError, match="skin= needs a model built with envelope="):
        model(x, pos, batch, 0.75, cells, skin=0.1)
    with pytest.raises(ValueError, match="7 image shells"):
        model(x, pos, batch, 7.5, cells)
    with pytest.raises(ValueError, match=r"outside \[0, 2\)"):
        model(x, pos, torch.tensor([0, 1, 2]), 0.75, cells)
    with pytest.raises(RuntimeError, match="ROCm tensors only"):
        model(x, pos, batch, 0.75, cells, forces=True)
    with pytest.raises(RuntimeError, match="ROCm tensors only"):
        model(torch.zeros(0, 4), torch.zeros(0, 3), torch.zeros(0, dtype=torch.long), 0.75, cells)
    with pytest.raises(ValueError, match=r"v must be \[N,3\] or \[K,N,3\]"):
        model.hessian_vector_product(x, pos, batch, 0.75, cells, v=torch.zeros(2, 3))
    # the same net: a state dict of the single-cell model loads as it is
    single = PeriodicEnergyModel("1x0e+1x1o", 8, 1, lmax=1)
    assert list(single.state_dict()) == list(model.state_dict())
    model.load_state_dict(single.state_dict())


def test_the_twin_on_the_standard_batch_reproduces_the_recorded_counts():
    """the cases scaled to r = 1 in one batch with an empty structure in the middle: shells, image counts and edge counts per
    structure are those ``cell_images_reference.CASES`` records, the merged order is (owner, shift), and no pair comes
    closer to the cutoff than the (scaled) gap of its case"""
    bt = BR.make_batch(R.ALL, empty_at=4)
    assert bt["B"] == 8 and 4 not in bt["names"] and len(bt["pos"]) == 323 + len(R.far_positions())
    for b in bt["names"]:                                         # interleaved: no structure of two atoms or more is contiguous
        idx = np.nonzero(bt["batch"] == b)[0]
        assert len(idx) == 1 or idx[-1] - idx[0] >= len(idx), (b, idx)
    shells, _ = BR.plan_batch(bt["cells"], bt["origins"], BR.BATCH_R)
    pos_w, owner, shift, image_pos, per = BR.select_batch(bt["pos"], bt["batch"], bt["cells"], bt["origins"], BR.BATCH_R)
    have = list(zip(owner.tolist(), *shift.T.tolist()))
    assert have == sorted(have) and len(set(have)) == len(have)
    assert len(per[4][0]) == 0 and len(per[4][2]) == 0
    assert sum(len(p[2]) for p in per.values()) == len(owner)
    for b, name in bt["names"].items():
        idx, w, o, s, p = per[b]
        o64 = np.asarray(bt["origins"][b], np.float32).astype(np.float64)
        cell32 = np.asarray(bt["cells"][b], np.float32).astype(np.float64)
        edges, gap = R.brute_edges64(w.astype(np.float64) - o64, cell32, BR.BATCH_R, shells[b])
        if name in R.CASES:
            c = R.CASES[name]
            assert tuple(shells[b]) == c["shells"] and len(o) == c["images"] and len(edges) == c["edges"], name
            assert gap >= 0.9 * c["gap"] / R.case(name)[2], (name, gap)
        else:
            assert len(edges) == 12 and gap > 1e-4, (gap, len(edges))
        mine = np.isin(owner, idx)
        assert np.array_equal(owner[mine], idx[o]) and np.array_equal(shift[mine], s)
        assert np.array_equal(image_pos[mine].view(np.uint32), p.view(np.uint32))

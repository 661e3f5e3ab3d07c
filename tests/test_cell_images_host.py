"""Image rows of small periodic cells, the parts that need no GPU: the selection twin (tests/cell_images_reference.py)
against a brute-force fp64 lattice sum on every case, the adjoint pair ``ops.image_rows_expand`` / ``ops.image_rows_reduce``
on CPU fp64, the refusals of ``images=`` and the exported symbols.

Cases (cell_images_reference.CASES and ``far``): fractional coordinates on the 2^-12 grid; the expected shells, image counts,
edge counts and the distance of the closest pair to the cutoff are those the cases were chosen by, and the twin must
reproduce them exactly."""
import ctypes

import numpy as np
import pytest
import torch

import cell_images_reference as R
import triclinic_reference as TR
import models  # noqa: F401
from scalable_e3_gnn_amd import _lib, ops
from scalable_e3_gnn_amd.batched import PeriodicEnergyModel
from scalable_e3_gnn_amd.cell_images import MAX_SHELLS, CellImages, ImageRowMap, image_shells

ORIGIN = [0.375, -1.25, 2.5]


def _placed(name, origin, unwrap):
    """positions of a case, moved to ``origin`` and (``unwrap``) by whole lattice vectors"""
    cell, pos, r = R.case(name)
    pos = pos + np.asarray(origin, np.float64)
    if unwrap:
        n = np.random.default_rng(11).integers(-3, 4, (len(pos), 3)).astype(np.float64)
        pos = pos + n @ cell
    return cell, pos, r


@pytest.mark.parametrize("origin,unwrap", [([0.0, 0.0, 0.0], False), (ORIGIN, True)])
@pytest.mark.parametrize("name", R.ALL)
def test_twin_keeps_every_needed_image(name, origin, unwrap):
    cell, pos, r = _placed(name, origin, unwrap)
    m, rho = R.plan(cell, origin, r)
    w, owner, shift, image_pos = R.select(pos, cell, origin, r)
    o64 = np.asarray(origin, np.float32).astype(np.float64)
    edges, gap = R.brute_edges64(w.astype(np.float64) - o64, cell, r, m)
    needed = {(j, a, b, c) for (j, a, b, c, i) in edges if (a, b, c) != (0, 0, 0)}
    have = list(zip(owner.tolist(), *shift.T.tolist()))
    assert needed <= set(have), sorted(needed - set(have))[:5]
    assert have == sorted(have) and len(set(have)) == len(have)            # (owner, shift lexicographic), no duplicates
    assert (0, 0, 0) not in {h[1:] for h in have} and np.abs(shift).max(0).tolist() <= list(m)
    want = w[owner].astype(np.float64) + shift.astype(np.float64) @ np.asarray(cell, np.float32).astype(np.float64)
    assert np.abs(image_pos - want).max() <= 4 * 2.0 ** -24 * (np.abs(want).max() + np.abs(cell).sum())
    if name in R.CASES:
        c = R.CASES[name]
        assert tuple(m) == c["shells"] and len(owner) == c["images"] and len(edges) == c["edges"]
        assert gap >= 0.9 * c["gap"]
    else:
        assert gap > 1e-4 * r and len(edges) == 12, (gap, len(edges))       # far: 6 straddling + 6 through-the-face edges
        assert float(rho) - r > 1e-3 and min(TR.derive(np.asarray(cell, np.float32))[1]) > 90 * r   # margin from the cell size


def test_plan_matches_the_library_and_refuses_eight_shells():
    for name in R.ALL:
        cell, _, r = R.case(name)
        for origin in ([0.0, 0.0, 0.0], ORIGIN):
            m, rho = R.plan(cell, origin, r)
            c9 = tuple(np.asarray(cell, np.float32).reshape(9).tolist())
            got_m, got_rho = image_shells(c9, tuple(np.asarray(origin, np.float32).tolist()), r)
            assert list(got_m) == m and got_rho == float(rho)
    eye = [[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]
    assert CellImages(eye).needs_images(0.5) and not CellImages(eye).needs_images(0.49)
    assert image_shells(CellImages(eye).cell, (0.0, 0.0, 0.0), 6.9)[0] == (7, 7, 7)
    with pytest.raises(ValueError, match=f"{MAX_SHELLS} image shells"):
        image_shells(CellImages(eye).cell, (0.0, 0.0, 0.0), 7.5)
    with pytest.raises(ValueError, match="r > 0"):
        image_shells(CellImages(eye).cell, (0.0, 0.0, 0.0), 0.0)
    with pytest.raises(ValueError, match="finite cell and origin"):
        image_shells(CellImages(eye).cell, (float("inf"), 0.0, 0.0), 1.0)


def test_empty_cloud_selects_nothing():
    w, owner, shift, image_pos = R.select(np.zeros((0, 3)), np.eye(3), [0, 0, 0], 1.5)
    assert w.shape == (0, 3) and owner.shape == (0,) and shift.shape == (0, 3) and image_pos.shape == (0, 3)
    rmap = ImageRowMap.build(torch.zeros(0, dtype=torch.int32))
    assert rmap.ptr.tolist() == [0] and rmap.rows.numel() == 0


def _random_map(M, n_owned, seed, with_shift=False):
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(M, generator=g)
    owned, images = perm[:n_owned], perm[n_owned:]
    source = torch.arange(M)
    source[images] = owned[torch.randint(0, n_owned, (M - n_owned,), generator=g)]
    shift = None
    if with_shift:
        shift = torch.zeros((M, 3), dtype=torch.int32)
        shift[images] = torch.randint(-2, 3, (M - n_owned, 3), generator=g).to(torch.int32)
    cell = [1.0, 0.0, 0.0, 0.25, 0.875, 0.0, 0.125, -0.25, 0.75]
    return ImageRowMap.build(source, shift, cell if with_shift else None)


def test_row_map_is_the_csr_of_the_image_rows():
    rmap = _random_map(37, 9, 1)
    ptr, rows = R.row_map_numpy(rmap.source.numpy())
    assert np.array_equal(rmap.ptr.numpy(), ptr) and np.array_equal(rmap.rows.numpy(), rows)
    src = rmap.source.long()
    for i in range(37):
        mine = rmap.rows[rmap.ptr[i]:rmap.ptr[i + 1]].tolist()
        assert mine == [j for j in range(37) if j != i and src[j] == i]     # ascending; empty on image rows
        assert src[src[i]] == src[i]                                          # an image row is never a source


def test_expand_and_reduce_are_adjoint_fp64():
    rmap = _random_map(41, 12, 2, with_shift=True)
    g = torch.Generator().manual_seed(3)
    for D in (1, 3, 7):
        a = torch.randn(41, D, dtype=torch.float64, generator=g)
        b = torch.randn(41, D, dtype=torch.float64, generator=g)
        lhs = (ops.image_rows_reduce(a, rmap) * b).sum()
        rhs = (a * ops.image_rows_expand(b, rmap)).sum()
        assert abs(float(lhs - rhs)) <= 1e-12 * max(1.0, abs(float(rhs)))
    red = ops.image_rows_reduce(a, rmap)
    image = rmap.source.long() != torch.arange(41)
    assert not red[image].any() and torch.equal(ops.image_rows_expand(b, rmap)[~image], b[~image])
    # the translation is a constant: expand(p, translate) - expand(p) = shift @ cell, and the adjoint identity is unchanged
    p = torch.randn(41, 3, dtype=torch.float64, generator=g)
    t = ops.image_rows_expand(p, rmap, translate=True) - ops.image_rows_expand(p, rmap)
    cell = torch.tensor(rmap.cell, dtype=torch.float64).view(3, 3)
    assert torch.allclose(t, rmap.shift.double() @ cell, atol=1e-14)
    with pytest.raises(ValueError, match="translate"):
        ops.image_rows_expand(torch.zeros(41, 4, dtype=torch.float64), rmap, translate=True)
    with pytest.raises(ValueError, match="translate"):
        ops.image_rows_expand(p, _random_map(41, 12, 2), translate=True)


def test_row_broadcast_inputs_and_sum_gradients():
    """the backward of ``.sum(0)`` hands a Function a gradient with strides (0, 1): values as torch indexing gives them"""
    rmap = _random_map(23, 7, 6)
    src = rmap.source.long()
    c = torch.randn(5, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    x = torch.randn(23, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(8), requires_grad=True)
    (got,) = torch.autograd.grad((ops.image_rows_expand(x, rmap).sum(0) * c).sum(), x)
    (want,) = torch.autograd.grad((x[src].sum(0) * c).sum(), x)
    assert torch.allclose(got, want, rtol=0, atol=1e-13)
    (got,) = torch.autograd.grad((ops.image_rows_reduce(x, rmap).sum(0) * c).sum(), x)
    (want,) = torch.autograd.grad((torch.zeros_like(x).index_add(0, src, x).sum(0) * c).sum(), x)
    assert torch.allclose(got, want, rtol=0, atol=1e-13)
    row = c.expand(23, 5)
    assert row.stride() == (0, 1) and torch.equal(ops.image_rows_expand(row, rmap), row[src])


def test_gradgradcheck_of_both_functions_cpu_fp64():
    rmap = _random_map(11, 4, 4, with_shift=True)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(11, 3, dtype=torch.float64, generator=g, requires_grad=True)
    # composed with a nonlinearity, so the second derivative is not identically zero
    for fn in (lambda t: ops.image_rows_expand(t, rmap).sin(), lambda t: ops.image_rows_expand(t, rmap, translate=True).sin(),
               lambda t: ops.image_rows_reduce(t, rmap).sin(), lambda t: ops.image_rows_reduce(ops.image_rows_expand(t, rmap),
                                                                                            rmap).sin()):
        assert torch.autograd.gradcheck(fn, (x,))
        assert torch.autograd.gradgradcheck(fn, (x,))
    # third order through the pair: d3/dx3 of sum(sin(E x)) exists and is what torch indexing gives
    y = ops.image_rows_expand(x, rmap).sin().sum()
    z = x[rmap.source.long()].sin().sum()
    for _ in range(3):
        (y,), (z,) = torch.autograd.grad(y, x, create_graph=True), torch.autograd.grad(z, x, create_graph=True)
        assert torch.allclose(y, z, atol=1e-13)
        y, z = (y * y).sum(), (z * z).sum()


SMALL_CELL = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]


def _model_and_cloud():
    torch.manual_seed(0)
    model = PeriodicEnergyModel("1x0e+1x1o", 8, 1, lmax=1)
    return model, torch.randn(3, 4), torch.rand(3, 3)


def test_refusals_need_no_device():
    model, x, pos = _model_and_cloud()
    calls = [lambda r=0.4, **kw: model(x, pos, r, **kw),
             lambda r=0.4, **kw: model.hessian_vector_product(x, pos, r, v=pos, **kw),
             lambda r=0.4, **kw: model.hessian(x, pos, r, **kw),
             lambda r=0.4, **kw: model.strain_hessian_vector_product(x, pos, r, v=pos, **kw),
             lambda r=0.4, **kw: model.elastic_tensor(x, pos, r, **kw)]
    for call in calls:
        for images in (True, "auto"):
            with pytest.raises(ValueError, match="images= .* needs cell="):
                call(lo=[0.0] * 3, hi=[1.0] * 3, images=images)
            with pytest.raises(ValueError, match="images= .* needs cell="):
                call(lo=[0.0] * 3, hi=[1.0] * 3, periodic=(True, True, False), images=images)
            with pytest.raises(ValueError, match="images= .* needs cell="):
                call(cell=SMALL_CELL, lo=[0.0] * 3, images=images)
            with pytest.raises(NotImplementedError, match="Verlet list over image rows"):
                call(cell=SMALL_CELL, neighbors=object(), images=images)
        with pytest.raises(ValueError, match="images must be False, True"):
            call(cell=SMALL_CELL, images="yes")
        with pytest.raises(ValueError, match="7 image shells"):
            call(r=7.5, cell=SMALL_CELL, images=True)


def test_images_false_on_a_small_cell_raises_todays_message():
    model, x, pos = _model_and_cloud()
    for kw in ({}, {"images": False}):
        with pytest.raises(ValueError, match="need 0 < 2 r < the smallest perpendicular height"):
            model(x, pos, 0.75, cell=SMALL_CELL, **kw)
        with pytest.raises(ValueError, match="need 0 < 2 r < the smallest perpendicular height"):
            model.hessian_vector_product(x, pos, 0.75, cell=SMALL_CELL, v=pos, **kw)


def test_create_graph_and_bf16_refusals_are_unchanged_on_the_image_path():
    model, x, pos = _model_and_cloud()
    with pytest.raises(NotImplementedError, match="create_graph=True with virial= / stress="):
        model(x, pos, 0.75, cell=SMALL_CELL, forces=True, stress=True, create_graph=True, images=True)
    with pytest.raises(NotImplementedError, match="create_graph=True with bf16 storage"):
        model(x.bfloat16(), pos, 0.75, cell=SMALL_CELL, forces=True, create_graph=True, images=True)
    with pytest.raises(ValueError, match="needs forces=True"):
        model(x, pos, 0.75, cell=SMALL_CELL, create_graph=True, images=True)
    with pytest.raises(ValueError, match="skin= needs a model built with envelope="):
        model(x, pos, 0.75, cell=SMALL_CELL, skin=0.1, images=True)


def test_symbols_are_exported_with_the_declared_argument_types():
    lib = _lib.load()
    assert lib.e3_abi_version() == 3
    names = ["e3_cell_images_plan", "e3_cell_images_workspace_bytes", "e3_cell_images_count", "e3_cell_images_fill",
             "e3_image_rows_expand", "e3_image_rows_reduce"]
    for name in names:
        fn = getattr(lib, name)                                   # AttributeError: the symbol is not exported
        res, args = _lib.SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert lib.e3_cell_images_workspace_bytes(0) > 0 and lib.e3_cell_images_workspace_bytes(-1) == -1
    # argument checks that return before any HIP call
    c9, o3 = _lib.Float9(1, 0, 0, 0, 1, 0, 0, 0, 1), _lib.Float3(0, 0, 0)
    m, rho = _lib.Int3(), ctypes.c_float()
    assert lib.e3_cell_images_plan(c9, o3, 7.5, m, ctypes.byref(rho)) == _lib.E3_OK and list(m) == [8, 8, 8]
    assert lib.e3_cell_images_count(None, 0, c9, o3, 7.5, None, None, None, 0, None) == 1      # 8 shells: invalid argument
    assert lib.e3_cell_images_fill(None, 0, c9, o3, 7.5, None, 0, None, None, None, None) == 1
    assert lib.e3_cell_images_fill(None, 0, c9, o3, 6.9, None, 0, None, None, None, None) == _lib.E3_OK
    assert lib.e3_cell_images_plan(_lib.Float9(*([0.0] * 9)), o3, 1.0, m, ctypes.byref(rho)) == 1
    assert lib.e3_image_rows_expand(None, 3, None, None, None, 0, 3, _lib.E3_F32, None, 3, None) == _lib.E3_OK
    assert lib.e3_image_rows_expand(None, 3, None, None, c9, 0, 3, _lib.E3_F32, None, 3, None) == 1     # cell without shift
    assert lib.e3_image_rows_expand(None, 2, None, None, None, 0, 3, _lib.E3_F32, None, 3, None) == 1   # ld below D
    assert lib.e3_image_rows_reduce(None, 3, None, None, None, 0, 0, 3, _lib.E3_BF16, None, 3, None) == 1
    assert lib.e3_image_rows_reduce(None, 3, None, None, None, 0, 0, 3, _lib.E3_F64, None, 3, None) == _lib.E3_OK

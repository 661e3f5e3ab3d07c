"""Batches of periodic cells on the device: the batched selection (``e3_cell_images_count_batch`` / ``_fill_batch``), the graph
over the extended cloud of a batch and ``BatchedPeriodicEnergyModel`` against fp64 on every structure's explicit supercell.

The standard batch (tests/batched_cells_reference.py): all seven cases of ``cell_images_reference.ALL`` -- ``tri5, sc1, mixed,
flat, fcc2, big300, far``; 1, 2, 3, 5, 12 and 300 atoms and the face-straddling ``far`` set; shells differ per structure -- in ONE
batch with an eighth structure without atoms at id 4, every structure at its own origin and moved by whole lattice vectors, the
atoms interleaved by a fixed permutation.  A batch has one cutoff, so every case is scaled to r = 1; shells, image counts and
edge counts do not depend on the scale and are those the cases record.

Selection: bit for bit against the numpy twin and against ``CellImages.setup`` on every structure alone.  Graph: per structure
the edge set (owner of src, shift of src, dst) equals the fp64 brute-force lattice sum; no edge joins two structures or ends in
an image row.  The batched builder searches on a copy of the cloud moved onto a lattice of boxes (``batched_radius_graph``), so
its edge TEST sees positions rounded at the lattice offset, at most three roundings of half a spacing each per coordinate; the
test checks that this stays below the distance of every pair to the cutoff (``far``: 1.5e-4 r), so the edge set is exact.  The
edge VECTORS are those of the extended cloud itself.

Derivatives: the five ``SMALL`` cases and a structure without atoms as one batch, hidden 32, 2 layers, l_max = 2, envelope 6,
against ``strain_hessian_reference.Reference`` on each structure's smallest supercell with 2 r < every height (a brute-force
minimum-image graph the code under test never builds).  Bounds, those of tests/test_cell_images_gpu.py: 1e-5 |E| on every
energy (the no_grad call too), 2e-5 of the largest magnitude on forces, virial and stress per structure (``sc1``: the force is a
cancellation, held to 1e-6 of max |dE/dpos_ext|), max(2e-5, 20 x the fp32 restatement's error) on H v and on the parameter
gradients of the force-matching loss.

Without the feature every test here fails: the names do not exist.  ``test_selection_*`` pins the new kernels."""
import functools

import numpy as np
import pytest
import torch

import batched_cells_reference as BR
import cell_images_reference as R
import force_loss_reference as FR
import models  # noqa: F401
import strain_hessian_reference as SR
from scalable_e3_gnn_amd import cell_images as CI
from scalable_e3_gnn_amd.batched import BatchedPeriodicEnergyModel, PeriodicEnergyModel, _energy_and_gradients
from test_force_loss_gpu import _quiet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IN = "1x0e+1x1o"
LAYERS, HID, P_ENV, K = 2, 32, 6, 2
RC = BR.BATCH_R


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _standard():
    bt = BR.make_batch(R.ALL, empty_at=4)
    return bt, BR.select_batch(bt["pos"], bt["batch"], bt["cells"], bt["origins"], RC)


def _device(bt, batch_dtype=torch.int64):
    return (torch.as_tensor(bt["pos"]).to(DEV), torch.as_tensor(bt["batch"]).to(batch_dtype).to(DEV), bt["cells"].tolist(),
            bt["origins"].tolist())


def test_selection_equals_the_twin_and_the_single_cell_selection_bit_for_bit():
    bt, (w, owner, shift, image_pos, per) = _standard()
    pos, batch, cells, origins = _device(bt, torch.int32)            # any integer dtype
    N = len(bt["pos"])
    x = torch.arange(N * 4, dtype=torch.float32, device=DEV).view(-1, 4)
    images = CI.BatchedCellImages(cells, origins)
    pos_ext, x_ext, batch_ext = images.setup(pos, x, batch, RC)
    G = len(owner)
    assert images.n_structures == 8 and images.n_owned == N and images.n_ghost == G and pos_ext.shape == (N + G, 3)
    assert images.counts == np.bincount(bt["batch"], minlength=8).tolist() and images.counts[4] == 0
    assert np.array_equal(images.owner.cpu().numpy(), owner) and np.array_equal(images.shift.cpu().numpy(), shift)
    got = pos_ext.cpu().numpy()
    assert np.array_equal(_bits(got[:N]), _bits(w)) and np.array_equal(_bits(got[N:]), _bits(image_pos))
    assert torch.equal(x_ext[:N], x) and torch.equal(x_ext[N:], x[images.owner.long()])
    assert batch_ext.dtype == torch.int64
    assert np.array_equal(batch_ext.cpu().numpy(), np.concatenate([bt["batch"], bt["batch"][owner]]))
    # per structure: what CellImages.setup returns for that structure alone, ids mapped; the recorded shells and image counts
    for b, name in bt["names"].items():
        idx = per[b][0]
        one = CI.CellImages(cells[b], origins[b])
        p1, _ = one.setup(pos[torch.as_tensor(idx).to(DEV)], x[torch.as_tensor(idx).to(DEV)], RC)
        mine = np.isin(owner, idx)
        n = len(idx)
        assert np.array_equal(_bits(p1[:n].cpu().numpy()), _bits(got[idx])), name
        assert np.array_equal(idx[one.owner.cpu().numpy()], owner[mine]), name
        assert np.array_equal(one.shift.cpu().numpy(), shift[mine]), name
        assert np.array_equal(_bits(p1[n:].cpu().numpy()), _bits(got[N:][mine])), name
        assert tuple(images.shells[b]) == tuple(one.shells) and images.rho[b] == one.rho
        if name in R.CASES:
            assert tuple(images.shells[b]) == R.CASES[name]["shells"] and int(mine.sum()) == R.CASES[name]["images"], name
    assert len({tuple(m) for m in images.shells}) > 1               # shells differ per structure
    with pytest.raises(ValueError, match="translate=True needs a map built with shift= and cell="):
        images.extend(pos, translate=True)


def test_graph_edges_equal_the_brute_force_lattice_sum_per_structure():
    bt, (w, owner, shift, image_pos, per) = _standard()
    pos, batch, cells, origins = _device(bt)
    N = len(bt["pos"])
    x = torch.zeros((N, 4), device=DEV)
    images, split, x_g, pos_g, structure_g = CI.batched_cell_image_graph(pos, x, batch, RC, cells, origins)
    g = split.graph
    perm = g.perm.cpu().numpy()
    ext_owner = np.concatenate([np.arange(N), owner])
    ext_shift = np.concatenate([np.zeros((N, 3), np.int32), shift])
    ext_batch = bt["batch"][ext_owner]
    src, dst = perm[g.src.cpu().numpy()], perm[g.dst.cpu().numpy()]
    assert (dst < N).all()                                          # no edge ends in an image row
    assert (ext_batch[src] == ext_batch[dst]).all()                 # no edge joins two structures
    assert np.array_equal(structure_g.cpu().numpy(), ext_batch[perm]) and structure_g.shape == (N + len(owner),)
    assert torch.equal(pos_g[images.owned_new].cpu(), torch.as_tensor(w))
    gaps = []
    for b, name in bt["names"].items():
        idx = per[b][0]
        local = np.full(N, -1)
        local[idx] = np.arange(len(idx))
        m = ext_batch[dst] == b
        got = set(zip(local[ext_owner[src[m]]].tolist(), *ext_shift[src[m]].T.tolist(), local[dst[m]].tolist()))
        o64 = np.asarray(origins[b], np.float32).astype(np.float64)
        cell32 = np.asarray(cells[b], np.float32).astype(np.float64)
        want, gap = R.brute_edges64(per[b][1].astype(np.float64) - o64, cell32, RC, images.shells[b])
        gaps.append(gap)
        assert len(got) == int(m.sum()) and got == want, (name, len(got), len(want), gap)
        assert len(want) == (R.CASES[name]["edges"] if name in R.CASES else 12), name
        print(f"\n{name} (structure {b}): rows {len(idx)} + {int(np.isin(owner, idx).sum())}, edges {len(got)}, gap {gap:.1e}")
    # The builder's lattice copy: coordinates reach top = side (extent + 2 r) + r, and a copy is fl(fl(fl(p - pmin) + offset) +
    # r), three roundings of at most half a spacing at `top` each.  A pair's distance moves by at most sqrt(3) * 2 * 1.5
    # spacings < 5.2 spacings, which must stay below the distance of every pair to the cutoff (far: 1.5e-4 r, big300: 1.1e-4 r)
    pe, be = np.concatenate([w, image_pos]).astype(np.float64), ext_batch
    extent = max(float((pe[be == b].max(0) - pe[be == b].min(0)).max()) for b in bt["names"])
    top = 2 * (extent + 2.0 * RC) + RC                              # 8 structures: a 2 x 2 x 2 lattice
    spacing = float(np.spacing(np.float32(top)))
    print(f"\nlattice copy: top coordinate {top:.1f}, fp32 spacing {spacing:.2e}, smallest gap {min(gaps):.2e}")
    assert spacing < 1.5e-4 * RC and 5.2 * spacing < min(gaps), (top, spacing, min(gaps))
    (si, di), (sb, db) = split.interior, split.boundary
    ghost = images.is_ghost
    assert not ghost[si.long()].any() and ghost[sb.long()].all() and si.numel() + sb.numel() == g.num_edges


# ---- derivatives against fp64 on every structure's supercell ---------------------------------------------------------
def _params(model):
    return {k[len("net."):]: v.detach().cpu().numpy() for k, v in model.state_dict().items()}


def _reference_args(model, bt, per, b, name, x):
    """the arguments of the fp64 restatement for structure b on its supercell -> (args, kw, n, k, V of the supercell)"""
    idx, w = per[b][0], per[b][1]
    tile = R.CASES[name]["tile"]
    k = int(np.prod(tile))
    cell32 = np.asarray(bt["cells"][b], np.float32).astype(np.float64)
    pos_s, cell_s = R.supercell(w.astype(np.float64), cell32, tile)
    rowptr, src = R.min_image_graph64(pos_s, cell_s, RC)
    assert len(src) == k * R.CASES[name]["edges"]
    args = (_params(model), HID, LAYERS, 2, IN, np.tile(x[idx].astype(np.float64), (k, 1)), pos_s, rowptr, src)
    return args, dict(cell=cell_s, envelope=(float(np.float32(RC)), P_ENV)), len(idx), k, abs(float(np.linalg.det(cell_s)))


@functools.lru_cache(maxsize=None)
def _small():
    """The five SMALL cases and a structure without atoms (id 2) as one batch: every call of the batched model, and per
    structure the fp64 reference and its fp32 restatement"""
    bt = BR.make_batch(R.SMALL, empty_at=2, seed=21)
    per = BR.select_batch(bt["pos"], bt["batch"], bt["cells"], bt["origins"], RC)[4]
    pos, batch, cells, origins = _device(bt)
    N, B = len(bt["pos"]), bt["B"]
    rng = np.random.default_rng(700)
    torch.manual_seed(800)
    model = BatchedPeriodicEnergyModel(IN, HID, LAYERS, lmax=2, envelope=P_ENV).to(DEV).eval()
    x = rng.standard_normal((N, 4)).astype(np.float32)
    v = rng.standard_normal((K, N, 3)).astype(np.float32)
    t = rng.standard_normal((B, 3)).astype(np.float32)              # one uniform translation per structure
    xd, vd = torch.as_tensor(x).to(DEV), torch.as_tensor(v).to(DEV)
    got = {}
    with _quiet():
        with torch.no_grad():
            got["fast"] = (model(xd, pos, batch, RC, cells, origins),)
            got["skin"] = (model(xd, pos, batch, RC, cells, origins, skin=0.05),)
        got["first"] = model(xd, pos, batch, RC, cells, origins, forces=True, virial=True, stress=True)
        got["hvp"] = (model.hessian_vector_product(xd, pos, batch, RC, cells, origins, v=vd),)
        got["one"] = (model.hessian_vector_product(xd, pos, batch, RC, cells, origins, v=vd[0]),)
        got["shift"] = (model.hessian_vector_product(xd, pos, batch, RC, cells, origins, v=torch.as_tensor(t).to(DEV)[batch]),)
        # max |dE/dpos| over the extended rows of every structure: the scale of the cancellation in the forces
        im, split, x_g, pos_g, structure_g, cut = model._image_cloud(xd, pos, batch, RC, cells, origins, 0.0)
        _, gext, _ = _energy_and_gradients(model.net, x_g, split.graph, pos_g, None, 1, True, 0, None, cut, halo=im, split=split)
        gmax = [float(gext[structure_g == b].abs().max()) if bool((structure_g == b).any()) else 0.0 for b in range(B)]
        # the five single-cell calls with the same state dict: information only
        single = PeriodicEnergyModel(IN, HID, LAYERS, lmax=2, envelope=P_ENV).to(DEV).eval()
        single.load_state_dict(model.state_dict())
        alone = {}
        for b in bt["names"]:
            idx = torch.as_tensor(per[b][0]).to(DEV)
            alone[b] = tuple(o.detach().double().cpu().numpy() for o in single(
                xd[idx], pos[idx], RC, cell=cells[b], origin=origins[b], forces=True, virial=True, stress=True, images=True))
    assert all(not o.requires_grad for pair in got.values() for o in pair)          # eval(): everything detached
    assert not [n for n, p in model.named_parameters() if p.grad is not None]
    got = {key: tuple(o.detach().double().cpu().numpy() for o in pair) for key, pair in got.items()}
    want, f32, second = {}, {}, {}
    for b, name in bt["names"].items():
        args, kw, n, k, V = _reference_args(model, bt, per, b, name, x)
        idx = per[b][0]
        for out, dtype in ((want, torch.float64), (f32, torch.float32)):
            ref = SR.Reference(*args, dtype=dtype, **kw)
            gpos, geps = ref.first()
            hv = ref.hvp(v=np.tile(v[:, idx].astype(np.float64), (1, k, 1)))[0][:, :n]
            out[b] = dict(E=float(ref.E.detach()) / k, F=-gpos[:n], W=-geps / k, S=geps / V, hvp=hv)
            if name == "sc1" and dtype == torch.float64:
                second[b] = float(np.abs(ref.elastic(V)[0]).max()) * V / k       # max |d2E/deps2| of the small cell
    return bt, per, got, want, f32, gmax, alone, second, dict(model=model, x=x)


def test_energies_forces_virials_stresses_vs_fp64_supercells():
    bt, per, got, want, _, gmax, alone, _, _ = _small()
    e, f, w_, s = got["first"]
    B, N = bt["B"], len(bt["pos"])
    assert e.shape == (B,) and f.shape == (N, 3) and w_.shape == (B, 3, 3) and s.shape == (B, 3, 3)
    assert got["fast"][0].shape == (B,)
    # the structure without atoms: energy 0, zero virial and stress
    assert e[2] == 0 and got["fast"][0][2] == 0 and not w_[2].any() and not s[2].any()
    for b, name in bt["names"].items():
        idx, ref = per[b][0], want[b]
        e_err = abs(e[b] - ref["E"]) / abs(ref["E"])
        fast = abs(got["fast"][0][b] - ref["E"]) / abs(ref["E"])
        skin = abs(got["skin"][0][b] - ref["E"]) / abs(ref["E"])
        fb = f[idx]
        errs = {"forces": np.abs(fb - ref["F"]).max() / (gmax[b] if name == "sc1" else np.abs(ref["F"]).max()),
                "virial": SR.rel_max(w_[b], ref["W"]), "stress": SR.rel_max(s[b], ref["S"])}
        a = alone[b]
        dev = {"energy": abs(e[b] - a[0]) / abs(a[0]), "forces": np.abs(fb - a[1]).max() / max(np.abs(a[1]).max(), gmax[b] * 1e-6),
               "virial": SR.rel_max(w_[b], a[2]), "stress": SR.rel_max(s[b], a[3])}
        print(f"\n{name} (structure {b}, N={len(idx)}): E = {ref['E']:.4f}, energy err {e_err:.2e} (no_grad {fast:.2e}, skin "
              f"{skin:.2e}), " + ", ".join(f"{n} {v:.2e}" for n, v in errs.items())
              + f"; max |F| = {np.abs(ref['F']).max():.2e}, max |dE/dpos_ext| = {gmax[b]:.2e}; vs the single-cell call: "
              + ", ".join(f"{n} {v:.2e}" for n, v in dev.items()))
        assert e_err < 1e-5 and fast < 1e-5 and skin < 1e-5, (name, e_err, fast, skin)
        if name == "sc1":                                           # one atom: every neighbour is its own image, the force is zero
            assert np.abs(ref["F"]).max() < 1e-12 * gmax[b] and np.abs(fb).max() < 1e-6 * gmax[b], (np.abs(fb).max(), gmax[b])
        else:
            assert errs["forces"] < 2e-5, (name, errs)
            assert np.abs(fb.sum(0)).max() < 1e-4 * np.abs(fb).max()
        assert errs["virial"] < 2e-5 and errs["stress"] < 2e-5, (name, errs)


def test_hessian_vector_products_vs_fp64_supercells():
    bt, per, got, want, f32, _, _, second, _ = _small()
    hv = got["hvp"][0]
    assert hv.shape == (K, len(bt["pos"]), 3) and got["one"][0].shape == (len(bt["pos"]), 3)
    worst = 0.0
    for b, name in bt["names"].items():
        idx = per[b][0]
        g_, w_, f_ = hv[:, idx], want[b]["hvp"], f32[b]["hvp"]
        if name == "sc1":
            # one atom: a lattice-periodic v is a translation, H v = 0; the zero is a cancellation among pair terms of the
            # size of the second derivatives, max |d2E/deps2|
            print(f"\n{name} H v: max |got| = {np.abs(g_).max():.2e}, max |want| = {np.abs(w_).max():.2e}, max |d2E/deps2| = "
                  f"{second[b]:.2e}")
            assert np.abs(w_).max() <= 1e-9 * second[b] and np.abs(g_).max() <= 2e-5 * second[b]
            continue
        err, yard = SR.rel_max(g_, w_), SR.rel_max(f_, w_)
        bound = max(2e-5, 20 * yard)
        print(f"\n{name} H v: max |.| = {np.abs(w_).max():.3e}, err {err:.2e}, fp32 yardstick {yard:.2e}, bound {bound:.1e}")
        assert np.abs(w_).max() > 0
        worst = max(worst, err / bound)
    assert worst < 1.0, worst
    # v [N,3] is the first of the K vectors: the same second backward on the same graph, compared to the bound above
    assert SR.rel_max(got["one"][0], hv[0]) < 2e-5
    assert not got["shift"][0].any()                               # a uniform translation per structure: exactly zero


def test_training_on_forces_vs_the_sum_of_the_fp64_references():
    bt = BR.make_batch(("tri5", "fcc2"), seed=31)
    per = BR.select_batch(bt["pos"], bt["batch"], bt["cells"], bt["origins"], RC)[4]
    pos, batch, cells, origins = _device(bt)
    N = len(bt["pos"])
    rng = np.random.default_rng(900)
    torch.manual_seed(901)
    model = BatchedPeriodicEnergyModel(IN, HID, LAYERS, lmax=2, envelope=P_ENV).to(DEV).train()
    x = rng.standard_normal((N, 4)).astype(np.float32)
    with _quiet():
        e, f = model(torch.as_tensor(x).to(DEV), pos, batch, RC, cells, origins, forces=True, create_graph=True)
    assert e.requires_grad and f.requires_grad and e.shape == (2,) and f.shape == (N, 3)
    total, want, g32 = 0.0, None, None
    add = lambda acc, new: new if acc is None else {n: acc[n] + new[n] for n in new}
    for b, name in bt["names"].items():
        args, kw, n, k, _ = _reference_args(model, bt, per, b, name, x)
        idx = torch.as_tensor(per[b][0]).to(DEV)
        E64, F64, leaves64 = FR.energy_forces(*args, dtype=torch.float64, **kw)
        E32, F32, leaves32 = FR.energy_forces(*args, dtype=torch.float32, **kw)
        loss = FR.matching_loss(float(E64.detach().abs().max()) / k * rng.standard_normal(1)[0],
                                float(F64.detach().abs().max()) * rng.standard_normal((n, 3)))
        assert abs(float(e[b].detach()) - float(E64[0].detach()) / k) < 1e-5 * abs(float(E64[0].detach()) / k)
        assert np.abs(f[idx].detach().double().cpu().numpy() - F64[:n].detach().numpy()).max() \
            < 2e-5 * float(F64[:n].detach().abs().max())
        total = total + loss(e[b], f[idx])
        want = add(want, FR.parameter_gradients(loss(E64[0] / k, F64[:n]), leaves64))
        g32 = add(g32, FR.parameter_gradients(loss(E32[0] / k, F32[:n]), leaves32))
    model.zero_grad()
    total.backward()
    got = {n[len("net."):]: p.grad.detach().double().cpu().numpy().copy() for n, p in model.named_parameters()}
    model.zero_grad()
    assert set(got) == set(want)
    err, yard = FR.worst(got, want), FR.worst(g32, want)
    worst = max(err, key=lambda n: err[n] / max(2e-5, 20 * yard[n]))
    print(f"\ntri5 + fcc2, force-matching loss: worst tensor {worst}: err {err[worst]:.2e}, fp32 yardstick {yard[worst]:.2e}; "
          f"largest err {max(err.values()):.2e}, largest yardstick {max(yard.values()):.2e}")
    for n in want:
        assert np.abs(want[n]).max() > 0, n
        assert err[n] < max(2e-5, 20 * yard[n]), (n, err[n], yard[n])


def test_energies_follow_a_permutation_of_the_structures():
    bt, per, got, want, _, _, _, _, made = _small()
    model, x = made["model"], made["x"]
    B, N = bt["B"], len(bt["pos"])
    rng = np.random.default_rng(41)
    ids, mix = rng.permutation(B), rng.permutation(N)
    assert (ids != np.arange(B)).any()
    cells, origins = np.empty_like(bt["cells"]), np.empty_like(bt["origins"])
    cells[ids], origins[ids] = bt["cells"], bt["origins"]
    with torch.no_grad():
        e = model(torch.as_tensor(x[mix]).to(DEV), torch.as_tensor(bt["pos"][mix]).to(DEV),
                  torch.as_tensor(ids[bt["batch"]][mix]).to(DEV), RC, cells.tolist(), origins.tolist()).double().cpu().numpy()
    assert e[ids[2]] == 0                                           # the structure without atoms moved with its id
    for b, name in bt["names"].items():
        ref = want[b]["E"]
        print(f"\n{name}: structure {b} -> {ids[b]}: E = {e[ids[b]]:.6f}, before {got['fast'][0][b]:.6f}, fp64 {ref:.6f}")
        assert abs(e[ids[b]] - ref) < 1e-5 * abs(ref) and abs(e[ids[b]] - got["fast"][0][b]) < 1e-5 * abs(ref)


def test_refusals_on_the_device_and_the_empty_batch():
    big, small = [[10.0, 0, 0], [0, 10.0, 0], [0, 0, 10.0]], [[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]
    cells = [big, small]
    pos = torch.rand(4, 3, device=DEV)
    x = torch.randn(4, 4, device=DEV)
    batch = torch.tensor([0, 1, 1, 0], device=DEV)
    torch.manual_seed(51)
    model = BatchedPeriodicEnergyModel(IN, HID, LAYERS, lmax=2).to(DEV).eval()
    with pytest.raises(ValueError, match=r"structure 1: r = 7.5 needs \(8, 8, 8\) image shells, more than 7 image shells"):
        model(x, pos, batch, 7.5, cells)
    with pytest.raises(ValueError, match=r"1 structure ids outside \[0, 2\)"):
        model(x, pos, torch.tensor([0, 1, 2, 0], device=DEV), 0.75, cells)
    with pytest.raises(NotImplementedError, match="create_graph=True with virial= / stress="):
        model(x, pos, batch, 0.75, cells, forces=True, stress=True, create_graph=True)
    with pytest.raises(RuntimeError, match="ROCm tensors only"):
        model(x, pos.cpu(), batch, 0.75, cells)
    # bf16 storage has no differentiable chain: refused exactly as the single-cell image path refuses it
    half, one = model.bfloat16(), PeriodicEnergyModel(IN, HID, LAYERS, lmax=2).bfloat16().to(DEV).eval()
    raised = []
    for call in (lambda: half(x.bfloat16(), pos, batch, 0.75, cells, forces=True),
                 lambda: one(x.bfloat16(), pos, 0.75, cell=small, forces=True, images=True)):
        with pytest.raises((RuntimeError, NotImplementedError)) as info:
            call()
        raised.append((type(info.value), str(info.value)))
    assert raised[0] == raised[1], raised
    with pytest.raises(NotImplementedError, match="create_graph=True with bf16 storage"):
        half(x.bfloat16(), pos, batch, 0.75, cells, forces=True, create_graph=True)
    # an empty batch: N = 0, B = 2 -> zeros
    model = model.float()
    none = (torch.zeros((0, 4), device=DEV), torch.zeros((0, 3), device=DEV), torch.zeros(0, dtype=torch.long, device=DEV))
    e = model(*none, 0.75, cells)
    assert e.shape == (2,) and not e.any()
    e, f, w, s = model(*none, 0.75, cells, forces=True, virial=True, stress=True)
    assert e.shape == (2,) and f.shape == (0, 3) and w.shape == (2, 3, 3) and s.shape == (2, 3, 3)
    assert not e.any() and not w.any() and not s.any()
    assert model.hessian_vector_product(*none, 0.75, cells, v=torch.zeros((K, 0, 3), device=DEV)).shape == (K, 0, 3)
    with pytest.raises(ValueError, match="7 image shells"):
        model(*none, 7.5, cells)

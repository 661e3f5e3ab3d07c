"""Every producer of the power-of-two operand scale against the numpy restatement (tests/scale_reference.py), bit for bit:
``s``, ``1/s`` and the bits of max |x| over the FINITE elements (the contract above ``e3_pow2_scale`` in include/e3gnn.h).

Producers: ``ops.pow2_scale`` (absmax_kernel: dense float4, strided float4 and scalar paths), ``ops.add_pow2_scale``
(add_absmax_kernel) and the epilogue of ``forward_fused(..., out_scale=t)`` (tp_fwd_mfma_r16_kernel: vector and scalar
emit paths, with and without residual, gated and not).  Cases: a planted maximum in every binade, NaN / +-inf in the same
4-aligned column group (same lane of every float4 path, same wave of the scalar path) or the same column one row away
(same lane of the scalar emit path) as a finite maximum that stands out of a small background, all-non-finite tensors,
and maxima at the first / last element and in the tail."""
import numpy as np
import pytest
import torch

import models  # noqa: F401
from scale_reference import expected_scale
from scalable_e3_gnn_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TARGETS = (10, 9, 6)          # 10: features, 9: the residual chain, 6: the sharded forward's head room
BINADES = list(range(-149, 128))
FLT_MAX = float(np.finfo(np.float32).max)
NONFINITE = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}


def _got(sc):
    sc = sc.cpu()
    return float(sc[0]), float(sc[1]), int(sc[2:3].view(torch.int32).item()) & 0xFFFFFFFF


def _want(ts, target):
    return expected_scale([t.detach().float().cpu().numpy() for t in ts], target)


def _planted(k):
    return FLT_MAX if k == 128 else float(np.float32(2.0 ** k))


def _paths(W):
    """Three views of one [R, 300] buffer whose scales take the three paths of absmax_kernel; column 100 of the aligned
    views starts a 4-aligned group (one lane's float4)."""
    return {"dense": W[:, 8:296].contiguous(),        # ld == cols == 288: one flat float4 range
            "strided float4": W[:, 8:296],            # ld 300, cols 288, 16-byte aligned start: a wave per row
            "scalar": W[:, 3:290]}                    # unaligned start, cols 287: scalar loads, a wave per row


def _background(R, k, zero, seed, C=300):
    """|x| <= 2^(k-2) (two binades below the planted maximum 2^k), or zero; in fp64 first so that tiny binades round once."""
    if zero:
        return torch.zeros(R, C, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(seed)
    return ((torch.rand(R, C, device=DEV, generator=g, dtype=torch.float64) - 0.5) * 2.0 ** (k - 1)).float()


# ---------------------------------------------------------------------------------------------------------------------
# binade sweep
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zero", [False, True], ids=["background", "zeros"])
def test_pow2_scale_binade_sweep(zero):
    got, want, what = [], [], []
    for k in BINADES + [128]:
        for sign in (1.0, -1.0):
            W = _background(67, min(k, 127), zero, seed=k + 200)
            W[41, 108] = sign * _planted(k)                    # view column 100 of the aligned views, 105 of the scalar one
            for name, v in _paths(W).items():
                for t in TARGETS:
                    got.append(ops.pow2_scale([v], target_log2=t))
                    want.append(_want([v], t))
                    what.append((name, k, sign, t))
    got = torch.stack(got).cpu()
    bad = [(w, _got(g), e) for g, e, w in zip(got, want, what) if _got(g) != e]
    assert not bad, f"{len(bad)} of {len(what)} scales differ; first: {bad[:4]}"


@pytest.mark.parametrize("zero", [False, True], ids=["background", "zeros"])
def test_add_pow2_scale_binade_sweep(zero):
    got, want, what = [], [], []
    for k in BINADES + [128]:
        for sign in (1.0, -1.0):
            W = _background(64, min(k, 127), zero, seed=k + 300)
            W[17, 201] = sign * _planted(k)
            h = W[:, :288].contiguous()
            u = torch.zeros_like(h)
            for t in TARGETS:
                out, sc = ops.add_pow2_scale(h, u, target_log2=t)
                assert torch.equal(out, h + u)
                got.append(sc)
                want.append(_want([out], t))
                what.append((k, sign, t))
    got = torch.stack(got).cpu()
    bad = [(w, _got(g), e) for g, e, w in zip(got, want, what) if _got(g) != e]
    assert not bad, f"{len(bad)} of {len(what)} scales differ; first: {bad[:4]}"


EPI = [("32x0e+32x1o+32x2e", "32x0e+32x1o+32x2e", False, 2),             # update product #2 (l_max = 2)
       ("32x0e+32x1o+32x2e", "32x0e+64x0e+32x1o+32x2e", True, 2)]         # gated


def _epi_module(irreps, out, lmax, seed=4):
    from scalable_e3_gnn_amd.tensor_product import SHTensorProduct
    torch.manual_seed(seed)
    return SHTensorProduct(irreps, out, lmax).to(DEV)


def _residual(shape, aligned):
    """[B, W] fp32 residual; `aligned` False: a view 4 bytes into a wider buffer, which sends the epilogue down its scalar
    emit path (the vector path needs 16-byte aligned residual rows)."""
    if aligned:
        return torch.zeros(shape, device=DEV)
    return torch.zeros(shape[0], shape[1] + 4, device=DEV)[:, 1:1 + shape[1]]


@pytest.mark.parametrize("irreps,out,gate,lmax", EPI)
def test_epilogue_scale_binade_sweep(irreps, out, gate, lmax):
    """out = product + residual: a zero product (x = 0) leaves out = residual exactly, so the planted residual maximum sweeps
    every binade; without a residual, x is swept over powers of two and the scale is checked against the output it wrote."""
    B = 203
    mod = _epi_module(irreps, out, lmax)
    g = torch.Generator(device=DEV).manual_seed(5)
    y = torch.randn(B, mod.in2_dim, device=DEV, generator=g)
    x0 = torch.zeros(B, mod.in1_dim, device=DEV)
    xr = torch.randn(B, mod.in1_dim, device=DEV, generator=g)
    got, want, what = [], [], []
    with torch.no_grad():
        plain = mod.forward_fused([(x0, None)], y, gate=gate)
        assert float(plain.abs().max()) == 0.0
        for aligned in (True, False):
            for k in BINADES + [128]:
                for sign in (1.0, -1.0):
                    res = _residual(plain.shape, aligned)
                    res.copy_(_background(B, min(k, 127), False, seed=k, C=plain.shape[1]))
                    res[B - 3, 37] = sign * _planted(k)
                    for t in TARGETS:
                        o, sc = mod.forward_fused([(x0, None)], y, gate=gate, residual=res, out_scale=t)
                        got.append(sc)
                        want.append(_want([o], t))
                        what.append(("residual", aligned, k, sign, t))
        for k in range(-100, 101, 5):
            x = xr * 2.0 ** k
            for t in TARGETS:
                o, sc = mod.forward_fused([(x, None)], y, gate=gate, out_scale=t)
                got.append(sc)
                want.append(_want([o], t))
                what.append(("no residual", k, t))
    got = torch.stack(got).cpu()
    bad = [(w, _got(g_), e) for g_, e, w in zip(got, want, what) if _got(g_) != e]
    assert not bad, f"{len(bad)} of {len(what)} scales differ; first: {bad[:4]}"


# ---------------------------------------------------------------------------------------------------------------------
# a non-finite value next to the finite maximum
# ---------------------------------------------------------------------------------------------------------------------
def _small(R, C, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.rand(R, C, device=DEV, generator=g) * 8.0 - 4.0            # |x| <= 4


# (row, column of the maximum, column of the non-finite value) in view coordinates: the same 4-aligned group of columns
SITES = [(41, 100, 101), (41, 103, 100), (0, 0, 1), (66, 283, 282), (66, 286, 284), (33, 284, 285)]


@pytest.mark.parametrize("bad", list(NONFINITE))
def test_pow2_scale_non_finite_next_to_maximum(bad):
    fails = []
    for path in ("dense", "strided float4", "scalar"):
        for r, cm, cb in SITES:
            W = _small(67, 300, seed=r + cm)
            v = _paths(W)[path]
            if cm >= v.shape[1] or cb >= v.shape[1]:
                continue
            v[r, cm] = -7e3
            v[r, cb] = NONFINITE[bad]
            for t in TARGETS:
                got, want = _got(ops.pow2_scale([v], target_log2=t)), _want([v], t)
                if got != want:
                    fails.append((path, (r, cm, cb), t, got, want))
    assert not fails, f"{len(fails)} wrong scales (path, site, target, got (s, 1/s, bits), want): {fails[:6]}"


def test_pow2_scale_all_non_finite_and_placement():
    for path in ("dense", "strided float4", "scalar"):
        for fill in NONFINITE.values():
            W = torch.full((67, 300), fill, device=DEV)
            v = _paths(W)[path]
            assert _got(ops.pow2_scale([v], target_log2=10)) == (1.0, 1.0, 0), (path, fill)
        # alternating NaN / inf with one finite value: first element, last element, last row
        for r, c in [(0, 0), (66, v.shape[1] - 1), (66, 0), (12, v.shape[1] - 2)]:
            W = torch.full((67, 300), float("inf"), device=DEV)
            W[::2] = float("nan")
            v = _paths(W)[path]
            v[r, c] = 3.5e-3
            for t in TARGETS:
                assert _got(ops.pow2_scale([v], target_log2=t)) == _want([v], t), (path, r, c, t)
    # several segments: the non-finite values in one, the maximum in another
    a = _small(100, 288, 1)
    b = _small(50, 288, 2)
    a[7, 9] = float("inf")
    b[49, 287] = 5e3
    for t in TARGETS:
        assert _got(ops.pow2_scale([a, b], target_log2=t)) == _want([a, b], t)
    # the flat tail: 67 x 12 floats = 201 float4, fewer than one workgroup
    v = _small(67, 12, 3)
    v[66, 11], v[66, 8] = 6e3, float("-inf")
    assert _got(ops.pow2_scale([v], target_log2=10)) == _want([v], 10)


@pytest.mark.parametrize("bad", list(NONFINITE))
def test_add_pow2_scale_non_finite_next_to_maximum(bad):
    fails = []
    for r, cm, cb in SITES:
        h = _small(67, 288, seed=r + cm)
        u = _small(67, 288, seed=r + cm + 1) * 0.25
        h[r, cm], u[r, cm] = -7e3, 0.0
        u[r, cb] = NONFINITE[bad]                               # the non-finite value arrives through the update
        for t in TARGETS:
            out, sc = ops.add_pow2_scale(h, u, target_log2=t)
            assert torch.equal(out.isnan(), (h + u).isnan())
            got, want = _got(sc), _want([out], t)
            if got != want:
                fails.append(((r, cm, cb), t, got, want))
    h = torch.full((64, 288), float("nan"), device=DEV)
    out, sc = ops.add_pow2_scale(h, torch.full_like(h, float("inf")))
    if _got(sc) != (1.0, 1.0, 0):
        fails.append(("all non-finite", _got(sc)))
    assert not fails, f"{len(fails)} wrong scales (site, target, got (s, 1/s, bits), want): {fails[:6]}"


@pytest.mark.parametrize("bad", list(NONFINITE))
@pytest.mark.parametrize("irreps,out,gate,lmax", EPI)
def test_epilogue_scale_non_finite_next_to_maximum(irreps, out, gate, lmax, bad):
    """The non-finite value arrives through `residual`: in the maximum's 4-aligned column group (one float4 of the vector
    emit path), or in its column one row away inside the same 16-row tile (one lane of the scalar emit path)."""
    B = 203
    mod = _epi_module(irreps, out, lmax)
    g = torch.Generator(device=DEV).manual_seed(6)
    x = torch.randn(B, mod.in1_dim, device=DEV, generator=g) * 0.1
    y = torch.randn(B, mod.in2_dim, device=DEV, generator=g)
    fails = []
    with torch.no_grad():
        plain = mod.forward_fused([(x, None)], y, gate=gate)
        Wd = plain.shape[1]
        assert float(plain.abs().max()) + 4.0 < 4096.0     # below the binade of 7e3: a lost maximum changes s
        sites = [((37, 40), (37, 41)), ((37, 40), (38, 40)), ((37, 43), (36, 43)), ((200, Wd - 1), (200, Wd - 2)),
                 ((202, Wd - 4), (201, Wd - 4)), ((0, 0), (1, 0)), ((0, 0), (0, 3))]
        for aligned in (True, False):
            for (rm, cm), (rb, cb) in sites:
                res = _residual(plain.shape, aligned)
                res.copy_(_small(B, Wd, seed=rm + cm))
                res[rm, cm] = 7e3
                res[rb, cb] = NONFINITE[bad]
                for t in TARGETS:
                    o, sc = mod.forward_fused([(x, None)], y, gate=gate, residual=res, out_scale=t)
                    got, want = _got(sc), _want([o], t)
                    if got != want:
                        fails.append(("vector" if aligned else "scalar", (rm, cm), (rb, cb), t, got, want))
        res = torch.full(plain.shape, NONFINITE[bad], device=DEV)
        o, sc = mod.forward_fused([(x, None)], y, gate=gate, residual=res, out_scale=10)
        if _got(sc) != (1.0, 1.0, 0):
            fails.append(("all non-finite", _got(sc)))
    assert not fails, f"{len(fails)} wrong scales (emit path, max, non-finite, target, got (s, 1/s, bits), want): {fails[:6]}"

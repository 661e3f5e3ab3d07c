"""The fused node update with its weights one path ahead (run_paths_ahead in csrc/e3_tp_mfma_r16.hip) against the two-launch
path: the prefetch runs across paths, chunks, the two products and -- when a wave owns more than one tile -- across tiles,
and must not change a bit of what is summed.  Sizes: below / at / above one 16-row tile, several workgroups, and one size
derived from the device at which some waves run two tiles and the rest one (the only size that reaches the prefetch at the
top of a wave's second tile and its end)."""
import numpy as np
import pytest
import torch

import models  # noqa: F401
from scale_reference import expected_scale
from scalable_e3_gnn_amd import _lib
from scalable_e3_gnn_amd.tensor_product import SHTensorProduct

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = 32
HID = f"{H}x0e+{H}x1o+{H}x2e"
GATED = f"{H}x0e+{2 * H}x0e+{H}x1o+{H}x2e"
SIZES = [1, 15, 16, 17, 4099, "resident"]


def _rows(B):
    if B != "resident":
        return B
    # the launch keeps 2 workgroups of 4 waves on every CU: 16 rows for each resident wave, then one more tile and a
    # row for 17 of them
    waves = torch.cuda.get_device_properties(0).multi_processor_count * 2 * 4
    return 16 * waves + 17


@pytest.fixture(scope="module")
def pairs():
    made = {}
    for dtype in (torch.float32, torch.bfloat16):
        torch.manual_seed(11)
        made[dtype] = (SHTensorProduct(f"{HID}+{HID}", GATED, 2).to(DEV).to(dtype),
                       SHTensorProduct(HID, HID, 2).to(DEV).to(dtype))
    return made


def _inputs(B, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    h, a = torch.randn(B, 288, generator=g), torch.randn(B, 288, generator=g) * 3
    A = torch.randn(B, 9, generator=g)
    return h.to(dtype).to(DEV), a.to(dtype).to(DEV), A.to(DEV)


def _fused(upd1, upd2, h, a, A):
    with torch.no_grad():
        if h.dtype == torch.float32:
            got = upd1.forward_update_pair(upd2, [(h, None), (a, None)], A, residual=h, out_scale=10)
        else:
            got = upd1.forward_update_pair(upd2, [(h, None), (a, None)], A, residual=h), None
    assert _lib.load().e3_tp_last_fused_kernel() == b"e3::tp_update_pair_r16_kernel"
    return got


def _two_launch(upd1, upd2, h, a, A):
    with torch.no_grad():
        if h.dtype == torch.float32:
            u, us = upd1.forward_fused([(h, None), (a, None)], A, gate=True, out_scale=10)
            return upd2.forward_fused([(u, None)], A, gate=False, in_scale=us, residual=h, out_scale=10)
        u = upd1.forward_fused([(h, None), (a, None)], A, gate=True)
        return upd2.forward_fused([(u, None)], A, gate=False, residual=h), None


def _same_scale(sc, rsc):
    """{s, 1/s} bit for bit.  The third slot holds the bits of max |h'| itself, which follows the fp32 outputs and so may
    differ between the two paths by their last-place difference; it is not part of the scale."""
    assert torch.equal(sc[:2].view(torch.int32), rsc[:2].view(torch.int32))


@pytest.mark.parametrize("B", SIZES)
def test_bf16_bit_identical_to_two_launch(pairs, B):
    B = _rows(B)
    upd1, upd2 = pairs[torch.bfloat16]
    h, a, A = _inputs(B, 100 + B, torch.bfloat16)
    got, _ = _fused(upd1, upd2, h, a, A)
    ref, _ = _two_launch(upd1, upd2, h, a, A)
    assert got.shape == ref.shape and torch.equal(got.view(torch.int16), ref.view(torch.int16))


@pytest.mark.parametrize("B", SIZES)
def test_fp32_matches_two_launch_with_the_same_scale(pairs, B):
    B = _rows(B)
    upd1, upd2 = pairs[torch.float32]
    h, a, A = _inputs(B, 200 + B, torch.float32)
    got, sc = _fused(upd1, upd2, h, a, A)
    ref, rsc = _two_launch(upd1, upd2, h, a, A)
    g, r = got.double().cpu().numpy(), ref.double().cpu().numpy()
    err = float(np.abs(g - r).max() / np.abs(r).max())
    print(f"\nB={B}: fused vs two launches {err:.2e}")
    assert err <= 1e-5   # the tolerance of tests/test_node_update_gpu.py
    _same_scale(sc, rsc)
    s, inv, _ = expected_scale([got.cpu().numpy()], 10)
    assert (float(sc[0]), float(sc[1])) == (s, inv)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_inf_in_one_row_of_a_stays_there(pairs, dtype):
    """An inf in one row of the aggregated messages: that row of h' alone is non-finite and the scale ignores it (the
    operand-scale contract of include/e3gnn.h).  Row 40 is the ninth row of the third tile."""
    upd1, upd2 = pairs[dtype]
    B, bad = 83, 40
    h, a, A = _inputs(B, 300, dtype)
    a[bad, 170] = float("inf")
    got, sc = _fused(upd1, upd2, h, a, A)
    ref, rsc = _two_launch(upd1, upd2, h, a, A)
    g = got.double().cpu().numpy()
    assert np.flatnonzero(~np.isfinite(g).all(1)).tolist() == [bad]
    ok = np.arange(B) != bad
    if dtype == torch.bfloat16:
        assert torch.equal(got.view(torch.int16)[ok], ref.view(torch.int16)[ok])
    else:
        r = ref.double().cpu().numpy()
        assert np.abs(g[ok] - r[ok]).max() <= 1e-5 * np.abs(r[ok]).max()
        _same_scale(sc, rsc)
        s, inv, _ = expected_scale([got.cpu().numpy()], 10)
        assert (float(sc[0]), float(sc[1])) == (s, inv) and np.isfinite(s) and s > 0

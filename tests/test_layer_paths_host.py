"""``SEGNNLayer.paths`` -- the one place that chooses a layer's kernels -- against a literal table (no GPU: the shapes with
an MFMA instantiation are asked of the library through host-only plan handles, as ``fused_available`` does).

The table was written down once from the predicates that ``SEGNNLayer.forward`` held inline before the choice had a method
of its own (``r16`` / ``one_launch`` / ``r16u`` and the bf16 check), evaluated for every row below; it does not come from the
method.  Per layer and per flag switched off, eight letters: storage fp32 then bf16, inside that no gradient then gradient,
inside that without then with edge weights ``w``.
    O = ("one_launch", "fused")   P = ("per_product", "fused")   C = ("chain", "chain")   R = raises RuntimeError"""
import pytest
import torch

from scalable_e3_gnn_amd.segnn import SEGNN, SEGNNLayer

CODE = {"O": ("one_launch", "fused"), "P": ("per_product", "fused"), "C": ("chain", "chain")}
TABLE = {
    (1, 16, None): "OCCC RRRR",
    (1, 16, "fused"): "CCCC RRRR",
    (1, 16, "fuse_message"): "CCCC RRRR",
    (1, 16, "fuse_scatter"): "CCCC RRRR",
    (1, 32, None): "OPCC OPRR",
    (1, 32, "fused"): "CCCC RRRR",
    (1, 32, "fuse_message"): "PPCC PPRR",
    (1, 32, "fuse_scatter"): "PPCC PPRR",
    (2, 16, None): "OCCC RRRR",
    (2, 16, "fused"): "CCCC RRRR",
    (2, 16, "fuse_message"): "CCCC RRRR",
    (2, 16, "fuse_scatter"): "CCCC RRRR",
    (2, 32, None): "OPCC OPRR",
    (2, 32, "fused"): "CCCC RRRR",
    (2, 32, "fuse_message"): "PPCC PPRR",
    (2, 32, "fuse_scatter"): "PPCC PPRR",
    (2, 64, None): "OCCC ORRR",
    (2, 64, "fused"): "CCCC RRRR",
    (2, 64, "fuse_message"): "CCCC RRRR",
    (2, 64, "fuse_scatter"): "CCCC RRRR",
}
CALLS = [(dtype, grad, w) for dtype in (torch.float32, torch.bfloat16) for grad in (False, True) for w in (False, True)]


@pytest.mark.parametrize("lmax,H,off", list(TABLE), ids=[f"lmax{l}-H{h}-{o or 'default'}" for l, h, o in TABLE])
def test_paths_match_the_table(lmax, H, off):
    layer = SEGNNLayer(H, lmax)
    if off:
        setattr(layer, off, False)
    for (dtype, grad, w), want in zip(CALLS, TABLE[(lmax, H, off)].replace(" ", "")):
        tag = (lmax, H, off, dtype, grad, w)
        if want == "R":
            with pytest.raises(RuntimeError, match="bf16 storage needs the fused MFMA kernels"):
                layer.paths(dtype, grad, w)
        else:
            assert layer.paths(dtype, grad, w) == CODE[want], tag


@pytest.mark.parametrize("lmax,H,off", list(TABLE), ids=[f"lmax{l}-H{h}-{o or 'default'}" for l, h, o in TABLE])
def test_the_model_wants_edge_geometry_off_the_one_launch_path(lmax, H, off):
    """fp32 inference: SEGNN builds per-edge Y / d exactly when a layer is not on the one-launch path"""
    model = SEGNN("1x0e+1x1o", H, "1x1o", 2, lmax=lmax)
    if off:
        setattr(model.layers[1], off, False)
    one_launch = TABLE[(lmax, H, None)][0] == "O" and TABLE[(lmax, H, off)][0] == "O"   # layer 0 default, layer 1 as set
    assert model.wants_edge_geometry(torch.float32, False) == (not one_launch)
    for layer in model.layers:
        assert (layer.paths(torch.float32, False)[0] == "one_launch") == \
            (TABLE[(lmax, H, off if layer is model.layers[1] else None)][0] == "O")

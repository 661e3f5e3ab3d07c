"""Every instantiation of the message kernels (e3::msg_fused_kernel, e3::msg_ws_kernel, msg_premix_kernel,
msg_refresh_rows_kernel) against oracle/segnn_oracle.message_sums (numpy fp64) on the storage-rounded inputs, PER OUTPUT BLOCK:
max |got_l - want_l| / max |want_l| over the columns of degree l.  The cases, graphs and support tables are in
tests/msg_cases.py (checked on the host by tests/test_msg_cases_host.py); DESIGN.md §4.1c has the table of what reaches what.

Bounds: 1e-5 per block in fp32 storage, 2e-2 per block in bf16 storage (msg_cases.BOUND).  Every case also prefills ``out=``
with NaN where ``forward`` takes it (every row must come back finite) and wants the rows of nodes without an incoming edge to
be exactly zero.  Lines that start with "MSG " carry the measured figures."""
import ctypes

import numpy as np
import pytest
import torch

import msg_cases as C
import scale_reference as R
from scalable_e3_gnn_amd import _lib, ops
from scalable_e3_gnn_amd.radius_graph import radius_graph

pytestmark = pytest.mark.gpu
DEV = C.DEV
NAN_BITS = 0x7FC12345        # a quiet NaN with a payload: the padding of the ld_out case


def _ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


def _deg(name):
    return torch.as_tensor(np.diff(C.edges(name)[0]))


def _forward(layer, h, g, tpb, owned, **kw):
    """layer._msg.forward into a NaN-filled ``out=`` (not with ``cont``); the knobs are put back afterwards"""
    msg = layer._msg
    msg.tiles_per_block, msg.owned_sums = tpb, owned
    try:
        if "cont" not in kw:
            n = h.shape[0]
            kw["out"] = torch.full((n, msg.width), float("nan"), device=DEV)
        with torch.no_grad():
            res = msg.forward(h, g, layer.msg1, layer.msg2, **kw)
        if "out" in kw:
            assert (res[0] if isinstance(res, tuple) else res).data_ptr() == kw["out"].data_ptr()
        return res
    finally:
        msg.tiles_per_block, msg.owned_sums = 0, True


def _check(got, want, lmax, H, storage, deg, tag, bound=None):
    """finite rows, exact zeros for isolated nodes, per-block error below the bound of the storage type"""
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert bool(torch.isfinite(got).all()), f"{tag}: a row was not written"
    iso = (deg == 0).to(got.device)
    if bool(iso.any()):
        assert float(got[iso].abs().max()) == 0.0, f"{tag}: rows of isolated nodes"
    errs = C.block_errors(got, want, lmax, H)
    whole = float(np.abs(got.double().cpu().numpy() - want).max() / np.abs(want).max())   # printed only: the norm of the older tests
    print(f"MSG {storage} {tag}: per block " + " ".join(f"{e:.2e}" for e in errs) + f" | whole matrix {whole:.2e}")
    bound = C.BOUND[storage] if bound is None else bound
    for l, e in enumerate(errs):
        assert e < bound, (tag, l, e, errs)
    return errs


def _check_scale(scale, a, tag):
    s, inv, bits = R.expected_scale([a.cpu().numpy()], 10)
    got = scale.cpu()
    assert float(got[0]) == s and float(got[1]) == inv and int(got.view(torch.int32)[2]) == bits, \
        (tag, got.tolist(), s, inv, hex(bits))


def _launch_paths(lmax, H, storage):
    """(tiles_per_block, owned_sums, a scale comes back) for every way the library runs the shape"""
    return [(tpb, owned, owned and tpb >= 0 and C.OWNED[(lmax, H, storage)])
            for tpb in C.tiles_per_block_of(lmax, H) for owned in (True, False)]


# ---- a. every instantiation ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lmax,H,storage,per", C.TABLE, ids=_ids(C.TABLE))
def test_every_instantiation(lmax, H, storage, per):
    layer, h = C.layer(lmax, H, storage), C.features(lmax, H, storage)
    assert layer._msg.supports(h.dtype)
    for name in ("A", "B"):
        g, want, deg = C.graph(name, per), C.reference(lmax, H, storage, per, name), _deg(name)
        for tpb, owned, scaled in _launch_paths(lmax, H, storage):
            tag = f"lmax{lmax} H{H} {per} graph {name} tpb {tpb} owned {int(owned)}"
            got, scale = _forward(layer, h, g, tpb, owned, return_scale=True)
            assert (scale is not None) == scaled, tag
            _check(got, want, lmax, H, storage, deg, tag)
            if scale is not None:
                _check_scale(scale, got, tag)


@pytest.mark.parametrize("lmax,H", C.SHAPES, ids=_ids(C.SHAPES))
def test_uneven_blocks(lmax, H):
    """msg2's norm of degree l_max times 2^-7: the last block lies two orders of magnitude below the others, where the
    whole-matrix norm no longer sees an error in it"""
    layer, h = C.layer(lmax, H, "fp32", True), C.features(lmax, H, "fp32")
    for name in ("A", "B"):
        g, want, deg = C.graph(name, "open"), C.reference(lmax, H, "fp32", "open", name, True), _deg(name)
        tops = [float(np.abs(want[:, s]).max()) for s in C.blocks(lmax, H)]
        assert tops[-1] < 0.05 * min(tops[:-1]), tops
        for tpb, owned, _ in _launch_paths(lmax, H, "fp32"):
            got = _forward(layer, h, g, tpb, owned)
            _check(got, want, lmax, H, "fp32", deg, f"uneven lmax{lmax} H{H} graph {name} tpb {tpb} owned {int(owned)}")


# ---- b. accumulating launch with a refresh of the ghost rows ---------------------------------------------------------
_SHAPES_ST = sorted({(l, H, st) for (l, H, st, _) in C.TABLE})


@pytest.mark.parametrize("stale", ["zeros", "same magnitude"])
@pytest.mark.parametrize("lmax,H,storage", _SHAPES_ST, ids=_ids(_SHAPES_ST))
def test_accumulating_launch_with_refresh(lmax, H, storage, stale):
    """The sharded layer's sequence: the edges with an owned source while the ghost rows (the last rows: sources only) are
    stale, the ghost rows overwritten, refresh_row_max, the ghost-source edges with ``cont=``.  Reference: all edges, true h."""
    layer, h_true = C.layer(lmax, H, storage), C.features(lmax, H, storage)
    g, want, deg = C.graph("A", "open"), C.reference(lmax, H, storage, "open", "A"), _deg("A")
    rows = torch.arange(C.N - C.GHOSTS, C.N, device=DEV)
    ghost = g.src >= C.N - C.GHOSTS
    own_edges = (g.src[~ghost].contiguous(), g.dst[~ghost].contiguous())
    ghost_edges = (g.src[ghost].contiguous(), g.dst[ghost].contiguous())
    assert 0 < ghost_edges[0].numel() < g.num_edges
    f32 = storage == "fp32"
    for tpb in C.tiles_per_block_of(lmax, H):
        h = h_true.clone()
        if stale == "zeros":
            h[rows] = 0
        else:
            h[rows] = torch.randn(C.GHOSTS, h.shape[1], generator=torch.Generator().manual_seed(9)).to(h.dtype).to(DEV)
        sc = ops.pow2_scale([h], target_log2=6) if f32 else None
        a, state = _forward(layer, h, g, tpb, True, in_scale=sc, edges=own_edges, return_state=True)
        assert bool(torch.isfinite(a).all())
        h[rows] = h_true[rows]
        top = layer._msg.refresh_row_max(state, h, rows, sc)
        s = float(sc[0]) if f32 else 1.0
        assert float(top) == float(h_true[rows].float().abs().max()) * s, (float(top), s)
        got = _forward(layer, h, g, tpb, True, in_scale=sc, edges=ghost_edges, cont=state)
        assert got.data_ptr() == a.data_ptr()
        _check(got, want, lmax, H, storage, deg, f"accumulate lmax{lmax} H{H} stale {stale} tpb {tpb}")


# ---- c. a feature matrix with a row stride above its width -----------------------------------------------------------
_STRIDE = [(16, "fp32"), (32, "fp32"), (32, "bf16"), (64, "fp32"), (64, "bf16")]


@pytest.mark.parametrize("H,storage", _STRIDE, ids=_ids(_STRIDE))
def test_row_stride_of_h(H, storage):
    """h as a view with ld_h = W + 16 bytes (rows stay 16-byte aligned: forward passes the view on), NaN in the row tails.
    Same bits as on the contiguous copy where the sums are owned (hidden 32: reproducible); the other shapes sum by fp32
    atomics in no fixed order and agree within 3e-6 of the matrix, the bound between two fp32 message paths."""
    lmax = 2
    layer, h = C.layer(lmax, H, storage), C.features(lmax, H, storage)
    W, pad = h.shape[1], 16 // h.element_size()
    big = torch.full((C.N, W + pad), float("nan"), dtype=h.dtype, device=DEV)
    big[:, :W] = h
    hv = big[:, :W]
    assert hv.stride(0) == W + pad and not hv.is_contiguous()
    assert hv.stride(1) == 1 and (hv.stride(0) * hv.element_size()) % 16 == 0 and hv.data_ptr() % 16 == 0   # no copy in forward
    g, want, deg = C.graph("A", "open"), C.reference(lmax, H, storage, "open", "A"), _deg("A")
    for tpb, owned, scaled in _launch_paths(lmax, H, storage):
        tag = f"ld_h H{H} tpb {tpb} owned {int(owned)}"
        got = _forward(layer, hv, g, tpb, owned)
        ref = _forward(layer, h, g, tpb, owned)
        _check(got, want, lmax, H, storage, deg, tag)
        if scaled:
            assert torch.equal(got, ref), tag
            if storage == "bf16":
                assert torch.equal(got.bfloat16(), ref.bfloat16())
        else:
            dev = float((got - ref).abs().max() / ref.abs().max())
            assert dev < 3e-6, (tag, dev)
    assert bool(torch.isnan(big[:, W:]).all())


# ---- d. ld_out above the width (the C entries directly) --------------------------------------------------------------
def _direct(layer, h, g, tpb, owned, ld_out):
    """e3_msg_premix + e3_msg_forward / e3_msg_forward_owned into a [N, ld_out] buffer filled with NAN_BITS"""
    lib, dev, msg = _lib.load(), torch.device(DEV), layer._msg
    n, W = h.shape
    E = g.num_edges
    code = _lib.dtype_code(h.dtype)
    out = torch.full((n, ld_out), NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    scale = None
    with torch.cuda.device(dev), torch.no_grad():
        hd = msg._plans.handle(dev)
        packed = msg.packed(layer.msg1, layer.msg2, dev, h.dtype)
        sc = ops.pow2_scale([h]) if h.dtype == torch.float32 else None
        scp = sc.data_ptr() if sc is not None else None
        stream = torch.cuda.current_stream(dev).cuda_stream
        premix = torch.empty(n * int(lib.e3_msg_premix_floats_per_node(hd)), dtype=torch.float32, device=DEV)
        _lib.check(lib.e3_msg_premix(hd, h.data_ptr(), h.stride(0), n, packed.data_ptr(), scp, premix.data_ptr(), code, stream),
                   "e3_msg_premix")
        head = (hd, h.data_ptr(), h.stride(0), n, g.pos4.data_ptr(), g.src.data_ptr(), g.dst.data_ptr(), E, packed.data_ptr(),
                scp, premix.data_ptr(), out.data_ptr(), ld_out, code)
        if owned:
            wsb = int(lib.e3_msg_owned_workspace_bytes(hd, E, code, tpb))
            assert wsb > 0
            work = torch.empty(wsb, dtype=torch.uint8, device=DEV)
            scale = torch.empty(4, dtype=torch.float32, device=DEV)
            _lib.check(lib.e3_msg_forward_owned(*head, tpb, work.data_ptr(), wsb, scale.data_ptr(), 10, stream),
                       "e3_msg_forward_owned")
        else:
            _lib.check(lib.e3_msg_forward(*head, 0, tpb, stream), "e3_msg_forward")
        torch.cuda.synchronize()
    return out, scale


_LD_OUT = [(2, 32, False, 0), (2, 32, False, -1), (1, 16, False, 0), (2, 32, True, 0), (2, 32, True, 1)]


@pytest.mark.parametrize("lmax,H,owned,tpb", _LD_OUT, ids=_ids(_LD_OUT))
def test_ld_out_above_the_width(lmax, H, owned, tpb):
    layer, h = C.layer(lmax, H, "fp32"), C.features(lmax, H, "fp32")
    W = h.shape[1]
    for name in ("A", "B"):
        g, want, deg = C.graph(name, "open"), C.reference(lmax, H, "fp32", "open", name), _deg(name)
        out, scale = _direct(layer, h, g, tpb, owned, W + 4)
        assert bool((out.view(torch.int32)[:, W:] == NAN_BITS).all()), "the padding behind the rows was written"
        got = out[:, :W].contiguous()
        tag = f"ld_out lmax{lmax} H{H} graph {name} tpb {tpb} owned {int(owned)}"
        _check(got, want, lmax, H, "fp32", deg, tag)
        if owned:
            _check_scale(scale, got, tag)
            assert torch.equal(got, _forward(layer, h, g, tpb, True)), tag   # owned sums: the same bits at any ld_out


# ---- e. the outer loop of the one-wave-per-tile kernel ---------------------------------------------------------------
@pytest.mark.parametrize("lmax,H", [(1, 16), (2, 64)], ids=["lmax1-H16", "lmax2-H64"])
def test_outer_loop_of_the_one_wave_per_tile_kernel(lmax, H):
    """tiles_per_block = -1: blocks of one tile.  The grid is at most 4 workgroups of 4 waves per CU, so with more than
    16 x 4 x 4 x CUs edges every wave walks more than one block (1.25 x that: the split into eighths leaves no wave idle)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    need = 1.25 * 16 * 4 * 4 * cus
    n = int(need / 10)
    pos = torch.rand(n, 3, generator=torch.Generator().manual_seed(12))
    g = radius_graph(pos.to(DEV), float((3 * 14.0 / (4 * np.pi * n)) ** (1 / 3)), [0, 0, 0], [1, 1, 1])
    E = g.num_edges
    print(f"MSG outer loop: {cus} CUs, {n} nodes, {E} edges (> {need:.0f})")
    assert E > need, (E, need)
    layer = C.layer(lmax, H, "fp32")
    h = torch.randn(n, C.width(lmax, H), generator=torch.Generator().manual_seed(13)).to(DEV)
    got = _forward(layer, h, g, -1, False)
    other = _forward(layer, h, g, -4, False)
    assert bool(torch.isfinite(got).all())
    dev = float((got - other).abs().max() / other.abs().max())
    print(f"MSG outer loop lmax{lmax} H{H}: tiles_per_block -1 vs -4 {dev:.2e}")
    assert dev < 3e-6, dev
    # 64 destination rows against the oracle on the edges into them
    src, dst = g.src.cpu().numpy().astype(np.int64), g.dst.cpu().numpy().astype(np.int64)
    degs = np.bincount(dst, minlength=n)
    cand = np.flatnonzero(degs > 0)
    rows = np.unique(np.concatenate([cand[[0, -1]], np.random.default_rng(14).choice(cand, 62, replace=False)]))
    sel = np.isin(dst, rows)
    p64 = g.pos4[:, :3].double().cpu().numpy()
    want = C.oracle(layer, h, lmax, H, p64[src[sel]] - p64[dst[sel]], src[sel], dst[sel], n)[rows]
    part = got[torch.as_tensor(rows, device=DEV)]
    _check(part, want, lmax, H, "fp32", torch.ones(len(rows)), f"outer loop lmax{lmax} H{H}: {len(rows)} rows, {int(sel.sum())} edges")
    iso = torch.as_tensor(degs == 0, device=DEV)
    if bool(iso.any()):
        assert float(got[iso].abs().max()) == 0.0


# ---- f. the cache of the packed weights ------------------------------------------------------------------------------
@pytest.mark.parametrize("lmax,H,storage", [(2, 32, "fp32"), (1, 64, "bf16"), (2, 16, "fp32")], ids=["lmax2-H32-fp32", "lmax1-H64-bf16",
                                                                                                   "lmax2-H16-fp32"])
def test_packed_weights_follow_the_tensors(lmax, H, storage):
    """FusedMessage.packed keys its image on (data_ptr, _version) of the twelve tensors: an in-place change of a weight, of
    a norm buffer and a load_state_dict must each reach the next forward; a stale image would be a silent wrong answer."""
    layer = C.make_layer(lmax, H, storage)
    h, g, deg = C.features(lmax, H, storage), C.graph("A", "open"), _deg("A")
    _, src, dst = C.edges("A")
    rel = C.edge_vectors(C.positions(), src, dst, "open")
    bound = C.BOUND[storage]

    def step(tag, before):
        want = C.oracle(layer, h, lmax, H, rel, src, dst, C.N)
        got = _forward(layer, h, g, 0, True)
        _check(got, want, lmax, H, storage, deg, f"cache lmax{lmax} H{H} {tag}")
        if before is not None:   # the change is one the bound sees
            assert max(C.block_errors(before, want, lmax, H)) > 10 * bound, tag
        again = _forward(layer, h, g, 0, True)
        if C.OWNED[(lmax, H, storage)]:
            assert torch.equal(again, got), tag
        return got

    got = step("as built", None)
    with torch.no_grad():
        getattr(layer.msg2, "weights_" + C.NAT[1]).mul_(1.5)
    got = step("msg2 weight x 1.5", got)
    with torch.no_grad():
        getattr(layer.msg1, "norm_" + C.NAT[0]).mul_(0.5)
    got = step("msg1 norm x 0.5", got)
    layer.load_state_dict(C.make_layer(lmax, H, storage, seed=1).state_dict())
    step("load_state_dict", got)


# ---- g. refusals -----------------------------------------------------------------------------------------------------
E3_ERR_INVALID_ARG, E3_ERR_UNSUPPORTED = 1, 4


def test_plan_create_refuses():
    lib = _lib.load()
    for lmax, H, code in [(3, 32, E3_ERR_INVALID_ARG), (0, 32, E3_ERR_INVALID_ARG), (2, 8, E3_ERR_UNSUPPORTED),
                          (1, 48, E3_ERR_UNSUPPORTED), (2, 48, E3_ERR_UNSUPPORTED)]:
        h = ctypes.c_void_p()
        assert lib.e3_msg_plan_create(lmax, H, ctypes.byref(h)) == code, (lmax, H)
        assert not h.value


def _canary(numel, dtype=torch.float32):
    t = torch.full((numel,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    return t.view(dtype) if dtype != torch.int32 else t


@pytest.mark.parametrize("lmax", C.LMAX)
def test_bf16_at_hidden_16_is_refused(lmax):
    """every entry answers E3_ERR_UNSUPPORTED from its host-side checks: nothing is launched, no buffer is touched"""
    H = 16
    lib, dev = _lib.load(), torch.device(DEV)
    layer = C.layer(lmax, H, "fp32")
    msg = layer._msg
    assert not msg.supports(torch.bfloat16)
    g = C.graph("A", "open")
    n, W, E = C.N, C.width(lmax, H), g.num_edges
    hb = C.features(lmax, H, "fp32").bfloat16()
    with torch.cuda.device(dev):
        hd = msg._plans.handle(dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        packed = _canary(int(lib.e3_msg_packed_bytes(hd)) // 4)
        premix = _canary(n * int(lib.e3_msg_premix_floats_per_node(hd)))
        out = _canary(n * W)
        keep = [t.clone() for t in (packed, premix, out)]
        P3 = ctypes.c_void_p * 3
        ws, ns = msg._tensors(layer.msg1)
        w1 = [t.detach().bfloat16() if t is not None else None for t in ws + ns]
        ws, ns = msg._tensors(layer.msg2)
        w2 = [t.detach().bfloat16() if t is not None else None for t in ws + ns]
        ptr = lambda t: t.data_ptr() if (t is not None and t.numel()) else None
        assert lib.e3_msg_pack_weights(hd, P3(*map(ptr, w1[0:3])), P3(*map(ptr, w1[3:6])), P3(*map(ptr, w2[0:3])),
                                       P3(*map(ptr, w2[3:6])), _lib.E3_BF16, packed.data_ptr(), stream) == E3_ERR_UNSUPPORTED
        assert lib.e3_msg_premix(hd, hb.data_ptr(), hb.stride(0), n, packed.data_ptr(), None, premix.data_ptr(), _lib.E3_BF16,
                                 stream) == E3_ERR_UNSUPPORTED
        rows = torch.arange(n - C.GHOSTS, n, device=DEV)
        assert lib.e3_msg_refresh_rows(hd, hb.data_ptr(), hb.stride(0), n, rows.data_ptr(), rows.numel(), None,
                                       premix.data_ptr(), _lib.E3_BF16, stream) == E3_ERR_UNSUPPORTED
        for tpb in (0, -1):
            assert lib.e3_msg_forward(hd, hb.data_ptr(), hb.stride(0), n, g.pos4.data_ptr(), g.src.data_ptr(), g.dst.data_ptr(),
                                      E, packed.data_ptr(), None, premix.data_ptr(), out.data_ptr(), W, _lib.E3_BF16, 0, tpb,
                                      stream) == E3_ERR_UNSUPPORTED
        with pytest.raises(RuntimeError):
            msg.forward(hb, g, layer.msg1, layer.msg2)
        torch.cuda.synchronize()
        for t, k in zip((packed, premix, out), keep):
            assert torch.equal(t.view(torch.int32), k.view(torch.int32))


_NO_WS = [(1, 16, 0), (1, 32, 0), (2, 64, 0), (2, 16, 2), (2, 32, -1), (2, 32, -4)]


@pytest.mark.parametrize("lmax,H,tpb", _NO_WS, ids=_ids(_NO_WS))
def test_forward_owned_refuses_without_the_weights_stationary_kernel(lmax, H, tpb):
    lib, dev = _lib.load(), torch.device(DEV)
    layer, h, g = C.layer(lmax, H, "fp32"), C.features(lmax, H, "fp32"), C.graph("A", "open")
    msg = layer._msg
    n, W, E = C.N, C.width(lmax, H), g.num_edges
    with torch.cuda.device(dev), torch.no_grad():
        hd = msg._plans.handle(dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        assert int(lib.e3_msg_owned_workspace_bytes(hd, E, _lib.E3_F32, tpb)) == -1
        packed = msg.packed(layer.msg1, layer.msg2, dev)
        sc = ops.pow2_scale([h])
        premix = torch.empty(n * int(lib.e3_msg_premix_floats_per_node(hd)), dtype=torch.float32, device=DEV)
        _lib.check(lib.e3_msg_premix(hd, h.data_ptr(), h.stride(0), n, packed.data_ptr(), sc.data_ptr(), premix.data_ptr(),
                                     _lib.E3_F32, stream), "e3_msg_premix")
        out, work, scale = _canary(n * W), _canary(1 << 16), _canary(4)
        keep = [t.clone() for t in (out, work, scale)]
        st = lib.e3_msg_forward_owned(hd, h.data_ptr(), h.stride(0), n, g.pos4.data_ptr(), g.src.data_ptr(), g.dst.data_ptr(), E,
                                      packed.data_ptr(), sc.data_ptr(), premix.data_ptr(), out.data_ptr(), W, _lib.E3_F32, tpb,
                                      work.data_ptr(), work.numel() * 4, scale.data_ptr(), 10, stream)
        assert st == E3_ERR_UNSUPPORTED, st
        torch.cuda.synchronize()
        for t, k in zip((out, work, scale), keep):
            assert torch.equal(t.view(torch.int32), k.view(torch.int32))

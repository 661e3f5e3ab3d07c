"""The two kernels of the differentiable ghost refresh (csrc/e3_halo_grad.hip) against their torch restatements, bit for
bit: values are dyadic (small integers / 8), so every sum is exact in any order.  ``e3_halo_refresh`` must equal
``h.clone().index_copy_(0, recv_idx, recv)`` and leave ``h`` alone; ``e3_halo_reduce`` must equal zero-the-ghost-rows +
``index_add``.  Row widths 1, 3 (the position gradient), 64, 72 and 288 (hidden widths), tight and padded leading dimensions
(D + 5: no 16-byte access possible), row counts around one wave / one block and 1000, fp32 and fp64, no ghosts at all, and a
send list in which one row appears 7 times, one once and most never.  Then ``Halo.refresh`` as an autograd node on a
world-1 periodic self-halo: the gradient of ``(refresh(h) * v).sum()`` is the reduce of ``v``, exactly."""
import numpy as np
import pytest
import torch

import models  # noqa: F401
from scalable_e3_gnn_amd import _lib
from scalable_e3_gnn_amd.sharding import GridHalo, halo_reduce_torch, halo_refresh_torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD_VALUE = -77.0


def _dyadic(rng, shape, dtype):
    return torch.as_tensor(rng.integers(-64, 65, size=shape) / 8.0).to(dtype)


def _padded(t, pad):
    """-> (buffer [n, D + pad] on the device filled with PAD_VALUE outside t, its [n, D] view)."""
    n, D = t.shape
    buf = torch.full((n, D + pad), PAD_VALUE, dtype=t.dtype, device=DEV)
    buf[:, :D] = t.to(DEV)
    return buf, buf[:, :D]


def _case(rng, n, ghosts, dtype, D):
    """Index lists of a local cloud of n rows -> (recv_idx [n_ghost], send_idx [n_send] over owned rows)."""
    n_ghost = min(n // 3, n - 1) if (ghosts and n > 1) else 0
    rows = rng.permutation(n)
    recv_idx, owned = rows[:n_ghost], rows[n_ghost:]
    if n == 0:
        send = np.zeros(0, np.int64)
    elif len(owned) < 8:
        send = np.repeat(owned[:1], 3)
    else:
        # one row 7 times, one row once, a few rows twice or three times, most rows never
        send = np.concatenate([np.repeat(owned[0], 7), owned[1:2], np.repeat(owned[2:5], 2), np.repeat(owned[5:7], 3)])
        send = send[rng.permutation(len(send))]
    return torch.as_tensor(recv_idx, dtype=torch.long), torch.as_tensor(send, dtype=torch.long)


def _maps(n, recv_idx, send_idx):
    slot = np.full(n, -1, np.int32)
    slot[recv_idx.numpy()] = np.arange(len(recv_idx), dtype=np.int32)
    red_k = np.argsort(send_idx.numpy(), kind="stable").astype(np.int32)
    red_ptr = np.concatenate([[0], np.cumsum(np.bincount(send_idx.numpy(), minlength=n))]).astype(np.int32)
    return [torch.as_tensor(a).to(DEV) for a in (slot, red_ptr, red_k)]


def _ptr(t):
    return t.data_ptr() if t.numel() else None


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("D", [1, 3, 64, 72, 288])
def test_kernels_equal_torch_restatement(D, dtype):
    lib = _lib.load()
    code = _lib.dtype_code(dtype)
    rng = np.random.default_rng(D)
    seen7 = False
    for n in (0, 1, 63, 65, 1000):
        for ghosts in (True, False):
            recv_idx, send_idx = _case(rng, n, ghosts, dtype, D)
            ng, ns = len(recv_idx), len(send_idx)
            counts = np.bincount(send_idx.numpy(), minlength=max(n, 1))
            seen7 |= n >= 63 and counts.max() == 7 and (counts == 1).any() and (counts == 0).sum() > n // 2
            slot, red_ptr, red_k = _maps(n, recv_idx, send_idx)
            h, recv, g, back = (_dyadic(rng, (m, D), dtype) for m in (n, ng, n, ns))
            want_refresh = halo_refresh_torch(h, recv, recv_idx)
            want_reduce = halo_reduce_torch(g, back, recv_idx, send_idx)
            for pad in (0, 5):
                (hb, hv), (rb, rv), (gb, gv), (bb, bv) = (_padded(t, pad) for t in (h, recv, g, back))
                hb0 = hb.clone()
                ob, ov = _padded(torch.zeros(n, D, dtype=dtype), pad)
                ld = D + pad
                assert lib.e3_halo_refresh(_ptr(hb), ld, _ptr(rb), ld, ng, _ptr(slot), n, D, code, _ptr(ob), ld,
                                           _stream()) == 0
                assert torch.equal(ov.cpu(), want_refresh), (n, ghosts, pad)
                assert torch.equal(hb, hb0)                                   # h is not written
                assert bool((ob[:, D:] == PAD_VALUE).all())                   # nor anything past column D
                ob, ov = _padded(torch.zeros(n, D, dtype=dtype), pad)
                assert lib.e3_halo_reduce(_ptr(gb), ld, _ptr(bb), ld, ns, _ptr(slot), _ptr(red_ptr), _ptr(red_k), n, D, code,
                                          _ptr(ob), ld, _stream()) == 0
                assert torch.equal(ov.cpu(), want_reduce), (n, ghosts, pad)
                assert bool((ob[:, D:] == PAD_VALUE).all())
    assert seen7                                                              # the 7 / 1 / never send list did occur


def test_bad_arguments_are_rejected_without_a_launch():
    lib = _lib.load()
    n, D, ng, ns = 8, 4, 2, 3
    t = lambda rows: torch.zeros((rows, D), device=DEV)
    h, recv, back, out = t(n), t(ng), t(ns), t(n)
    slot = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    slot[:ng] = torch.arange(ng, dtype=torch.int32, device=DEV)
    red_ptr = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    red_ptr[ng + 1:] = ns
    red_k = torch.arange(ns, dtype=torch.int32, device=DEV)
    s = _stream()

    def refresh(h=h.data_ptr(), ld_h=D, recv=recv.data_ptr(), ld_r=D, ng=ng, slot=slot.data_ptr(), n=n, D=D, dt=0,
                out=out.data_ptr(), ld_o=D):
        return lib.e3_halo_refresh(h, ld_h, recv, ld_r, ng, slot, n, D, dt, out, ld_o, s)

    def reduce(g=h.data_ptr(), ld_g=D, back=back.data_ptr(), ld_b=D, ns=ns, slot=slot.data_ptr(), ptr=red_ptr.data_ptr(),
               k=red_k.data_ptr(), n=n, D=D, dt=0, out=out.data_ptr(), ld_o=D):
        return lib.e3_halo_reduce(g, ld_g, back, ld_b, ns, slot, ptr, k, n, D, dt, out, ld_o, s)

    assert refresh() == 0 and reduce() == 0 and refresh(dt=1) == 0 and reduce(dt=1) == 0
    for fn, ptrs, lds in ((refresh, ("h", "recv", "slot", "out"), ("ld_h", "ld_r", "ld_o")),
                          (reduce, ("g", "back", "slot", "ptr", "k", "out"), ("ld_g", "ld_b", "ld_o"))):
        for name in ptrs:
            assert fn(**{name: None}) == 1, name                             # NULL with n > 0
        for name in lds:
            assert fn(**{name: D - 1}) == 1, name                            # leading dimension below D
        assert fn(D=0) == 1 and fn(D=-3) == 1 and fn(n=-1) == 1
        assert fn(dt=2) == 1 and fn(dt=7) == 1 and fn(dt=-1) == 1           # bf16 / unknown dtypes
    assert refresh(ng=-1) == 1 and reduce(ns=-1) == 1
    # n = 0 and n_ghost = 0 / nothing sent are valid, with NULL buffers
    assert refresh(n=0, h=None, recv=None, slot=None, out=None, ng=0) == 0
    assert reduce(n=0, g=None, back=None, slot=None, ptr=None, k=None, out=None, ns=0) == 0
    slot.fill_(-1)
    assert refresh(recv=None, ng=0) == 0 and reduce(back=None, ptr=None, k=None, ns=0) == 0
    torch.cuda.synchronize()
    assert not out.any()                                                      # all-zero inputs; nothing else was written


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_refresh_gradient_is_the_reduce_world1_self_halo(dtype):
    from scalable_e3_gnn_amd.radius_graph import radius_graph
    M, D, r = 300, 72, 1.0 / 4.2
    rng = np.random.default_rng(9)
    pos = torch.as_tensor((rng.integers(0, 1 << 16, size=(M, 3)) / float(1 << 16)).astype(np.float32)).to(DEV)
    halo = GridHalo((1, 1, 1), (0, 0, 0), (1, 1, 1), periodic=True)
    lpos, ids = halo.setup(pos, torch.arange(M, dtype=torch.float32, device=DEV)[:, None], r)
    g = radius_graph(lpos, r, *halo.local_bounds(r))
    halo.renumber(g.perm)
    n = lpos.shape[0]
    assert halo.n_ghost > M and halo.neighbours == []
    assert int((halo._maps()[1][1:] - halo._maps()[1][:-1]).max()) == 7     # a corner particle has 7 images
    owner = ids[g.perm.long(), 0].long()                                     # owned particle behind every local row
    h = _dyadic(rng, (n, D), dtype).to(DEV).requires_grad_(True)
    v = _dyadic(rng, (n, D), dtype).to(DEV)
    out = halo.refresh(h)
    with torch.no_grad():
        want = halo.exchange(h.detach().clone())                             # the in-place inference refresh
    assert torch.equal(out.detach(), want) and out.data_ptr() != h.data_ptr()
    (out * v).sum().backward()
    # the reduce of v, restated with the owner ids: an owned row collects its own v and the v of all its images
    own_rows = halo.owned_new
    row_of_owner = torch.empty(M, dtype=torch.long, device=DEV)
    row_of_owner[owner[own_rows]] = own_rows
    ghost = halo.is_ghost
    want_grad = torch.where(ghost[:, None], torch.zeros_like(v), v).index_add_(0, row_of_owner[owner[ghost]], v[ghost])
    assert torch.equal(h.grad, want_grad)
    assert torch.equal(halo.reduce_ghosts(v), want_grad[own_rows])
    assert halo.anchor.grad is not None and float(halo.anchor.grad) == 0.0

"""SEGNN forward built on ``L1TensorProduct`` (builder-defined architecture: the reference mount has
only the tensor product; this file is the repo's written contract for the rest).

Steerable E(3) message passing with ``l_max`` 1 (``Hx0e+Hx1o`` hidden features, every TP is the
reference operator) or 2 (``Hx0e+Hx1o+Hx2e``, TPs = ``SHTensorProduct``), for a radius graph given
as CSR-by-dst in Morton order (``radius_graph``):

    Y_e = SH_{l<=1}(x_src - x_dst)  (component norm.),  d_e = |x_src - x_dst|,  A_i = [1, mean_e Y1_e]
    h   = TP_embed(x ; A)
    per layer:
        m  = gate(TP_m1([h_dst | h_src | d] ; Y));   m = gate(TP_m2(m ; Y))
        a_i = sum_{e -> i} m_e
        u  = gate(TP_u1([h | a] ; A));               u = TP_u2(u ; A)
        h  = h + u
    out = TP_out(h ; A)

``gate``: TP output ``Hx0e + Hx0e + Hx1o`` = (scalars, gate scalars, vectors) -> ``silu(s)``, ``sigmoid(g) v``.
Every TP is the reference operator (`L1TensorProduct`), i.e. the pinned hot path.
"""
from __future__ import annotations

import torch
from torch import nn

from . import ops
from .irreps import Irreps
from .l1_tensor_prod import L1TensorProduct
from .message import FusedMessage
from .radius_graph import RadiusGraph
from .tensor_product import SHTensorProduct


def _hidden_irreps(H: int, lmax: int):
    hid = Irreps(f"{H}x0e+{H}x1o" + (f"+{H}x2e" if lmax == 2 else ""))
    gated = Irreps(f"{H}x0e+{lmax * H}x0e+{H}x1o" + (f"+{H}x2e" if lmax == 2 else ""))
    return hid, gated


def _make_tp(in_irreps, out_irreps, lmax: int):
    """l_max = 1: the reference operator (pinned).  l_max = 2: its builder-defined generalisation -- also used with
    lmax_sh = 1 for the shapes the reference class rejects (it asserts lmax == 1 on both irreps, l1_tensor_prod.py:13-14,
    so a scalar-only head such as the 1x0e energy readout cannot be an L1TensorProduct)."""
    if lmax == 1:
        if Irreps(in_irreps).lmax == 1 and Irreps(out_irreps).lmax == 1:
            return L1TensorProduct(in_irreps, out_irreps)
        return SHTensorProduct(in_irreps, out_irreps, lmax_sh=1)
    return SHTensorProduct(in_irreps, out_irreps, lmax_sh=2)


_PERIODIC_NOT_SHARDED = ("a periodic graph cannot be sharded (halo / split): build the local graph OPEN over the ghost images "
                         "of GridHalo(..., periodic=...)")
_ENVELOPE_NEEDS_BOTH = ("the cutoff envelope on the sharded path works on the split graph with a refresh per layer: halo= and "
                        "split= (halo.split_graph) come together; one without the other is not implemented")


class SEGNNLayer(nn.Module):
    _warned_unfused = False   # the fused -> unfused switch is announced once per process

    def __init__(self, H: int, lmax: int = 1):
        super().__init__()
        hid, gated = _hidden_irreps(H, lmax)
        self.H, self.lmax = H, lmax
        self.fused = True           # fused gather + TP + gate (+ segment-sum) kernels when the shapes allow it
        self.fuse_scatter = True    # segment-sum inside the message kernel.  The one-launch message kernel for hidden 32,
        #                             l_max = 2 writes every row once (FusedMessage.owned_sums): reproducible from run to
        #                             run.  The other fused kernels (and sharded / accumulating launches) sum by fp32
        #                             atomics: sums agree to fp32 rounding, not bit for bit.
        #                             False = separate, bitwise reproducible e3_segment_sum
        self.fuse_message = True    # fp32: the whole message function in one launch (message.FusedMessage)
        self._msg = FusedMessage(lmax, H) if FusedMessage.supported(lmax, H) else None
        self.msg1 = _make_tp(hid + hid + Irreps("1x0e"), gated, lmax)
        self.msg2 = _make_tp(hid, gated, lmax)
        self.upd1 = _make_tp(hid + hid, gated, lmax)
        self.upd2 = _make_tp(hid, hid, lmax)

    def _gate(self, t):
        H = self.H
        return ops.gate(t, H, H) if self.lmax == 1 else ops.gate_blocks(t, H, [(1, H), (2, H)])

    def fused_available(self) -> bool:
        """Static part only (shapes with an MFMA instantiation); grad mode is looked at on every call.  True when the
        per-product fused kernels exist for BOTH message products and the update product."""
        f = getattr(self, "_fused_ok", None)
        if f is None:
            f = self._fused_ok = all(tp.fused_supported(True) for tp in (self.msg1, self.msg2, self.upd1))
        return f

    def fused_update_available(self) -> bool:
        """The update product alone (gather + concat + TP + gate in one launch) -- enough when the one-launch message kernel
        handles the messages (hidden 16 / 64: only the node-level products have per-product MFMA instantiations)."""
        f = getattr(self, "_fused_upd_ok", None)
        if f is None:
            f = self._fused_upd_ok = bool(self.upd1.fused_supported(True))
        return f

    def paths(self, dtype, needs_grad: bool, weighted: bool = False):
        """The kernels a call runs -> (message path, update path), from what ``forward`` can observe: the storage dtype,
        whether a gradient is needed, whether edge weights ``w`` are given, and the three flags.

        message: "one_launch" (``FusedMessage``: both products, both gates and the sums in one launch; it sums with weight
        1, so not with ``w``), "per_product" (gather + TP + gate per product, needs an MFMA instantiation of both message
        products and update #1) or "chain" (the differentiable chain on the generic kernels).
        update: "fused" or "chain".  bf16 storage has the fused kernels only: a RuntimeError otherwise."""
        fast = self.fused and not needs_grad
        per_product = fast and self.fused_available()
        one_launch = (fast and self.fuse_message and self.fuse_scatter and self._msg is not None and
                      self._msg.supports(dtype) and not weighted)
        fused_update = per_product or (one_launch and self.fused_update_available())
        if dtype == torch.bfloat16 and not ((one_launch or per_product) and fused_update):
            raise RuntimeError("bf16 storage needs the fused MFMA kernels (inference; hidden 32, or 64 at l_max = 2)")
        return ("one_launch" if one_launch else "per_product" if per_product else "chain",
                "fused" if fused_update else "chain")

    def forward(self, h, g: RadiusGraph, Y, d, A, h_scale=None, halo=None, split=None, w=None):
        """-> (h_next, operand scale of h_next | None).  ``halo`` / ``split`` (sharding.Halo / SplitGraph): the layer
        refreshes the ghost rows of ``h`` itself -- in place -- and overlaps the transfer with the interior edges; a call
        that needs a gradient refreshes out of place through ``halo.refresh`` (differentiable, blocking) instead.

        ``w`` [E] (``ops.cutoff_envelope``): the messages are summed with these edge weights, a_i = sum_e w_e m_e
        (``ops.segment_sum(weight=)``).  The one-launch message kernel and the scatter epilogue of message TP #2 sum with
        weight 1 and are not used; fp32 only.  Sharded (``halo`` / ``split``): ``g`` is ``split.graph`` and the refresh is
        the blocking one (``halo.exchange``, or ``halo.refresh`` with a gradient) -- the interior / boundary overlap is the
        one-launch kernel's and is not available with an envelope; ``halo`` and ``split`` come together there."""
        if w is not None:
            if (halo is None) != (split is None):
                raise NotImplementedError(_ENVELOPE_NEEDS_BOTH)
            if h.dtype != torch.float32:
                raise RuntimeError("the cutoff envelope is fp32: bf16 storage has no weighted aggregation")
        if (halo is not None or split is not None) and g.periodic:
            raise NotImplementedError(_PERIODIC_NOT_SHARDED)
        needs_grad = torch.is_grad_enabled() and _needs_grad(self, h)
        if needs_grad and self.fused and not SEGNNLayer._warned_unfused:
            # the switch is visible: the fused MFMA kernels are inference kernels (no backward); a call that needs a gradient
            # runs the differentiable chain (gather -> TP -> gate -> TP -> gate -> segment-sum on the generic FMA kernels,
            # [E, width] tensors in HBM), which is several times slower -- tools/train_step_bench.py measures both
            SEGNNLayer._warned_unfused = True
            import warnings
            warnings.warn("SEGNNLayer: a gradient is required (grad mode on and an input or parameter requires grad) -> the "
                          "unfused differentiable chain runs instead of the fused MFMA inference kernels; wrap inference in "
                          "torch.no_grad() to get the fast path", RuntimeWarning, stacklevel=2)
        message, update = self.paths(h.dtype, needs_grad, w is not None)
        overlap = message == "one_launch" and halo is not None and split is not None
        if halo is not None and needs_grad:
            h = halo.refresh(h)  # differentiable refresh, out of place: ghost-row gradients return to their owners
        elif halo is not None and not overlap:
            halo.exchange(h)  # blocking refresh of the ghost rows, in place
        # ---- message function -> aggregated messages a [N, width] ----
        a_scale = None  # operand scale of the aggregated messages where the message launch returns it
        if overlap:
            a = self._messages_overlapped(h, h_scale, halo, split)
        elif message == "one_launch":
            a, a_scale, h_scale = self._messages_one_launch(h, g, h_scale)
        elif message == "per_product":
            a = self._messages_per_product(h, g, Y, d, w)
        else:
            a = self._messages_chain(h, g, Y, d, w)
        # ---- node update ----
        if update == "fused":
            # operand scale of [h | a]: h's is known (the previous layer returned it), so only `a` is scanned
            # (the one-launch message kernel returns the scale of its sums: no scan)
            sc = None
            if h.dtype == torch.float32 and h_scale is not None and halo is None:
                sc = ops.join_pow2_scales(h_scale, a_scale if a_scale is not None else ops.pow2_scale([a]))
            return self._update_fused(h, a, A, sc)
        u = self.upd2(self._gate(self.upd1(torch.cat([h, a], 1), A)), A)
        if h.dtype == torch.float32 and not needs_grad:
            return ops.add_pow2_scale(h, u)
        return h + u, None

    def _messages_one_launch(self, h, g, h_scale):
        """SH + TP #1 + gate + TP #2 + gate + segment-sum in one launch (message.FusedMessage) -> (a, operand scale of a
        | None, operand scale of h)."""
        if h_scale is None and h.dtype == torch.float32:
            h_scale = ops.pow2_scale([h])
        a, a_scale = self._msg.forward(h, g, self.msg1, self.msg2, h_scale, return_scale=True)
        return a.to(h.dtype), a_scale, h_scale

    def _messages_overlapped(self, h, h_scale, halo, split):
        """The one-launch kernel around the halo refresh (``halo.start`` / ``halo.finish``), in place."""
        # the refresh is posted first; interior edges (owned src) run while it is in flight, boundary edges after it
        # landed.  The operand scale has to be fixed BEFORE the refreshed ghost rows are known (the pre-mix table and
        # the interior launch use it): it is taken from the owned + stale ghost rows with NINE binades of head room
        # (joint maximum at 2^6 instead of 2^10) -- the fp16 (hi, lo) pair keeps an absolute error of 2^-25 of the scaled
        # range, so the lower target costs no accuracy, and refreshed rows up to 512 x larger than anything this rank
        # held stay inside the fp16 range.  Beyond that the overflow flag of the halo is raised (checked once per forward).
        f32 = h.dtype == torch.float32
        tok = halo.start(h)
        if h_scale is None and f32:
            h_scale = ops.pow2_scale([h], target_log2=6)
        a, state = self._msg.forward(h, split.graph, self.msg1, self.msg2, h_scale, edges=split.interior,
                                     return_state=True)
        halo.finish(h, tok)
        if state is not None:
            # the pre-mix launch saw the STALE ghost rows: their row maxima (bound of a row's messages) are recomputed
            top = self._msg.refresh_row_max(state, h, halo.ghost_rows(), h_scale if f32 else None)
            if f32:
                flag = top >= 2.0 ** 15
                halo.overflow = flag if getattr(halo, "overflow", None) is None else (halo.overflow | flag)
        return self._msg.forward(h, split.graph, self.msg1, self.msg2, h_scale, edges=split.boundary, cont=state).to(h.dtype)

    def _messages_per_product(self, h, g, Y, d, w):
        # gather + concat + TP + gate in one kernel each: no [E, 2D+1] / raw-TP tensors in HBM
        if d.dtype != h.dtype:
            d = d.to(h.dtype)
        m = self.msg1.forward_fused([(h, g.dst), (h, g.src), (d, None)], Y, gate=True,
                                    in_scale=ops.pow2_scale([h, d]) if h.dtype == torch.float32 else None)
        a = None
        if self.fuse_scatter and w is None:  # segment-sum in the epilogue of message TP #2 where the library has that kernel
            a = self.msg2.forward_fused([(m, None)], Y, gate=True, scatter=(g.dst, g.rowptr.numel() - 1))
        if a is None:
            m = self.msg2.forward_fused([(m, None)], Y, gate=True)
            a = ops.segment_sum(m, g, weight=w)
        return a

    def _messages_chain(self, h, g, Y, d, w):
        m = ops.gather_concat(h, g, d)
        m = self._gate(self.msg1(m, Y))
        m = self._gate(self.msg2(m, Y))
        return ops.segment_sum(m, g, weight=w)

    def _update_fused(self, h, a, A, sc):
        """h + TP_u2(gate(TP_u1([h | a]))) on the fused kernels, with what the library has for the shape: both products
        in one launch, else two fused launches, else fused #1 + the module's #2.  ``sc``: operand scale of [h | a]."""
        f32 = h.dtype == torch.float32
        if self.upd2.fused_supported(False) and h.stride(-1) == 1:
            if isinstance(self.upd1, SHTensorProduct) and a.stride(-1) == 1:
                # both products in one launch: u stays on chip with a power-of-two scale per row
                r = self.upd1.forward_update_pair(self.upd2, [(h, None), (a, None)], A, in_scale=sc, residual=h,
                                                  out_scale=10 if f32 else None)
                if r is not None:
                    return r if f32 else (r, None)
            # the scale of u comes out of update #1's epilogue; update #2 adds the residual and emits the scale of the
            # new h in its own: no pass over [N, width] outside the two products
            if f32:
                u, u_scale = self.upd1.forward_fused([(h, None), (a, None)], A, gate=True, in_scale=sc, out_scale=10)
                return self.upd2.forward_fused([(u, None)], A, gate=False, in_scale=u_scale, residual=h, out_scale=10)
            u = self.upd1.forward_fused([(h, None), (a, None)], A, gate=True)
            return self.upd2.forward_fused([(u, None)], A, gate=False, residual=h), None
        u = self.upd2(self.upd1.forward_fused([(h, None), (a, None)], A, gate=True, in_scale=sc), A)
        return ops.add_pow2_scale(h, u) if f32 else (h + u, None)


def _needs_grad(mod: nn.Module, *tensors) -> bool:
    return any(t.requires_grad for t in tensors) or any(p.requires_grad for p in mod.parameters())


class SEGNN(nn.Module):
    def __init__(self, in_irreps="1x0e+1x1o", hidden: int = 32, out_irreps="1x1o", num_layers: int = 4, lmax: int = 1,
                 envelope: int | None = None):
        """``envelope``: the exponent p of the polynomial cutoff envelope (``ops.cutoff_envelope``; 6 is the usual choice),
        None = no envelope.  With it every message is weighted by u_p(d / cutoff) in the aggregation and the node attribute
        is the enveloped one (``ops.enveloped_node_attr``), so the output is a smooth function of the positions across the
        cutoff; ``forward`` then needs ``cutoff=``.  It adds no parameter and no buffer."""
        super().__init__()
        assert lmax in (1, 2)
        self.hidden, self.lmax = hidden, lmax
        self.envelope = None if envelope is None else ops._envelope_args(1.0, envelope)[1]
        hid, _ = _hidden_irreps(hidden, lmax)
        self.in_irreps, self.out_irreps = Irreps(in_irreps), Irreps(out_irreps)
        self.embed = _make_tp(self.in_irreps, hid, lmax)
        self.layers = nn.ModuleList([SEGNNLayer(hidden, lmax) for _ in range(num_layers)])
        self.readout = _make_tp(hid, self.out_irreps, lmax)

    def forward(self, x: torch.Tensor, g: RadiusGraph, geometry=None, halo=None, split=None,
                cutoff: float | None = None) -> torch.Tensor:
        """x [N, in_dim] node features in the graph's (Morton) order -> [N, out_dim] in the same order.

        ``cutoff``: the envelope's radius r_c of a model built with ``envelope=`` (required then, a ValueError without
        one).  The graph may be built at a larger radius (a skin): an edge with d >= cutoff contributes exactly zero.

        ``halo`` (a ``sharding.Halo``): when the cloud is spatially sharded, ghost rows of ``h`` are
        refreshed from their owners before every message-passing layer; only owned rows of the result
        are meaningful.  ``split`` (``halo.split_graph(g)``): edges into ghost rows dropped and the rest split into
        interior / boundary lists so that the refresh overlaps the interior edges."""
        if (halo is not None or split is not None) and g.periodic:
            raise NotImplementedError(_PERIODIC_NOT_SHARDED)
        if (cutoff is None) != (self.envelope is None):
            raise ValueError("cutoff= is the radius of the envelope: a model built with envelope= needs it, and a model "
                             "without an envelope takes none")
        if self.envelope is not None:
            return self._forward_enveloped(x, g, geometry, halo, split, cutoff)
        if x.dtype == torch.bfloat16 and self.lmax != 2:
            raise RuntimeError("bf16 storage is implemented for l_max = 2 (BASELINE config 3)")
        # a differentiable geometry needs the chain also when no parameter does (forces / Hessian of a frozen model)
        needs_grad = torch.is_grad_enabled() and _needs_grad(self, x, *(t for t in geometry or () if t is not None))
        if split is not None:
            g = split.graph
        if geometry is not None:
            Y, d, A = geometry
        else:
            Y, d, A = ops.edge_geometry(g, lmax=self.lmax, want_edge=self.wants_edge_geometry(x.dtype, needs_grad))
        sc = None
        if (x.dtype == torch.float32 and not needs_grad and x.is_cuda and
                getattr(self.embed, "exact", None) is False and A.shape[0] == x.shape[0] and x.shape[0] > 0 and
                self.embed.fused_supported(False)):
            # inference, fp32, a shape of the fused kernel: the embedding's epilogue emits the operand scale of h, so that
            # layer 0 runs no scan over h
            h, sc = self.embed.forward_fused([(x, None)], A, gate=False, out_scale=10)
        else:
            h = self.embed(x, A)
        if halo is not None:
            halo.overflow = None
        for layer in self.layers:
            if halo is not None:
                sc = None  # the ghost rows are about to change: the scale of the previous layer's output is stale
            h, sc = layer(h, g, Y, d, A, sc, halo=halo, split=split)
        out = self.readout(h, A)
        if halo is not None and getattr(halo, "overflow", None) is not None and bool(halo.overflow):
            raise RuntimeError("sharded forward: a refreshed ghost row is more than 512 x larger than every row this rank held "
                               "when the layer's operand scale was fixed (fp16-split operands would overflow); run the layer "
                               "without `split` (blocking exchange) for such inputs")
        return out

    def wants_edge_geometry(self, dtype, needs_grad: bool) -> bool:
        """Per-edge Y [E, (l_max+1)^2] and d [E] are only needed off the one-launch message path (no envelope)."""
        return any(l.paths(dtype, needs_grad)[0] != "one_launch" for l in self.layers)

    def _forward_enveloped(self, x, g, geometry, halo, split, cutoff):
        """The forward with the cutoff envelope: w = u_p(d / cutoff) once from the edge lengths, the enveloped node
        attribute in place of the mean, and w on every layer's aggregation.  Sharded: the graph is ``split.graph`` (the
        edges into ghost rows removed) and every layer refreshes the ghost rows before its messages, blocking: the
        overlap of the refresh with the interior edges needs the one-launch message kernel, which has no envelope.
        ``halo`` and ``split`` come together: the weights and the enveloped node attribute are those of ``split.graph``,
        and without the refresh of ``halo`` its ghost rows would be stale."""
        if (halo is None) != (split is None):
            raise NotImplementedError(_ENVELOPE_NEEDS_BOTH)
        if x.dtype != torch.float32:
            raise RuntimeError("the cutoff envelope is fp32: bf16 storage has no weighted aggregation")
        if split is not None:
            g = split.graph
        if geometry is not None:
            Y, d, _ = geometry
        else:
            Y, d, _ = ops.edge_geometry(g, lmax=self.lmax, want_node_attr=False, want_edge=True)
        w = ops.cutoff_envelope(d, cutoff, self.envelope)
        # sharded: a ghost row has no incoming edge in split.graph, so its A is that of an isolated node; it only enters
        # the ghost row's own update, whose result the next refresh overwrites and no owned result reads
        A = ops.enveloped_node_attr(Y, w, g)
        h = self.embed(x, A)
        sc = None
        for layer in self.layers:
            if halo is not None:
                sc = None  # the ghost rows are about to change: the scale of the previous layer's output is stale
            h, sc = layer(h, g, Y, d, A, sc, halo=halo, split=split, w=w)
        return self.readout(h, A)

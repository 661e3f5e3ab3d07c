"""The packed-weight cache (``_lib.PackedCache``) through its three owners at their smallest shapes -- ``L1TensorProduct``,
``SHTensorProduct`` (``TPPlan``) and ``FusedMessage`` -- and copies of modules that have already run.

The message owner runs on graph "B" of tests/msg_cases.py (12 edges: less than one tile, so every row of the sums receives
a single contribution and two launches agree bit for bit although the hidden-16 kernel sums by atomics).
tests/test_msg_table_gpu.py::test_packed_weights_follow_the_tensors checks the same cache against the fp64 oracle."""
import copy
import pickle

import pytest
import torch

import msg_cases as C
import r16_cases as R
from scalable_e3_gnn_amd import ops
from scalable_e3_gnn_amd.l1_tensor_prod import L1TensorProduct
from scalable_e3_gnn_amd.tensor_product import SHTensorProduct

pytestmark = pytest.mark.gpu
DEV = torch.device(C.DEV)
F32 = torch.float32


class _Product:
    """one tensor product with a fixed input"""

    def __init__(self, cls, irreps, B, **kw):
        torch.manual_seed(7)
        self.root = cls(irreps, irreps, **kw).to(DEV)
        gen = torch.Generator().manual_seed(8)
        self.x = torch.randn(B, self.root.in1_dim, generator=gen).to(DEV)
        self.y = torch.randn(B, self.root.in2_dim, generator=gen).to(DEV)
        self.weight, self.norm = self.root.weights_l0e, self.root.norm_l0e

    def packed(self):
        with torch.cuda.device(DEV):
            return self.root._packed_weights(F32, DEV)

    def forward(self):
        with torch.no_grad():
            return self.root(self.x, self.y)


class _Message:
    """FusedMessage(1, 16) with the two message products of a SEGNNLayer"""

    def __init__(self):
        self.root = C.make_layer(1, 16, "fp32")
        self.weight, self.norm = self.root.msg2.weights_l1o, self.root.msg1.norm_l0e

    def packed(self):
        return self.root._msg.packed(self.root.msg1, self.root.msg2, DEV, dtype=F32)

    def forward(self):
        with torch.no_grad():
            return self.root._msg.forward(C.features(1, 16, "fp32"), C.graph("B", "open"), self.root.msg1, self.root.msg2)


OWNERS = {"l1tp": lambda: _Product(L1TensorProduct, "4x0e+4x1o", 8),
          "shtp": lambda: _Product(SHTensorProduct, "16x0e+16x1o+16x2e", 16, lmax_sh=2),
          "msg": _Message}


@pytest.mark.parametrize("owner", list(OWNERS))
def test_cache_follows_the_tensors_and_the_streams(owner):
    o = OWNERS[owner]()
    out = o.forward()
    buf = o.packed()
    assert o.packed() is buf, "an unchanged second call repacks"
    assert torch.equal(o.forward(), out) and o.packed() is buf
    for what in ("weight", "norm"):
        with torch.no_grad():
            getattr(o, what).mul_(1.5)
        new = o.packed()
        assert new is not buf, f"{what}.mul_ did not reach the packed image"
        changed = o.forward()
        assert not torch.equal(changed, out), what
        buf, out = new, changed
    # packed on a side stream, used on the default stream: the forward waits for the pack and computes what a module
    # that packs on the default stream computes
    want = OWNERS[owner]().forward()
    p = OWNERS[owner]()
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()   # the module's tensors were written on the default stream
    with torch.cuda.stream(side):
        buf = p.packed()
    got = p.forward()
    assert p.packed() is buf, "the forward did not use the image packed on the side stream"
    assert torch.equal(got, want)
    torch.cuda.synchronize()


def _layer_case():
    layer = C.make_layer(1, 16, "fp32")
    g = C.graph("B", "open")
    Y, d, A = ops.edge_geometry(g, lmax=1)
    h = C.features(1, 16, "fp32")

    def forward(m):
        with torch.no_grad():
            return m(h, g, Y, d, A)[0]

    def buffers(m):
        bufs = [m._msg.packed(m.msg1, m.msg2, DEV)]
        for tp in (m.upd1, m.upd2):
            plan, ws, ns = R.plan_of(tp)
            bufs.append(plan.packed(ws, ns, F32, DEV))
        return bufs
    return layer, forward, buffers


def _product_case(owner):
    o = OWNERS[owner]()

    def forward(m):
        with torch.no_grad():
            return m(o.x, o.y)
    return o.root, forward, lambda m: [m._packed_weights(F32, DEV)]


COPIES = {"l1tp": lambda: _product_case("l1tp"), "shtp": lambda: _product_case("shtp"), "layer": _layer_case}


@pytest.mark.parametrize("how", ["deepcopy", "pickle"])
@pytest.mark.parametrize("module", list(COPIES))
def test_copy_after_use(module, how):
    """A module that has run copies and pickles (EMA copies, torch.save of a whole module): the copy computes the same
    bits and packs its own weights."""
    mod, forward, buffers = COPIES[module]()
    out = forward(mod)
    dup = copy.deepcopy(mod) if how == "deepcopy" else pickle.loads(pickle.dumps(mod))
    assert torch.equal(forward(dup), out)
    with torch.cuda.device(DEV):
        mine, theirs = buffers(mod), buffers(dup)
    assert not {b.data_ptr() for b in mine} & {b.data_ptr() for b in theirs}
    assert torch.equal(forward(mod), out)

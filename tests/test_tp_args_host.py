"""Status codes of the argument checks of the general tensor product's C entries (include/e3gnn.h), on the host alone.

Every case has exactly one fault and is rejected (or, with B = 0, accepted) before the first HIP call, so the pointers are fake
non-null values and nothing here needs a GPU.  No case would pass the checks: such a call would reach the device with those
pointers.  ``out_scale4`` stays NULL except where the fault is its ``target_log2``: the entries zero it on the stream before
some of their later checks.  Plans come from ``e3_tp_plan_create``, which is host only.

EXPECTED is what the library returned for these cases BEFORE e3_tp.hip was split by role (recorded from a build of that
commit): the first failing check decides the status, so the table pins the order of the checks inside each entry."""
import ctypes
from ctypes import c_int, c_int64, c_void_p

import pytest

import bwd_cases as C
from r16_cases import GATED
from scalable_e3_gnn_amd import _lib
from scalable_e3_gnn_amd.irreps import as_blocks
from scalable_e3_gnn_amd.tensor_product import TPSegment

F32, F64, BF16 = _lib.E3_F32, _lib.E3_F64, _lib.E3_BF16
P, I, L = c_void_p, c_int, c_int64

ROWS = [("plan", P), ("in1", P), ("ld1", L), ("in2", P), ("ld2", L)]
FUSED = [("plan", P), ("segs", P), ("nseg", I), ("in2", P), ("ld2", L), ("packed", P)]
SCALE = [("out_scale4", P), ("target_log2", I)]
PARAMS = {
    "e3_tp_forward": ROWS + [("packed", P), ("out", P), ("ldo", L), ("B", L), ("dtype", I), ("in_scale", P), ("exact", I)],
    "e3_tp_forward_fused": FUSED + [("out", P), ("ldo", L), ("B", L), ("dtype", I), ("gate", I), ("in_scale", P)],
    "e3_tp_forward_fused_epilogue": FUSED + [("out", P), ("ldo", L), ("B", L), ("dtype", I), ("gate", I), ("in_scale", P),
                                             ("residual", P), ("ld_residual", L)] + SCALE,
    "e3_tp_forward_update_pair": [("plan", P), ("plan2", P), ("segs", P), ("nseg", I), ("in2", P), ("ld2", L), ("packed", P),
                                  ("packed2", P), ("in_scale", P), ("residual", P), ("ld_residual", L), ("out", P),
                                  ("ldo", L), ("B", L), ("dtype", I)] + SCALE,
    "e3_tp_forward_fused_scatter": FUSED + [("row_node", P), ("out", P), ("ldo", L), ("B", L), ("dtype", I), ("gate", I),
                                            ("in_scale", P)],
    "e3_tp_backward": ROWS + [("packed", P), ("grad_out", P), ("ldg", L), ("grad_in1", P), ("ldg1", L), ("grad_in2", P),
                              ("ldg2", L), ("grad_weights", P), ("B", L), ("dtype", I)],
    "e3_tp_backward_operands": ROWS + [("packed", P), ("grad_out", P), ("ldg", L), ("features", P), ("gout", P), ("B", L),
                                       ("dtype", I)],
    "e3_tp_backward_contract": ROWS + [("t", P), ("grad_in1", P), ("ldg1", L), ("grad_in2", P), ("ldg2", L), ("B", L),
                                       ("dtype", I)],
    "e3_tp_backward_weights": ROWS + [("packed", P), ("grad_out", P), ("ldg", L), ("grad_weights", P), ("B", L), ("dtype", I)],
    "e3_tp_pack_weights": [("plan", P), ("w", P), ("n", P), ("dtype", I), ("packed", P)],
}
FUSED_ENTRIES = [e for e in PARAMS if "fused" in e or "pair" in e]

# (in1 irreps, out irreps, lmax_sh): the gated node update #1 and update #2 of hidden 32 at l_max 2 (together the fused pair)
# and at l_max 1, and a product with a 1e input, which the MFMA path does not take
assert "upd1" in GATED
PLANS = {"l2": C.product_irreps("upd1", 32, 2) + (2,), "l2b": C.product_irreps("upd2", 32, 2) + (2,),
         "l1": C.product_irreps("upd1", 32, 1) + (1,), "odd": ("4x0e+4x1e", "4x0e+4x1e", 1)}


@pytest.fixture(scope="module")
def lib():
    _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)  # own prototypes: the six-pointer arrays and the segments go in as void*
    for e, ps in PARAMS.items():
        fn = getattr(raw, e)
        fn.restype, fn.argtypes = c_int, [t for _, t in ps] + [c_void_p]  # ... and the stream
    for e in ("e3_tp_in1_dim", "e3_tp_in2_dim", "e3_tp_out_dim", "e3_tp_plan_destroy"):
        getattr(raw, e).restype, getattr(raw, e).argtypes = c_int, [c_void_p]
    raw.e3_tp_weight_shape.restype, raw.e3_tp_weight_shape.argtypes = c_int, [c_void_p, c_int, c_void_p, c_void_p]
    raw.e3_tp_norm_len.restype, raw.e3_tp_norm_len.argtypes = c_int, [c_void_p, c_int]
    raw.e3_tp_packed_bytes.restype, raw.e3_tp_packed_bytes.argtypes = c_int64, [c_void_p, c_int]
    raw.e3_tp_fused_supported.restype, raw.e3_tp_fused_supported.argtypes = c_int, [c_void_p, c_int]
    return raw


@pytest.fixture(scope="module")
def plans(lib):
    made = {}
    for key, (i, o, lmax_sh) in PLANS.items():
        (bi, ni), (bo, no) = _lib.blocks_array(as_blocks(i)), _lib.blocks_array(as_blocks(o))
        p = c_void_p()
        assert lib.e3_tp_plan_create(bi, ni, lmax_sh, bo, no, ctypes.byref(p)) == 0
        made[key] = p
    assert lib.e3_tp_fused_supported(made["l2"], 1) == 1 and lib.e3_tp_fused_supported(made["l1"], 1) == 1
    assert lib.e3_tp_fused_supported(made["odd"], 0) == 0
    yield made
    for p in made.values():
        assert lib.e3_tp_plan_destroy(p) == 0


SIX = (c_void_p * 6)(*[0xA0000 + 0x1000 * c for c in range(6)])      # fake per-class pointers, every class present
SIX_GAP = (c_void_p * 6)(None, *[0xA1000 + 0x1000 * c for c in range(5)])  # class 0e missing
SEGS = (TPSegment * 2)(TPSegment(0x10000, 1024, None, 288, 0), TPSegment(0x18000, 1024, None, 288, 0))


def addr(a):
    return ctypes.cast(a, c_void_p).value


def call(lib, plans, entry, plan, fault):
    """The entry with operands that would pass every check of `plan`, except for `fault` (ld*: an offset to the width)."""
    h = plans[plan]
    D1, Dy, Dout = lib.e3_tp_in1_dim(h), lib.e3_tp_in2_dim(h), lib.e3_tp_out_dim(h)
    h2 = plans["l2b"]
    a = dict(plan=h, plan2=h2, in1=0x10000, ld1=D1, in2=0x20000, ld2=Dy, packed=0x30000, packed2=0x38000, out=0x40000,
             ldo=lib.e3_tp_out_dim(h2) if "pair" in entry else Dout, B=33, dtype=F32, in_scale=None, exact=0, segs=addr(SEGS),
             nseg=2, gate=1, residual=None, ld_residual=0, out_scale4=None, target_log2=0, row_node=0x50000, grad_out=0x60000,
             ldg=Dout, grad_in1=0x70000, ldg1=D1, grad_in2=0x80000, ldg2=Dy, grad_weights=addr(SIX), features=addr(SIX),
             gout=addr(SIX), t=addr(SIX), w=addr(SIX), n=None)
    for k, v in fault.items():
        if k.startswith("ld") and k != "ld_residual" and isinstance(v, str):  # "-1": one below the width; "0": broadcast
            v = a[k] + int(v) if v != "0" else 0
        a[k] = plans[v] if k in ("plan", "plan2") and v is not None else v
    return getattr(lib, entry)(*[a[name] for name, _ in PARAMS[entry]], None)




OK, INVALID_ARG, MISSING_WEIGHT, UNSUPPORTED = 0, 1, 3, 4


def build_cases():
    """[(id, entry, plan, fault, status)] -- the status is the one recorded before the split (module docstring)"""
    cases = []

    def add(entry, plan, name, status, /, **fault):
        cases.append((f"{entry[6:]}-{plan}-{name}", entry, plan, fault, status))

    for plan in ("l2", "l1", "odd"):
        e = "e3_tp_forward"
        add(e, plan, "null_plan", INVALID_ARG, plan=None)
        add(e, plan, "negative_B", INVALID_ARG, B=-1)
        add(e, plan, "dtype_-1", INVALID_ARG, dtype=-1)
        add(e, plan, "dtype_3", INVALID_ARG, dtype=3)
        add(e, plan, "B0_null_in1_ok", OK, B=0, in1=None)
        for ptr in ("in1", "in2", "packed", "out"):
            add(e, plan, "null_" + ptr, INVALID_ARG, **{ptr: None})
        if plan != "odd":
            add(e, plan, "bf16_broadcast_in2", UNSUPPORTED, dtype=BF16, ld2="0")
        for ld in ("ld1", "ld2", "ldo"):
            add(e, plan, ld + "_below", INVALID_ARG, **{ld: "-1"})
        add(e, plan, "f64_ld1_below", INVALID_ARG, dtype=F64, ld1="-1")
        for e in ("e3_tp_backward", "e3_tp_backward_operands", "e3_tp_backward_contract", "e3_tp_backward_weights"):
            bad_dtype = UNSUPPORTED if e == "e3_tp_backward_weights" else INVALID_ARG
            add(e, plan, "null_plan", INVALID_ARG, plan=None)
            add(e, plan, "negative_B", INVALID_ARG, B=-1)
            add(e, plan, "dtype_bf16", bad_dtype, dtype=BF16)
            add(e, plan, "dtype_3", bad_dtype, dtype=3)
            add(e, plan, "B0_null_in1_ok", OK, B=0, in1=None)
            for ptr in [n for n, _ in PARAMS[e] if n in ("in1", "in2", "packed", "grad_out", "t")]:
                add(e, plan, "null_" + ptr, INVALID_ARG, **{ptr: None})
            for ld in [n for n, _ in PARAMS[e] if n in ("ld1", "ld2", "ldg")]:
                add(e, plan, ld + "_below", INVALID_ARG, **{ld: "-1"})
            if e in ("e3_tp_backward", "e3_tp_backward_contract"):
                add(e, plan, "ldg1_below", INVALID_ARG, ldg1="-1")
                add(e, plan, "ldg2_below", INVALID_ARG, ldg2="-1")
                add(e, plan, "broadcast_in2_full_grad", INVALID_ARG, ld2="0")   # the broadcast-in2 rule:
                add(e, plan, "full_in2_broadcast_grad", INVALID_ARG, ldg2="0")  # (ld2 == 0) != (ldg2 == 0)
        add("e3_tp_backward_contract", plan, "no_grad_wanted", INVALID_ARG, grad_in1=None, grad_in2=None)
        add("e3_tp_backward_operands", plan, "nothing_wanted", INVALID_ARG, features=None, gout=None)
        add("e3_tp_backward_operands", plan, "gout_without_grad_out", INVALID_ARG, features=None, grad_out=None)
        add("e3_tp_backward_weights", plan, "null_grad_weights", INVALID_ARG, grad_weights=None)
        add("e3_tp_backward_weights", plan, "dtype_f64", UNSUPPORTED, dtype=F64)
        e = "e3_tp_pack_weights"
        add(e, plan, "null_plan", INVALID_ARG, plan=None)
        add(e, plan, "null_w", INVALID_ARG, w=None)
        add(e, plan, "null_packed", INVALID_ARG, packed=None)
        add(e, plan, "dtype_-1", INVALID_ARG, dtype=-1)
        add(e, plan, "dtype_3", INVALID_ARG, dtype=3)
        add(e, plan, "missing_weight", MISSING_WEIGHT, w=addr(SIX_GAP))
    add("e3_tp_forward", "odd", "bf16_without_mfma", UNSUPPORTED, dtype=BF16)
    for plan in ("l2", "l1"):
        for e in FUSED_ENTRIES:
            pair = "pair" in e
            if pair and plan != "l2":
                continue
            add(e, plan, "null_plan", INVALID_ARG, plan=None)
            add(e, plan, "null_segs", INVALID_ARG, segs=None)
            add(e, plan, "negative_B", INVALID_ARG, B=-1)
            add(e, plan, "dtype_f64", UNSUPPORTED, dtype=F64)
            add(e, plan, "dtype_3", UNSUPPORTED, dtype=3)
            add(e, plan, "broadcast_in2", UNSUPPORTED, ld2="0")
            add(e, plan, "ld2_below", INVALID_ARG, ld2="-1")
            for ptr in ("in2", "packed", "out"):
                add(e, plan, "null_" + ptr, INVALID_ARG, **{ptr: None})
            if not pair:
                add(e, plan, "B0_null_in2_ok", OK, B=0, in2=None)
                if plan == "l2":
                    add(e, "odd", "without_mfma", UNSUPPORTED)
            if "scatter" in e:
                add(e, plan, "null_row_node", INVALID_ARG, row_node=None)
                add(e, plan, "no_gate", UNSUPPORTED, gate=0)
            if pair or "epilogue" in e:
                add(e, plan, "residual_without_ld", INVALID_ARG, residual=0x90000)
                add(e, plan, "residual_negative_ld", INVALID_ARG, residual=0x90000, ld_residual=-4)
                add(e, plan, "target_log2_-21", INVALID_ARG, out_scale4=0x98000, target_log2=-21)
                add(e, plan, "target_log2_15", INVALID_ARG, out_scale4=0x98000, target_log2=15)
    e = "e3_tp_forward_update_pair"
    add(e, "l2", "null_plan2", INVALID_ARG, plan2=None)
    add(e, "l2", "null_packed2", INVALID_ARG, packed2=None)
    add(e, "l2", "ldo_below_plan2", INVALID_ARG, ldo="-1")
    add(e, "l2", "plan2_not_the_pair", UNSUPPORTED, plan2="odd")
    add(e, "l1", "no_pair_at_lmax_1", UNSUPPORTED, plan2="l1")
    return cases


CASES = build_cases()


def test_cases_are_distinct_and_cover_every_entry():
    ids = [c[0] for c in CASES]
    assert len(set(ids)) == len(ids) == 337
    assert {c[1] for c in CASES} == set(PARAMS)


@pytest.mark.parametrize("name,entry,plan,fault,status", CASES, ids=[c[0] for c in CASES])
def test_one_fault(lib, plans, name, entry, plan, fault, status):
    assert call(lib, plans, entry, plan, fault) == status


def test_queries_with_bad_arguments(lib, plans):
    r, c = c_int(), c_int()
    rp, cp = addr(ctypes.pointer(r)), addr(ctypes.pointer(c))
    h = plans["l2"]
    assert [lib.e3_tp_weight_shape(None, 0, rp, cp), lib.e3_tp_weight_shape(h, -1, rp, cp),
            lib.e3_tp_weight_shape(h, 6, rp, cp), lib.e3_tp_weight_shape(h, 0, None, cp),
            lib.e3_tp_weight_shape(h, 0, rp, None)] == [INVALID_ARG] * 5
    assert [lib.e3_tp_norm_len(None, 0), lib.e3_tp_norm_len(h, -1), lib.e3_tp_norm_len(h, 6)] == [-1, -1, -1]
    assert [lib.e3_tp_packed_bytes(None, F32), lib.e3_tp_packed_bytes(h, -1), lib.e3_tp_packed_bytes(h, 3)] == [-1, -1, -1]

"""Status codes of the argument checks of the six ``e3_msg_forward*`` entries (include/e3gnn.h), on the host alone.

Every case has exactly one fault and is rejected before the first HIP call, so the pointers are fake non-null values
(16-byte aligned unless the case is about alignment) and nothing here needs a GPU.  No case is valid: a call that passed the
checks would reach the device with those pointers.  Plans come from ``e3_msg_plan_create``, which is host only."""
import ctypes
from ctypes import c_int, c_int64, c_void_p

import pytest

from scalable_e3_gnn_amd import _lib

OK, INVALID_ARG, UNSUPPORTED = 0, 1, 4
F32, BF16 = _lib.E3_F32, _lib.E3_BF16

ENTRIES = ("e3_msg_forward", "e3_msg_forward_pbc", "e3_msg_forward_cell",
           "e3_msg_forward_owned", "e3_msg_forward_owned_pbc", "e3_msg_forward_owned_cell")
OWNED = ENTRIES[3:]

COMMON = [("plan", c_void_p), ("h", c_void_p), ("ld_h", c_int64), ("N", c_int64), ("pos4", c_void_p), ("src", c_void_p),
          ("dst", c_void_p), ("E", c_int64), ("packed", c_void_p), ("in_scale", c_void_p), ("premix", c_void_p),
          ("out", c_void_p), ("ld_out", c_int64), ("dtype", c_int)]
SUMS = [("accumulate", c_int), ("tiles_per_block", c_int)]
OWNED_SUMS = [("tiles_per_block", c_int), ("workspace", c_void_p), ("workspace_bytes", c_int64), ("out_scale4", c_void_p),
              ("target_log2", c_int)]


def params(entry):
    """(name, ctype) of the entry's arguments, in order (the box / cell as void*: a case passes NULL there)."""
    p = COMMON + (OWNED_SUMS if "owned" in entry else SUMS)
    if entry.endswith("_pbc"):
        p = p + [("box", c_void_p)]
    if entry.endswith("_cell"):
        p = p + [("cell", c_void_p)]
    return p + [("stream", c_void_p)]


@pytest.fixture(scope="module")
def lib():
    _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)  # own prototypes: the binding's Float3 / Float9 do not take NULL
    for e in ENTRIES:
        fn = getattr(raw, e)
        fn.restype, fn.argtypes = c_int, [t for _, t in params(e)]
    raw.e3_msg_plan_create.restype, raw.e3_msg_plan_create.argtypes = c_int, [c_int, c_int, ctypes.POINTER(c_void_p)]
    raw.e3_msg_plan_destroy.restype, raw.e3_msg_plan_destroy.argtypes = c_int, [c_void_p]
    raw.e3_msg_owned_workspace_bytes.restype = c_int64
    raw.e3_msg_owned_workspace_bytes.argtypes = [c_void_p, c_int64, c_int, c_int]
    return raw


@pytest.fixture(scope="module")
def plans(lib):
    made = {}
    for lmax, hidden in ((2, 32), (1, 32), (2, 16), (1, 16)):
        p = c_void_p()
        assert lib.e3_msg_plan_create(lmax, hidden, ctypes.byref(p)) == OK
        made[(lmax, hidden)] = p
    yield made
    for p in made.values():
        assert lib.e3_msg_plan_destroy(p) == OK


BOX = (ctypes.c_float * 3)(4.0, 5.0, 0.0)
CELL = (ctypes.c_float * 9)(4.0, 0.0, 0.0, 1.0, 5.0, 0.0, 0.5, 0.25, 6.0)


def floats(*v):
    return (ctypes.c_float * len(v))(*v)


def call(lib, plans, entry, shape=(2, 32), **fault):
    """The entry with operands that would pass every check of plan `shape`, except for `fault`."""
    lmax, hidden = shape
    D = hidden * (lmax + 1) ** 2
    a = dict(plan=plans[shape], h=0x10000, ld_h=D, N=64, pos4=0x20000, src=0x30000, dst=0x40000, E=1000, packed=0x50000,
             in_scale=None, premix=0x60000, out=0x70000, ld_out=D, dtype=F32, accumulate=0, tiles_per_block=0,
             workspace=0x80000, workspace_bytes=None, out_scale4=0x90000, target_log2=0, box=BOX, cell=CELL, stream=None)
    a.update(fault)
    if a["workspace_bytes"] is None:  # what the entry asks for (or 0 where it does not get that far)
        a["workspace_bytes"] = max(0, lib.e3_msg_owned_workspace_bytes(a["plan"], a["E"], a["dtype"], a["tiles_per_block"]))
    return getattr(lib, entry)(*[a[name] for name, _ in params(entry)])


# one fault each, every entry: (id, overrides, status)
EVERY_ENTRY = [
    ("null_plan", dict(plan=None, workspace_bytes=1 << 20), INVALID_ARG),
    ("negative_N", dict(N=-1), INVALID_ARG),
    ("negative_E", dict(E=-1), INVALID_ARG),
    ("E_above_2^31-17", dict(E=2**31 - 16), INVALID_ARG),
    ("null_h", dict(h=None), INVALID_ARG),
    ("null_pos4", dict(pos4=None), INVALID_ARG),
    ("null_packed", dict(packed=None), INVALID_ARG),
    ("null_premix", dict(premix=None), INVALID_ARG),
    ("null_out", dict(out=None), INVALID_ARG),
    ("ld_h_below_D", dict(ld_h=-1), INVALID_ARG),      # -1: D - 1 of the case's plan (below)
    ("ld_out_below_D", dict(ld_out=-1), INVALID_ARG),
    ("null_src", dict(src=None), INVALID_ARG),
    ("h_4_mod_16", dict(h=0x10004), INVALID_ARG),
    ("premix_4_mod_16", dict(premix=0x60004), INVALID_ARG),
    ("fp32_rows_not_16_bytes", dict(ld_h=+1), INVALID_ARG),  # +1: D + 1
]


def resolve(fault, shape):
    D = shape[1] * (shape[0] + 1) ** 2
    return {k: (D + v if k in ("ld_h", "ld_out") else v) for k, v in fault.items()}


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name,fault,status", EVERY_ENTRY, ids=[c[0] for c in EVERY_ENTRY])
def test_one_fault_every_entry(lib, plans, entry, name, fault, status):
    assert call(lib, plans, entry, **resolve(fault, (2, 32))) == status
    if "owned" not in entry:  # a plan of the one-wave-per-tile kernel too (the owned entries do not take it)
        assert call(lib, plans, entry, shape=(1, 16), **resolve(fault, (1, 16))) == status


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("shape", [(2, 16), (1, 16)])
def test_bf16_on_hidden_16(lib, plans, entry, shape):
    assert call(lib, plans, entry, shape=shape, dtype=BF16) == UNSUPPORTED


@pytest.mark.parametrize("entry", OWNED)
def test_owned_entries(lib, plans, entry):
    assert call(lib, plans, entry, out_scale4=None) == INVALID_ARG
    assert call(lib, plans, entry, target_log2=-21) == INVALID_ARG
    assert call(lib, plans, entry, target_log2=15) == INVALID_ARG
    # shapes of the one-wave-per-tile kernel have no owned sums
    assert call(lib, plans, entry, shape=(1, 32)) == UNSUPPORTED
    assert call(lib, plans, entry, shape=(2, 16)) == UNSUPPORTED
    need = lib.e3_msg_owned_workspace_bytes(plans[(2, 32)], 1000, F32, 0)
    assert need > 0
    assert call(lib, plans, entry, workspace=None) == INVALID_ARG
    assert call(lib, plans, entry, workspace_bytes=need - 1) == INVALID_ARG
    assert call(lib, plans, entry, workspace=0x80008) == INVALID_ARG


@pytest.mark.parametrize("entry", [e for e in ENTRIES if e.endswith("_pbc")])
def test_bad_box(lib, plans, entry):
    assert call(lib, plans, entry, box=None) == INVALID_ARG
    assert call(lib, plans, entry, box=floats(4.0, -1.0, 5.0)) == INVALID_ARG
    assert call(lib, plans, entry, box=floats(4.0, float("nan"), 5.0)) == INVALID_ARG


@pytest.mark.parametrize("entry", [e for e in ENTRIES if e.endswith("_cell")])
def test_bad_cell(lib, plans, entry):
    assert call(lib, plans, entry, cell=None) == INVALID_ARG
    assert call(lib, plans, entry, cell=floats(4.0, 0.0, 0.0, 4.0, 0.0, 0.0, 0.0, 0.0, 6.0)) == INVALID_ARG  # two equal rows
    assert call(lib, plans, entry, cell=floats(4.0, 0.0, 0.0, 0.0, float("inf"), 0.0, 0.0, 0.0, 6.0)) == INVALID_ARG


@pytest.mark.parametrize("entry", [e for e in ENTRIES if "owned" not in e])
def test_no_nodes_is_ok_without_the_device(lib, plans, entry):
    # (the owned entries are not here: with N = 0 they still write the scale of `out`, on the device)
    assert call(lib, plans, entry, N=0) == OK

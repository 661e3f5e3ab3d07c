"""The weights-stationary message kernel (e3::msg_ws_kernel) gives THE SAME BITS as the commit before the fold of its first
product was moved between that product's MFMAs: where an instruction is emitted may change, the sequence of operations
on every accumulator element may not.

Every instantiation (fp32 / bf16 storage x open / box / cell) runs once per graph and chunk size on the two hand-made 80-node
graphs of tests/msg_cases.py (one-run tiles, two-run tiles, a run of 70 edges, a ragged last tile; E = 314 and E = 12) with
owned sums, which are reproducible, and the SHA-256 of the output bytes is compared with the digest recorded from the parent
commit on an MI355X (tests/golden/msg_ws_parent_digests.json, written by tests/golden/make_msg_ws_digests.py).  On a mismatch
the failure carries the worst per-block error against the fp64 oracle: a reordered sum stays at rounding level, a wrong
value does not.

The accumulating launch (``owned_sums = False``) sums with fp32 atomics in no fixed order, so it has no digest: it is held
to the 1e-5 per-block bound of tests/test_msg_table_gpu.py against oracle/segnn_oracle.message_sums."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import msg_cases as C

pytestmark = pytest.mark.gpu
LMAX, H = 2, 32
GRAPHS = ("A", "B")
CHUNKS = (0, 1)              # tiles per block: the default chunk (256 edges) and chunks of one tile (every boundary case)
CASES = [(st, per) for st in C.STORAGE for per in C.PERIODICITY]
DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msg_ws_parent_digests.json")


def key(storage, per, name, tpb):
    return f"{storage}-{per}-{name}-tpb{tpb}"


def run(storage, per, name, tpb, owned=True):
    """one launch of the weights-stationary kernel into a NaN-filled ``out``; shared layer and features (seeds: msg_cases)"""
    layer, h, g = C.layer(LMAX, H, storage), C.features(LMAX, H, storage), C.graph(name, per)
    msg = layer._msg
    msg.tiles_per_block, msg.owned_sums = tpb, owned
    try:
        out = torch.full((C.N, msg.width), float("nan"), device=C.DEV)
        with torch.no_grad():
            got = msg.forward(h, g, layer.msg1, layer.msg2, out=out)
        assert got.data_ptr() == out.data_ptr() and got.dtype == torch.float32
        return got
    finally:
        msg.tiles_per_block, msg.owned_sums = 0, True


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def all_digests():
    """what make_msg_ws_digests.py records"""
    return {key(st, per, name, tpb): digest(run(st, per, name, tpb))
            for st, per in CASES for name in GRAPHS for tpb in CHUNKS}


def test_the_shape_has_the_kernel():
    assert C.OWNED[(LMAX, H, "fp32")] and C.OWNED[(LMAX, H, "bf16")]
    with open(DIGESTS) as f:
        rec = json.load(f)
    assert sorted(rec["digests"]) == sorted(key(st, per, name, tpb) for st, per in CASES for name in GRAPHS for tpb in CHUNKS)


@pytest.mark.parametrize("storage,per", CASES, ids=[f"{st}-{per}" for st, per in CASES])
def test_same_bits_as_the_parent(storage, per):
    with open(DIGESTS) as f:
        want = json.load(f)["digests"]
    bad = []
    for name in GRAPHS:
        for tpb in CHUNKS:
            got = run(storage, per, name, tpb)
            assert bool(torch.isfinite(got).all()), (name, tpb)
            d = digest(got)
            print(f"FOLD {key(storage, per, name, tpb)}: {d}")
            if d != want[key(storage, per, name, tpb)]:
                errs = C.block_errors(got, C.reference(LMAX, H, storage, per, name), LMAX, H)
                bad.append((key(storage, per, name, tpb), "worst per-block error vs the fp64 oracle %.2e (bound %.0e)"
                            % (max(errs), C.BOUND[storage])))
    assert not bad, bad


def test_accumulating_launch_against_the_oracle():
    want = C.reference(LMAX, H, "fp32", "open", "A")
    deg = np.diff(C.edges("A")[0])
    for tpb in CHUNKS:
        got = run("fp32", "open", "A", tpb, owned=False)
        assert bool(torch.isfinite(got).all())
        assert float(got[torch.as_tensor(deg == 0, device=C.DEV)].abs().max()) == 0.0
        errs = C.block_errors(got, want, LMAX, H)
        print(f"FOLD accumulating tpb {tpb}: per block " + " ".join(f"{e:.2e}" for e in errs))
        assert max(errs) < C.BOUND["fp32"], (tpb, errs)

"""Helpers of tests/test_tp_r16_table_gpu.py: the six tensor products of a SEGNN taken from the model's own constructors,
their inputs in the segments the model passes, the fp64 oracle of one product (oracle/tp_oracle.py, followed by
oracle/segnn_oracle.gate_blocks where gated) and the per-block error norm.  TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np
import torch

from oracle import segnn_oracle as S
from oracle import tp_oracle as T

DEV = "cuda:0"
KERNEL = b"e3::tp_fwd_mfma_r16_kernel"
PRODUCTS = ("embed", "msg1", "msg2", "upd1", "upd2", "readout")
GATED = ("msg1", "msg2", "upd1")          # products whose output has the gated layout [H | nb H | H x1o (| H x2e)]
HIDDEN = (16, 32, 64)
LMAX = (1, 2)
NTABLE = 23                               # node rows of the table message product #1 gathers from
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def hidden_dim(H, lmax):
    return H * (lmax + 1) ** 2


@functools.lru_cache(maxsize=None)
def model(H, lmax, storage):
    """One single-layer model per (H, l_max, storage): the products under test are its submodules."""
    from scalable_e3_gnn_amd.segnn import SEGNN
    torch.manual_seed(1000 + 10 * H + lmax)
    return SEGNN("1x0e+1x1o", H, "1x1o", 1, lmax).to(DTYPES[storage]).to(DEV)


def product(name, H, lmax, storage):
    m = model(H, lmax, storage)
    return {"embed": m.embed, "readout": m.readout}.get(name) or getattr(m.layers[0], name)


def plan_of(mod):
    """(TPPlan, weights[6], norms[6]) of either module class (L1TensorProduct is the lmax_sh = 1 plan)."""
    if hasattr(mod, "_fused_plan"):
        return mod._fused_plan(), mod._weights() + [None, None], mod._norms() + [None, None]
    return (mod._plan,) + tuple(mod._tensors())


def out_blocks(mod, H, gate):
    """[(name, column slice)] the error is taken over: every contiguous block of the out irreps, or after a gate
    silu(scalars), gated 1o, gated 2e."""
    if gate:
        lmax = max(b.ir.l for b in mod.iro)
        names = ["silu(0e)", "gated 1o", "gated 2e"][:lmax + 1]
        widths = [H, 3 * H, 5 * H][:lmax + 1]
    else:
        names = [f"{i}:{b}" for i, b in enumerate(mod.iro)]
        widths = [b.dim for b in mod.iro]
    out, c = [], 0
    for n, w in zip(names, widths):
        out.append((n, slice(c, c + w)))
        c += w
    return out


def block_errors(got, want, blocks):
    """per block: max |got - want| / max |want|, both maxima over the block's columns and all rows"""
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return [(n, float(np.abs(got[:, s] - want[:, s]).max() / max(np.abs(want[:, s]).max(), 1e-300))) for n, s in blocks]


def worst(errs):
    return max(errs, key=lambda e: e[1])


def _f64(t):
    return t.detach().float().double().cpu().numpy()


def weights_norms(mod):
    W = {c: _f64(getattr(mod, "weights_" + c)) for c in T.CLASSES if hasattr(mod, "weights_" + c)}
    N = {c: (_f64(getattr(mod, "norm_" + c)) if hasattr(mod, "norm_" + c) else np.zeros(0)) for c in T.CLASSES}
    return W, N


def oracle(mod, H, gate, in1, in2):
    """fp64 product (+ gate) on the given (already storage-rounded) in1 [B, D1] / in2 [B, Dy] numpy arrays"""
    lmax_sh = int(round(mod.in2_dim ** 0.5)) - 1
    raw = T.forward(str(mod.iri1), str(mod.iro), lmax_sh, in1, in2, *weights_norms(mod))
    if not gate:
        return raw
    return S.gate_blocks(raw, H, [(l, H) for l in range(1, max(b.ir.l for b in mod.iro) + 1)])


def index_pair(B, seed):
    """dst (ascending) and src (random) rows of the NTABLE-row node table: both hold row 0, the last row and repeated
    rows as soon as B allows it (B >= 3)."""
    g = torch.Generator().manual_seed(seed)
    dst = torch.randint(0, NTABLE, (B,), generator=g)
    src = torch.randint(0, NTABLE, (B,), generator=g)
    if B >= 3:
        dst[0], dst[1], dst[2] = 0, NTABLE - 1, NTABLE - 1
        src[0], src[1], src[2] = NTABLE - 1, 0, 0
    elif B == 2:
        dst[0], dst[1], src[0], src[1] = 0, NTABLE - 1, NTABLE - 1, 0
    else:
        dst[0], src[0] = NTABLE - 1, 0
    return torch.sort(dst).values.int(), src.int()


class Inputs:
    """Inputs of one product in the segments the model passes; ``segments(rows)`` / ``in2`` for the launch, ``dense(rows)``
    the concatenated, storage-rounded in1 rows (numpy fp64) the oracle reads."""

    def __init__(self, name, H, lmax, storage, B, seed, device_rng=False):
        dt = DTYPES[storage]
        D = hidden_dim(H, lmax)
        self.name, self.B, self.dtype = name, B, dt
        if device_rng:   # large batches: drawn on the device, only sampled rows ever come back
            g = torch.Generator(device=DEV).manual_seed(seed)
            rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
            ru = lambda *s: torch.rand(*s, device=DEV, generator=g)
        else:
            g = torch.Generator().manual_seed(seed)
            rn = lambda *s: torch.randn(*s, generator=g).to(DEV)
            ru = lambda *s: torch.rand(*s, generator=g).to(DEV)
        self.in2 = rn(B, (lmax + 1) ** 2)
        self.idx = [None]
        if name == "embed":
            self.tensors = [rn(B, 4).to(dt)]
        elif name == "msg1":
            h = rn(NTABLE, D).to(dt)
            self.tensors = [h, h, ru(B).to(dt)]
            dst, src = index_pair(B, seed + 1)
            self.idx = [dst.to(DEV), src.to(DEV), None]
        elif name == "upd1":
            self.tensors = [rn(B, D).to(dt), (rn(B, D) * 3).to(dt)]   # aggregated messages: three times the scale of h
            self.idx = [None, None]
        else:
            self.tensors = [rn(B, D).to(dt)]

    def segments(self, lo=0, hi=None, tensors=None):
        hi = self.B if hi is None else hi
        return [(t if i is not None else t[lo:hi], i[lo:hi] if i is not None else None)
                for t, i in zip(tensors or self.tensors, self.idx)]

    def y(self, lo=0, hi=None):
        return self.in2[lo:self.B if hi is None else hi]

    def cat(self, lo=0, hi=None):
        """[hi - lo, D1] in1 rows in the storage type, on the device"""
        hi = self.B if hi is None else hi
        parts = []
        for t, i in zip(self.tensors, self.idx):
            r = t[i[lo:hi].long()] if i is not None else t[lo:hi]
            parts.append(r if r.dim() == 2 else r[:, None])
        return torch.cat(parts, 1)

    def dense(self, lo=0, hi=None):
        return _f64(self.cat(lo, hi)), self.y(lo, hi).double().cpu().numpy()


def exact_fp32(mod, H, gate, x, y):
    """The same product on the exact fp32 FMA kernel (``exact = True`` / ``kernel = 1``), gated by ops.gate_blocks."""
    from scalable_e3_gnn_amd import ops
    attr, on, off = ("exact", True, False) if hasattr(mod, "exact") else ("kernel", 1, 0)
    setattr(mod, attr, on)
    try:
        with torch.no_grad():
            raw = mod(x, y)
    finally:
        setattr(mod, attr, off)
    if not gate:
        return raw
    return ops.gate_blocks(raw, H, [(l, H) for l in range(1, max(b.ir.l for b in mod.iro) + 1)])


def misaligned_copy(t):
    """The rows of ``t`` as a column slice at offset 1 of a tensor two columns wider: contiguous rows, a leading dimension
    that is no multiple of 16 bytes, a base that is not 16-byte aligned."""
    if t.dim() == 1:
        t = t[:, None]
    wide = torch.zeros(t.shape[0], t.shape[1] + 2, dtype=t.dtype, device=t.device)
    v = wide[:, 1:t.shape[1] + 1]
    v.copy_(t)
    return v


# ---- hand-made dst arrays of the fused scatter (ascending, 40 nodes) ----
SCATTER_NODES = 40


def scatter_dst(case):
    if case == "B1":
        deg = {17: 1}
    elif case == "B17":
        deg = {3: 5, 4: 1, 9: 11}                    # rows 6..16: a run across the tile edge; node 39 and others isolated
    else:
        # rows 0..15: node 1 (exactly one tile); 16, 17: degree-1 nodes 2, 3; 18..31: node 4, ending on the tile edge at 32;
        # node 5 isolated behind it; 32..121: node 6, 90 rows (more than a workgroup's 64); nodes 0, 20, 21, 39 isolated
        deg = {1: 16, 2: 1, 3: 1, 4: 14, 6: 90}
        cyc = [1, 3, 2, 5, 1, 4]
        free = [n for n in range(7, 39) if n not in (20, 21)]
        for k, n in enumerate(free[:-1]):
            deg[n] = cyc[k % len(cyc)]
        deg[free[-1]] = 211 - sum(deg.values())
        assert deg[free[-1]] >= 1
    d = np.zeros(SCATTER_NODES, np.int64)
    for n, c in deg.items():
        d[n] = c
    return np.repeat(np.arange(SCATTER_NODES), d).astype(np.int32), d

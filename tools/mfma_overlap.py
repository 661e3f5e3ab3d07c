#!/usr/bin/env python3
"""Where do the fold fma sit relative to the MFMAs?  Reads a `hipcc -S` listing of csrc/e3_msg_ws.hip (flags of
tools/build_variant.sh + `--cuda-device-only -S`) and prints, for every kernel whose mangled name starts with the prefix,
one line per MFMA run.  A run = the MFMAs of one straight-line stretch (no label, branch or barrier inside): the tensor
product of one role.  Columns:

  mfma    MFMA instructions of the run
  span    instructions from the first to the last MFMA (both included)
  inside  fold-type fma (v_pk_fma_f32, v_fmac_f32, v_fma_f32) inside the span
  clump   the longest stretch of fold-type fma inside the span with no MFMA in it
  behind  fold-type fma between the last MFMA and the next barrier or branch

It looks at nothing but MFMA and fma placement.  Usage: tools/mfma_overlap.py listing.s [kernel-name prefix]"""
import re
import sys

FOLD = ("v_pk_fma_f32", "v_fmac_f32", "v_fma_f32")
END = ("s_barrier", "s_cbranch", "s_branch", "s_endpgm", "s_setpc")


def kernels(text, prefix):
    """(name, [opcode | None for a label], [line number]) of every kernel whose name starts with prefix"""
    out, name, ops, lines = [], None, None, None
    for no, line in enumerate(text.split("\n"), 1):
        m = re.match(r"(\w+):\s*; @", line)
        if m:
            name, ops, lines = m.group(1), [], []
            continue
        if name is None:
            continue
        if ".end_amdhsa_kernel" in line or line.startswith(".Lfunc_end"):
            if name.startswith(prefix):
                out.append((name, ops, lines))
            name = None
            continue
        if re.match(r"\.L\w+:", line):
            ops.append(None)
            lines.append(no)
            continue
        m = re.match(r"\s+([a-z][a-z_0-9]+)", line)
        if m and not line.lstrip().startswith("."):
            ops.append(re.sub(r"_(e32|e64|dpp|sdwa)$", "", m.group(1)))
            lines.append(no)
    return out


def runs(ops, lines):
    """-> [(mfma, span, inside, clump, behind, first line, last line)]"""
    out, i, n = [], 0, len(ops)
    while i < n:
        # one straight-line stretch [i, j)
        j = i
        while j < n and ops[j] is not None and not ops[j].startswith(END):
            j += 1
        seg = ops[i:j]
        at = [k for k, o in enumerate(seg) if o.startswith("v_mfma")]
        if at:
            first, last = at[0], at[-1]
            inside = clump = cur = 0
            for o in seg[first:last + 1]:
                if o.startswith("v_mfma"):
                    cur = 0
                elif o in FOLD:
                    inside += 1
                    cur += 1
                    clump = max(clump, cur)
            behind = sum(1 for o in seg[last + 1:] if o in FOLD)
            out.append((len(at), last - first + 1, inside, clump, behind, lines[i + first], lines[i + last]))
        i = j + 1
    return out


def main():
    text = open(sys.argv[1]).read()
    prefix = sys.argv[2] if len(sys.argv) > 2 else "_ZN2e313msg_ws_kernel"
    for name, ops, lines in kernels(text, prefix):
        print(name)
        print(f"  {'run':>3} {'mfma':>5} {'span':>5} {'inside':>6} {'clump':>5} {'behind':>6}  lines")
        for k, r in enumerate(runs(ops, lines)):
            print(f"  {k:3d} {r[0]:5d} {r[1]:5d} {r[2]:6d} {r[3]:5d} {r[4]:6d}  {r[5]}-{r[6]}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Record the SHA-256 digests that tests/test_l1tp_parent_bits_gpu.py compares against.

Run on an MI355X with the library built from the commit whose bits are to be kept (the parent of the change that gave the
pinned operator its class table and shared W-mix helpers): generic and MFMA forward, packed weights and e3_l1tp_backward on
the four plans of the test.  The file it writes, tests/golden/l1tp_parent_digests.json, is committed data.

    python tests/golden/make_l1tp_digests.py [output.json [commit]]
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import models  # noqa: E402,F401
import test_l1tp_parent_bits_gpu as T  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.DIGESTS
    first = T.all_digests()
    assert T.all_digests() == first, "these launches sum in a fixed order"
    rev = sys.argv[2] if len(sys.argv) > 2 else subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True,
                                                               text=True).stdout.strip()
    with open(out, "w") as f:
        json.dump({"recorded_from": rev, "what": "sha256 of the raw bytes of each tensor, B = 33; packed buffers pre-filled "
                   "with 0xA5", "digests": first}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(first)} digests -> {out}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Golden fixture for the scan: what the REFERENCE's own iterator visited on
the two streams stored in tests/golden/get_keys.npz.

For each stream, oracle/_ref/ref_db writes the database and `ref_db --verify`
reopens a copy (make_golden_getkeys.run_ref_verified, with its
raise_hstable_size step) and walks it with Database::NewIterator: it prints how
many entries the iterator visited (`iterated`) and how many of those had a key
never put, a status that is not OK or a value other than the last one put for
that key (`iterator_bad`).  Exit 0 with iterator_bad 0 and iterated equal to
the number of distinct keys is the reference confirming that its iterator
visits exactly the distinct keys, each with its last value.  Those two counts
per stream are all this fixture stores; the files the run leaves must be the
ones get_keys.npz already holds.

    python tests/golden/make_golden_scan.py      -> tests/golden/scan.npz
"""
from __future__ import annotations

import contextlib
import io
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import oracle  # noqa: E402
from make_golden_getkeys import run_ref_verified  # noqa: E402

SRC = os.path.join(ROOT, "tests", "golden", "get_keys.npz")
OUT = os.path.join(ROOT, "tests", "golden", "scan.npz")


def main() -> None:
    orc = oracle.Oracle()
    z = np.load(SRC, allow_pickle=False)
    arrs, names = {}, []
    for name in (str(n) for n in z["names"]):
        stream = z[f"{name}__stream"].tobytes()
        hash_type = int(z[f"{name}__opts"][1])
        printed = io.StringIO()
        with contextlib.redirect_stdout(printed):
            files = run_ref_verified(orc, stream, hash_type)     # raises unless --verify exits 0
        m = re.search(r"(\d+) iterated (\d+) iterator_bad", printed.getvalue())
        if not m:
            raise SystemExit(f"{name}: no iterator counts in {printed.getvalue()!r}")
        iterated, bad = int(m.group(1)), int(m.group(2))
        stored = {str(f): z[f"{name}__file_{f}"].tobytes() for f in z[f"{name}__files"]}
        # the HSTable header holds the time of writing: compare the files from the entries on
        if sorted(files) != sorted(stored) or any(files[f][8192:] != stored[f][8192:] for f in files):
            print(f"   note: {name}: this run's files differ from get_keys.npz beyond the header block")
        nkeys = len(z[f"{name}__keys"])
        print(f"{name}: iterated {iterated}, iterator_bad {bad}, distinct keys {nkeys}")
        if bad != 0 or iterated != nkeys:
            raise SystemExit(f"{name}: the reference's iterator did not visit exactly the distinct keys")
        names.append(name)
        arrs[f"{name}__iterated"] = np.array([iterated], np.uint64)
        arrs[f"{name}__iterator_bad"] = np.array([bad], np.uint64)
    arrs["names"] = np.array(names, dtype="U16")
    np.savez_compressed(OUT, **arrs)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

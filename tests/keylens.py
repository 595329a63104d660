"""tests/golden/key_lengths.npz as the key-length tests read it (not a test
module): per stream the files the reference wrote, the put stream, the
distinct keys (sorted) with the length and CRC32C of the value the reference's
own Database::Get returned, the twin pairs, the hot keys and the reference's
iterator counts.  See tests/golden/make_golden_keylens.py.
"""
from __future__ import annotations

import os
import sys

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_golden_put import decode_stream  # noqa: E402


def load() -> dict:
    z = load_golden("key_lengths.npz")
    out = {}
    for name in (str(n) for n in z["names"]):
        kb, ko = z[f"{name}__keys"].tobytes(), [int(o) for o in z[f"{name}__key_off"]]
        keys = [kb[a:b] for a, b in zip(ko, ko[1:])]
        puts = decode_stream(z[f"{name}__stream"].tobytes())
        out[name] = {
            "files": {str(f): z[f"{name}__file_{f}"].tobytes() for f in z[f"{name}__files"]},
            "hstable_size": int(z[f"{name}__opts"][0]), "hash_type": int(z[f"{name}__opts"][1]),
            "puts": puts, "last": {k: v for k, v, _ in puts},
            "keys": keys, "lens": z[f"{name}__len"], "crcs": z[f"{name}__crc"],
            "twins": [(keys[int(a)], keys[int(b)], int(at)) for a, b, at in z[f"{name}__twins"]],
            "hot": [keys[int(i)] for i in z[f"{name}__hot"]],
            "iterated": int(z[f"{name}__iterated"][0]), "iterator_bad": int(z[f"{name}__iterator_bad"][0]),
        }
    return out

"""CPU: the sequence-level block builder (tests/lz4_blocks.py) against the
oracle and the reference, the coverage conditions of the GPU sets, and the
fixture tests/golden/foreign_blocks.npz.

Three independent statements of the decode rules meet here: the builder's
byte-by-byte copy, the oracle's C restatement (oracle/lz4_oracle.c) and the
reference's own LZ4_decompress_safe_partial (oracle/_ref, where built).  The
GPU tests (tests/test_gpu_foreign_blocks.py) then hold the kernels to the
builder's bytes for well-formed blocks and to the oracle's result otherwise.
"""
import os
import random

import numpy as np
import pytest

import lz4_blocks as L
import oracle
from conftest import load_golden

SET_NAMES = ("a", "b", "c", "d", "e")


def _ref():
    if not os.path.exists(oracle.REF_SO):
        pytest.skip("oracle/_ref not built (no reference here)")
    return oracle.Reference()


def _orc_fill(orc, blk, size, tgt, fill):
    """The oracle's decode into a buffer filled with `fill` (tests/golden/
    make_golden.py's convention: bytes that differ between a 0x00 and a 0xFF
    fill were never written by the decoder -- an offset-0 copy -- and are
    unspecified)."""
    src = np.zeros(len(blk) + 64, np.uint8)
    src[: len(blk)] = np.frombuffer(blk, np.uint8)
    dst = np.full(max(size, 0) + 64, fill, np.uint8)
    r = orc.lib.orc_decompress_safe_partial(oracle._ptr(src), oracle._ptr(dst), len(blk), tgt, size)
    return r, (dst[:r].tobytes() if r > 0 else b"")


# ------------------------------------------------------------- the builder
def test_encode_hand_checked():
    """Token nibbles, 255-chains and the little-endian offset, against bytes
    written by hand."""
    blk, dec = L.encode([(b"abcdefgh", 3, 4)], b"ijklmnopqrstuvwx")
    assert blk == bytes([0x80]) + b"abcdefgh" + b"\x03\x00" + bytes([0xF0, 0x01]) + b"ijklmnopqrstuvwx"
    assert dec == b"abcdefgh" + b"fghf" + b"ijklmnopqrstuvwx"
    # 15 literals: nibble 15 + a 0 byte; 270: 15 + 255 + 0; match 19: nibble 15 + 0; 274: 15 + 255 + 0
    assert L.encode_sequence(b"x" * 15, 0x1234, 19) == bytes([0xFF, 0]) + b"x" * 15 + b"\x34\x12" + bytes([0])
    assert L.encode_sequence(b"x" * 270, 1, 274)[:3] == bytes([0xFF, 255, 0])
    assert L.encode_sequence(b"x" * 270, 1, 274)[-4:] == bytes([1, 0, 255, 0])
    assert L.encode_sequence(b"", 65535, 18) == bytes([0x0E, 0xFF, 0xFF])
    # an overlapping match repeats its period byte by byte
    assert L.encode([(b"ab", 2, 7)], b"")[1] == b"ab" + b"abababa"
    assert L.encode([(b"abc", 1, 5)], b"")[1] == b"abc" + b"ccccc"


def test_well_formed_rule():
    seq = (bytes(32), 7, 4)
    assert L.well_formed([seq], bytes(8), 44)           # literals end at size - 12
    assert not L.well_formed([seq], bytes(7), 43)       # ... at size - 11
    assert not L.well_formed([seq], bytes(5), 41)       # the 41-byte block
    assert L.well_formed([(bytes(20), 20, 7)], bytes(5), 32)      # match ends at size - 5
    assert not L.well_formed([(bytes(20), 21, 7)], bytes(5), 32)  # offset past the start
    assert not L.well_formed([(bytes(20), 0, 7)], bytes(5), 32)
    assert not L.well_formed([(bytes(20), 20, 7)], bytes(5), 33)  # the last run does not end at size


def test_classify_by_hand():
    seqs = [(bytes(60), 10, 19), (b"", 63, 64), (bytes(61), 4033, 274)]
    blk, dec = L.encode(seqs, bytes(40))
    c = L.classify(seqs, len(dec), len(blk))
    assert (c[0]["lit_class"], c[0]["ml_class"], c[0]["off_class"], c[0]["nt"]) == (
        "byte<=45", "byte<=254", "periodic", 63)
    assert (c[0]["tok_ip"], c[0]["lit_ip"], c[0]["off_ip"], c[0]["mllen_ip"], c[0]["end_ip"]) == (
        0, 2, 62, (64, 65), 65)
    assert (c[1]["tok_ip"], c[1]["lit_class"], c[1]["ml_class"], c[1]["off_class"], c[1]["steps"], c[1]["nt"]) == (
        65, "nibble", "byte<=254", "periodic", "one", 3)
    assert (c[2]["lit_class"], c[2]["ml_class"], c[2]["off_class"], c[2]["steps"], c[2]["nt"]) == (
        "byte>45", "chain", "far", "many", None)
    assert c[2]["op"] == 60 + 19 + 64 and not c[2]["block_fast"] and c[0]["block_fast"]
    # straddles: a token as the last byte before input position 2 048, its offset across 4 096
    rng = random.Random(1)
    cs = L.straddle_block(rng, "offset", 2, "x")
    cl = L.classify(cs.seqs, cs.size, len(cs.block))
    assert [x["off_ip"] for x in cl if "offset" in x["straddle"][2048]] == [2047, 4095]
    assert [x["off_ip"] for x in cl if "offset" in x["straddle"][4096]] == [4095]


# ---------------------------------------------------- coverage conditions
@pytest.mark.parametrize("name", SET_NAMES)
def test_coverage_conditions(name):
    """At least 20 sequences on each side of every boundary of the launch, every
    pair of the sweep, every constructed straddle, every ill-formed class, at
    least 90 % well-formed (lz4_blocks.coverage_problems)."""
    assert L.coverage_problems(name) == []


def test_sets_reach_their_launch():
    """Sizes that select each launch (lz4_decompress.hip launch_decompress)."""
    a, b, c, d, e = (L.SETS[n]() for n in SET_NAMES)
    assert max(len(x.block) for x in a) <= 3057 and max(x.size for x in a) <= 2900 and min(
        x.size for x in a if x.kind == "random") >= 20 and len(a) > 1300
    assert 3057 < max(len(x.block) for x in b) <= 8192 + 32 + 24 and max(x.size for x in b) == 8192
    assert any(x.size == 8192 and not x.seqs and len(x.block) > 8192 for x in b)
    assert 8192 < max(x.size for x in c) == 65546
    assert max(x.size for x in d) == 70000
    assert [x.size for x in e] == [9000, 20000, 70000]
    svc = L.service_cases()
    assert 180 <= len(svc) <= 260 and max(x.size for x in svc) <= 8192
    assert sum(1 for x in svc if x.decoded is None) >= 30


# --------------------------------------------- oracle = builder = reference
@pytest.mark.parametrize("name", SET_NAMES)
def test_oracle_equals_builder(orc, name):
    n = 0
    for c in L.SETS[name]():
        if c.decoded is None:
            continue
        r, out = orc.decompress(c.block, c.size)
        assert r == c.size and out == c.decoded, c.name
        n += 1
    assert n >= 3


def test_known_end_rule(orc):
    """32 literals, a 4-byte match and 5 last literals: the literals end past
    size - 12, so the decoder takes them for the last run and returns 32."""
    b41 = [c for c in L.ill_fixed() if c.name == "b41"][0]
    r, out = orc.decompress(b41.block, 41)
    assert r == 32 and out == bytes(range(65, 97))
    assert orc.decompress(b"\x00", 0)[0] == 0 and orc.decompress(b"\x10\x41", 0)[0] == -1


@pytest.mark.parametrize("name", ("a", "bx", "c", "dx", "e"))
def test_oracle_equals_reference(orc, name):
    """Return codes always, bytes where r > 0 and the output is specified, for
    the full size and the partial targets 1, 64, size // 3, size - 13, size - 1."""
    ref = _ref()
    for c in L.stored_sets()[name]:
        for t in [c.size] + L.targets_for(c.size):
            rr, rout = ref.decompress(c.block, c.size, t)
            r0, o0 = _orc_fill(orc, c.block, c.size, t, 0x00)
            r1, o1 = _orc_fill(orc, c.block, c.size, t, 0xFF)
            assert r0 == rr and r1 == rr, (c.name, t, r0, rr)
            if rr > 0 and o0 == o1:
                assert o0 == rout, (c.name, t)
            if c.decoded is not None:
                assert o0 == o1, (c.name, t)      # a well-formed block leaves nothing unspecified
                if t == c.size:
                    assert rr == c.size and rout == c.decoded, c.name


# ------------------------------------------------------------- the fixture
def test_fixture_matches_oracle(orc):
    """foreign_blocks.npz (the reference's return codes and output CRC32Cs)
    against the oracle on the sets regenerated from their seeds."""
    g = load_golden("foreign_blocks.npz")
    sets = L.stored_sets()
    assert sorted(g) == sorted("%s_%s" % (s, k) for s in sets for k in ("ret", "crc", "tret", "tcrc"))
    for s, cases in sets.items():
        got = L.results(orc, cases)
        for k, v in got.items():
            assert np.array_equal(g["%s_%s" % (s, k)], v), (s, k)


def test_fixture_matches_reference():
    ref = _ref()
    g = load_golden("foreign_blocks.npz")
    for s, cases in L.stored_sets().items():
        got = L.results(ref, cases)
        for k, v in got.items():
            assert np.array_equal(g["%s_%s" % (s, k)], v), (s, k)

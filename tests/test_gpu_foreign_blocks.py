"""GPU: every decode launch on LZ4 blocks built sequence by sequence
(tests/lz4_blocks.py), not by a compressor.

Every other block the suite decodes is one parser's output or a byte
mutation of it, so the decoders (kingdb_amd/csrc/lz4_decompress.hip:
decode_block, decode_ring) were pinned only on the sequences that parser
emits.  Their fast paths turn on exact properties of one sequence (literal
count 60|61, match length 273|274 and 64|65, offset against the match length
and against 4 032, the next token's lane 62|63, the distance to both ends,
the input ring's refills); these sets put at least 20 sequences on each side
of each (tests/test_lz4_blocks_model.py asserts the counts without a GPU).

  a  lz4_decompress_kernel<false, 3u>    ~1 350 blocks, outputs <= 2 900 B, blocks <= 3 057 B
  b  lz4_decompress_kernel<false, 5u>    (a) + blocks up to 8 192 B of output
  c  lz4_decompress_mixed_kernel<false>  4 KiB input ring: LDS pass <= 4 096 B, ring pass up to 65 546 B
  d  the same kernel, 8 KiB input ring   (c) + one block of 70 000 B (LDS pass <= 6 144 B)
  e  lz4_decompress_big_kernel           three single-block calls: 9 000, 20 000, 70 000 B
  f  frame mode                          the well-formed blocks of (a), (c), (d) behind the 8-byte header
  g  the per-call service                ~220 blocks <= 8 192 B, well- and ill-formed, with targets

Every comparison is exact: the return code and every byte.  The expectation
for a well-formed block is the builder's own bytes; for an ill-formed one, and
for partial targets, the oracle's result (pinned to the reference by the CPU
tests).  Independently of the oracle, each result must also match the
reference's return code and output CRC32C in tests/golden/foreign_blocks.npz.
"""
import struct

import numpy as np
import pytest

import lz4_blocks as L
from conftest import load_golden

pytestmark = pytest.mark.gpu

K3 = "lz4_decompress_kernel<false, 3u>"
K5 = "lz4_decompress_kernel<false, 5u>"
KMIX = "lz4_decompress_mixed_kernel<false>"
KBIG = "lz4_decompress_big_kernel<false, 4096u>"


@pytest.fixture(scope="module")
def golden():
    g = load_golden("foreign_blocks.npz")
    for k in ("ret", "crc", "tret", "tcrc"):
        g["b_" + k] = np.concatenate([g["a_" + k], g["bx_" + k]])
        g["d_" + k] = np.concatenate([g["c_" + k], g["dx_" + k]])
    return g


def _check(orc, golden, name, idx, cases, got, partial):
    """got[j] is the device's (ret, bytes) for cases[j], which is case idx[j] of
    set `name`, decoded with its partial target or with the full size."""
    assert len(got) == len(cases)
    gr, gc = golden[name + ("_tret" if partial else "_ret")], golden[name + ("_tcrc" if partial else "_crc")]
    for (r, out), c, i in zip(got, cases, idx):
        t = L.target_of(c) if partial else c.size
        if c.decoded is not None and not partial:
            er, eout = c.size, c.decoded
        else:
            er, eout = orc.decompress(c.block, c.size, t)
        assert r == er, (c.name, t, r, er)
        assert out == eout, (c.name, t)
        assert r == int(gr[i]), (c.name, t, r, int(gr[i]))
        if r > 0:
            assert orc.crc32c(out) == int(gc[i]), (c.name, t)


@pytest.mark.parametrize("partial", [False, True], ids=["full", "targets"])
@pytest.mark.parametrize("name,kernel,top", [("a", K3, 2900), ("b", K5, 8192), ("c", KMIX, 65546),
                                             ("d", KMIX, 70000)])
def test_batch_launch(gpu, orc, golden, name, kernel, top, partial):
    """(a)-(d): one launch over the whole set (ill-formed blocks included), and
    one over its well-formed blocks with a target below the size each."""
    cases = L.SETS[name]()
    idx = [i for i, c in enumerate(cases) if c.decoded is not None or not partial]
    sub = [cases[i] for i in idx]
    # what selects the launch (launch_decompress): the largest output and block
    mo, mi = max(c.size for c in sub), max(len(c.block) for c in sub)
    if name == "a":
        assert mo <= top and mi <= 3057
    elif name == "b":
        assert mo == top and 3057 < mi <= 8192 + 8192 // 255 + 24
    else:
        assert mo == top
    tg = [L.target_of(c) for c in sub] if partial else None
    got = gpu.decompress_blocks([c.block for c in sub], [c.size for c in sub], tg)
    assert gpu.last_kernels() == [kernel]
    _check(orc, golden, name, idx, sub, got, partial)


@pytest.mark.parametrize("partial", [False, True], ids=["full", "targets"])
def test_single_block_ring_launch(gpu, orc, golden, partial):
    """(e): n == 1 in block mode with an output above 8 192 bytes is the ring
    decoder's own launch."""
    for i, c in enumerate(L.set_e()):
        tg = [L.target_of(c)] if partial else None
        got = gpu.decompress_blocks([c.block], [c.size], tg)
        assert gpu.last_kernels() == [KBIG]
        _check(orc, golden, "e", [i], [c], got, partial)


@pytest.mark.parametrize("name,kernel", [("a", "lz4_decompress_kernel<true, 3u>"),
                                         ("c", "lz4_decompress_mixed_kernel<true>"),
                                         ("d", "lz4_decompress_mixed_kernel<true>")])
def test_frame_mode(gpu, name, kernel):
    """(f): CompressorLZ4 frames (u32 stored size = block + 8, u32 source size)
    around the well-formed blocks: status 0 and the builder's bytes."""
    cases = [c for c in L.SETS[name]() if c.decoded is not None]
    frames = [struct.pack("<II", len(c.block) + 8, c.size) + c.block for c in cases]
    got = gpu.decompress_frames(frames, [c.size for c in cases])
    assert gpu.last_kernels() == [kernel]
    for (st, out), c in zip(got, cases):
        assert st == 0, c.name
        assert out == c.decoded, c.name


def test_service(gpu, orc, golden):
    """(g): LZ4_decompress_safe_partial one block per call."""
    cases = L.service_cases()
    for partial in (False, True):
        got = [gpu.decompress_safe_partial(c.block, L.target_of(c) if partial else c.size, c.size)
               for i, c in enumerate(cases)]
        _check(orc, golden, "g", list(range(len(cases))), cases, got, partial)

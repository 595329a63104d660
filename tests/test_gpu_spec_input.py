"""GPU: the batched parse (lz4_compress.hip, compress_block's kBatch) on inputs
sorted by how a sequence's match length relates to the one before it.

Written for a parse that reads the next sequence's input words early, at a
match end guessed from the value's previous sequence (DESIGN.md section 4.1;
measured in round 8 and not kept, profiles/r08/r08_spec_input.patch).  Such a
parse must give the oracle's bytes whether a guess is right or wrong, and the
cases stay as parity cases of the parse that is built: values whose match
lengths repeat (the match lane early, mid and late in the search chunk), values
whose consecutive match lengths always differ, matches that take the count's
>= 64-byte continuation and two length-run bytes, values cut around the
end-of-value limits (the last match ends at, before and past mflimit), every
entry point that runs the batched parse, and a launch that gives every parse
wave of a workgroup values.  Where a case is about repeating or differing
lengths, that property is asserted from the oracle's parse of the input, so a
changed generator cannot hollow the case out.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

BATCHED = "lz4_compress_kernel<true, true, 1u, 10u>"
BATCHED_BLOCKS = "lz4_compress_kernel<false, true, 1u, 10u>"
MIXED = "lz4_compress_mixed_kernel<true, 10u>"


def _runs_value(seed, n, tail):
    """tests/test_gpu_batch_emit.py's value shape: runs of 1-30 letters of a
    12-letter alphabet, optionally an incompressible tail."""
    rng = np.random.default_rng(seed)
    runs = rng.integers(1, 31, n)
    letters = rng.integers(0, 12, n).astype(np.uint8) + ord("a")
    v = np.repeat(letters, runs)[:n].tobytes()
    if tail:
        cut = int(rng.integers(0, n))
        v = v[:cut] + rng.integers(0, 256, n - cut, dtype=np.uint8).tobytes()
    return v


def _pieces(seed, n, lens):
    """n bytes of pieces X X, each X fresh random bytes, |X| cycling through lens."""
    rng = np.random.default_rng(seed)
    out, total, k = [], 0, 0
    while total < n:
        x = rng.integers(0, 256, lens[k % len(lens)], dtype=np.uint8).tobytes()
        out.append(x + x)
        total += 2 * len(x)
        k += 1
    return b"".join(out)[:n]


def _match_lengths(block):
    """The match lengths of an LZ4 block's sequences, in order."""
    i, out = 0, []
    while i < len(block):
        tok = block[i]
        i += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                b = block[i]
                i += 1
                lit += b
                if b != 255:
                    break
        i += lit
        if i >= len(block):
            break
        i += 2
        ml = tok & 15
        if ml == 15:
            while True:
                b = block[i]
                i += 1
                ml += b
                if b != 255:
                    break
        out.append(ml + 4)
    return out


def _repeats(orc, vals):
    """(pairs of consecutive sequences of a value, pairs with equal match length) over vals."""
    pairs = same = 0
    for v in vals:
        m = _match_lengths(orc.compress(v))
        pairs += max(len(m) - 1, 0)
        same += sum(1 for a, b in zip(m, m[1:]) if a == b)
    return pairs, same


FILL = [_runs_value(9100 + k, 600 + 7 * k, False) for k in range(4)]   # keeps every launch batched (a value >= 512 B)


def _check_frames(gpu, orc, vals, kernel=BATCHED):
    want = [orc.frame(v) for v in vals]
    got = gpu.compress_frames(vals)          # raises unless every status is 0
    import kingdb_amd as K
    assert K.last_kernels()[0] == kernel, K.last_kernels()
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, [(i, len(vals[i]), len(got[i]), len(want[i])) for i in bad[:10]]


def _hit_values():
    return [_pieces(100 * x + s, n, [x]) for x in (8, 25, 50, 60) for n in (512, 1000, 4096) for s in range(6)]


def test_hits(gpu, orc):
    vals = _hit_values()
    pairs, same = _repeats(orc, vals)
    print(f"hits: {same} of {pairs} consecutive sequences repeat their match length")
    assert pairs > 1000 and same >= 0.8 * pairs, (pairs, same)
    _check_frames(gpu, orc, vals + FILL)


def _miss_values():
    return [_pieces(700 + s, n, lens) for lens in ([20, 33], [50, 9], [60, 61]) for n in (512, 1000, 4096)
            for s in range(4)]


def test_misses_only(gpu, orc):
    vals = _miss_values()
    pairs, same = _repeats(orc, vals)
    print(f"misses: {same} of {pairs} consecutive sequences repeat their match length")
    assert pairs > 500 and same == 0, (pairs, same)
    # irregular lengths, catch-up through overlapping matches
    runs = [_runs_value(40 + k, 512 + (k * 211) % 3585, k % 3 == 0) for k in range(60)]
    _check_frames(gpu, orc, vals + runs + FILL)


def test_long_matches(gpu, orc):
    v100 = [_pieces(1100 + s, n, [100]) for n in (1000, 4096) for s in range(6)]
    v300 = [_pieces(1300 + s, n, [300]) for n in (1300, 4096) for s in range(6)]
    for vals, x in ((v100, 100), (v300, 300)):
        for v in vals:
            m = _match_lengths(orc.compress(v))
            # every count but a value's last (cut by the end of the value) takes the continuation
            assert len(m) >= 2 and all(a >= 4 + 64 for a in m[:-1]), (x, m)
            if x == 300:
                assert all(a >= 4 + 15 + 255 for a in m[:-1]), m      # two run-length bytes
    pairs, same = _repeats(orc, v100 + v300)
    print(f"long matches: {same} of {pairs} consecutive sequences repeat their match length")
    assert same >= 0.5 * pairs, (pairs, same)                       # long lengths mostly repeat, too
    _check_frames(gpu, orc, v100 + v300 + FILL)


def test_value_end(gpu, orc):
    stream = _pieces(1500, 4096, [50])
    vals = [stream[:n] for n in list(range(4084, 4097)) + list(range(512, 525))]
    assert len(vals) == 26
    # the last match ends at, before and past mflimit (S - 12): the block's
    # last literals are then 5 bytes (the match ran to matchlimit) or more
    tails = set()
    for v in vals:
        blk = orc.compress(v)
        m = _match_lengths(blk)
        assert len(m) >= 4
        tails.add(_last_literals(blk))
    assert 5 in tails and max(tails) > 12, sorted(tails)
    _check_frames(gpu, orc, vals)


def _last_literals(block):
    """The length of an LZ4 block's last literal run."""
    i, lit = 0, 0
    while i < len(block):
        tok = block[i]
        i += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                b = block[i]
                i += 1
                lit += b
                if b != 255:
                    break
        i += lit
        if i >= len(block):
            return lit
        i += 2
        if tok & 15 == 15:
            while block[i] == 255:
                i += 1
            i += 1
    return lit


def _entry_values():
    return _hit_values()[::3] + _miss_values()[::3] + [_runs_value(60 + k, 512 + (k * 197) % 3585, k % 4 == 0)
                                                       for k in range(40)]


def test_blocks_entry_point(gpu, orc):
    import kingdb_amd as K
    vals = _entry_values()
    want = [orc.compress(v) for v in vals]
    got = gpu.compress_blocks(vals)                    # caps at the bound: batched, kFrame = false
    assert K.last_kernels()[0] == BATCHED_BLOCKS, K.last_kernels()
    for i, ((r, blk), w) in enumerate(zip(got, want)):
        assert r == len(w) and blk == w, (i, r, len(w))
    caps = [orc.compress_bound(len(v)) - 1 for v in vals]   # one byte below: the guard path
    got = gpu.compress_blocks(vals, caps=caps)
    for i, ((r, blk), w) in enumerate(zip(got, want)):
        assert r == len(w) and blk == w, (i, r, len(w))


def test_mixed_launch(gpu, orc):
    """600 B, 4 KiB and 20 KiB values in one launch: the mixed kernel, whose
    small pass parses values of 512 bytes and more in the batched form."""
    vals = []
    for s in range(12):
        vals += [_pieces(1700 + s, 600, [25]), _pieces(1800 + s, 4096, [50]), _pieces(1900 + s, 4096, [20, 33]),
                 _pieces(2000 + s, 20000, [50])]
    _check_frames(gpu, orc, vals, MIXED)


def _child():
    import kingdb_amd as K
    import oracle
    K.set_device(0)
    orc = oracle.Oracle()
    vals = _entry_values() + FILL
    got = K.compress_frames(vals)
    bad = [i for i, (g, v) in enumerate(zip(got, vals)) if g != orc.frame(v)]
    print("PARITY OK" if not bad and K.last_kernels()[0] == BATCHED else f"PARITY FAIL {bad[:10]}", K.last_kernels())
    return 1 if bad else 0


def test_helpers_off_child(gpu):
    """The frames case with the emission helpers off: every value is emitted by its parse wave."""
    e = dict(os.environ)
    e["KDB_LZ4_EMIT_HELPERS"] = "0"
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=e, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PARITY OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


def test_all_ten_regions(gpu, orc):
    """4 096 short values of the hit shape in one launch: every parse wave of a
    workgroup takes values, the one in the last 16 KiB of the 160 KiB included."""
    streams = [_pieces(2100 + s, 640, [(8, 25, 50, 60)[s % 4]]) for s in range(64)]
    vals = [streams[k % 64][:512 + (k * 7) % 129] for k in range(4096)]
    assert min(len(v) for v in vals) == 512 and max(len(v) for v in vals) == 640
    pairs, same = _repeats(orc, vals[:256])
    assert same > 0.5 * pairs, (pairs, same)             # the repeating shape: most lengths repeat
    _check_frames(gpu, orc, vals)


if __name__ == "__main__":
    sys.exit(_child())

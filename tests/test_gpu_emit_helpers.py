"""GPU: the emission helper waves of the batched <= 4 KiB compress kernel
(lz4_compress.hip, "emission helper waves").  A parse wave whose value ended
as one batch (at most 64 sequences) hands the emission to an LDS-free helper
wave of its workgroup through a ring in global scratch; values that flushed
mid-value, and every value when the ring is full or the helpers are off, are
emitted by the parse wave.  Whichever wave wrote a frame, it must be the
oracle's byte for byte, with status 0 and the right frame length
(compress_frames raises on any other status, so a sentinel left behind fails).

The cases sit on the hand-off's edges: 0, 1, 63, 64 and 65 sequences (65 is
the first value that flushes mid-value), literal and match runs around the
length-run boundaries read from global memory instead of LDS, the raw fallback
taken in the helper, launches smaller than the grid and one past it, ring depth
1 (hand-offs faster than a helper emits: the ring-full path), helpers off,
back-to-back launches (no slot of an earlier launch may be consumed), and the
blocks entry point (kFrame = false) on both sides of the guard path.
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

# the batched ten-wave kernel (its helper waves are part of the same kernel)
BATCHED = "lz4_compress_kernel<true, true, 1u, 10u>"
BATCHED_BLOCKS = "lz4_compress_kernel<false, true, 1u, 10u>"


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


def _sequences(block):
    """[(literal length, match length)] of an LZ4 block; the last literals have match length 0."""
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
            out.append((lit, 0))
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
        out.append((lit, ml + 4))
    return out


def _nseq(orc, v):
    return sum(1 for _, m in _sequences(orc.compress(v)) if m)


def _with_count(orc, want, seed):
    """A runs value (short runs of a small alphabet) that parses into exactly `want` sequences."""
    for s in range(seed, seed + 20):         # (a length step can skip a count: then the next seed)
        n = 16
        while n <= 4096:
            c = _nseq(orc, _runs_value(s, n, False))
            if c == want:
                return _runs_value(s, n, False)
            if c > want:
                break
            n += max(1, (want - c) * 4)      # a sequence takes at least 4 bytes
    raise AssertionError(f"no runs value of seeds {seed}.. with {want} sequences")


def _check_frames(gpu, orc, vals, kernels=BATCHED):
    assert max(len(v) for v in vals) >= 512 and max(len(v) for v in vals) <= 4096   # the batched <= 4 KiB launch
    want = [orc.frame(v) for v in vals]
    got = gpu.compress_frames(vals)          # raises unless every status is 0
    import kingdb_amd as K
    assert K.last_kernels()[0] == kernels, K.last_kernels()
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, [(i, len(vals[i]), len(got[i]), len(want[i])) for i in bad[:10]]


FILL = [_runs_value(9000 + k, 600 + 7 * k, False) for k in range(8)]   # keeps every launch batched (a value >= 512 B)


def test_sequence_count_boundaries(gpu, orc):
    vals = [b"", b"x", b"hello", b"abcdefghijkl", b"a" * 12, b"a" * 13, b"abcdefghijklm", bytes(range(40))]
    assert all(_nseq(orc, v) == 0 for v in vals if len(v) < 13)
    counts = []
    for want in (1, 2, 62, 63, 64, 65, 66):
        for seed in range(12):
            v = _with_count(orc, want, 100 * want + seed)
            vals.append(v)
            counts.append(_nseq(orc, v))
    vals += [b"a" * 600, b"ab" * 700] + [_runs_value(50 + k, 4096, False) for k in range(6)]   # several flushes
    assert all(_nseq(orc, v) > 128 for v in vals[-6:])
    assert _nseq(orc, b"a" * 600) == 1
    assert {1, 63, 64, 65} <= set(counts)
    _check_frames(gpu, orc, (vals + FILL) * 4)


def test_long_literal_and_match_runs(gpu, orc):
    rng = np.random.default_rng(5)
    vals, lits, mls = [], set(), set()
    for L in list(range(58, 70)) + list(range(262, 276)) + [505, 511, 530, 700, 1200]:
        noise = rng.integers(0, 256, L, dtype=np.uint8).tobytes()
        for v in (noise + b"z" * 40, b"q" * 30 + noise + b"q" * 400, noise + (b"xyz" * 200)[:330 + L % 7]):
            vals.append(v)
            for lit, ml in _sequences(orc.compress(v)):
                lits.add(lit)
                mls.add(ml)
    vals += [b"a" * n for n in (269 + 5, 270 + 5, 271 + 5, 285, 540, 4096)] + [(b"xyz" * 1400)[:n] for n in (300, 4000)]
    for v in vals[-8:]:
        mls.update(m for _, m in _sequences(orc.compress(v)))
    assert {64, 65, 269, 270} <= lits and max(lits) > 510, sorted(lits)
    assert max(mls) >= 270 and any(270 <= m < 300 for m in mls), sorted(mls)[-5:]
    _check_frames(gpu, orc, (vals + FILL) * 3)


def test_frame_size_boundary(gpu, orc):
    rng = np.random.default_rng(6)
    vals = [rng.integers(0, 256, 4096, dtype=np.uint8).tobytes() for _ in range(40)]      # raw fallback
    assert all(orc.frame(v)[:4] == b"\0\0\0\0" and len(orc.frame(v)) == 4096 + 8 for v in vals)
    vals += [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (13, 64, 600, 4095)]
    vals += [_runs_value(300 + k, n, False) for k in range(40) for n in (4095, 4096)]
    vals += [_runs_value(400 + k, 4096, True) for k in range(40)]
    _check_frames(gpu, orc, vals * 3)


@pytest.mark.parametrize("n", [1, 3, 11, 2561])
def test_small_launches(gpu, orc, n):
    """Fewer values than waves, one more than the resident grid's waves, helpers with nothing to do."""
    vals = [_runs_value(7000 + k % 97, 512 + (k * 37) % 1500, k % 5 == 0) for k in range(n)]
    _check_frames(gpu, orc, vals)


def _child(mode):
    """Runs in a child process (the knobs are read from the environment per
    launch, but a process of its own also starts from a fresh scratch pool)."""
    import kingdb_amd as K
    import oracle
    K.set_device(0)
    orc = oracle.Oracle()
    if mode == "ring1":
        vals = [_runs_value(k % 251, 600, False) for k in range(20000)]
    else:
        vals = [_runs_value(k % 251, 600 + (k * 13) % 3400, k % 4 == 0) for k in range(3000)]
    memo = {}
    for v in vals:
        if v not in memo:
            memo[v] = orc.frame(v)
    got = K.compress_frames(vals)
    bad = [i for i, (g, v) in enumerate(zip(got, vals)) if g != memo[v]]
    print("PARITY OK" if not bad else f"PARITY FAIL {bad[:10]}", K.last_kernels())
    return 1 if bad else 0


def _run_child(mode, env):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode], env=e, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "PARITY OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


def test_ring_depth_one_child(gpu):
    """20 000 x 600 B: hand-offs arrive faster than a helper emits them, so with one
    slot per parse wave the ring-full path (the parse wave emits) runs beside the
    hand-off.  Parity only: the test cannot see which wave wrote a frame."""
    _run_child("ring1", {"KDB_LZ4_EMIT_RING": "1"})


def test_helpers_off_child(gpu):
    _run_child("off", {"KDB_LZ4_EMIT_HELPERS": "0"})


def test_back_to_back_launches(gpu, orc):
    """Two different batches on one stream, then the first again, with no host
    synchronisation between them: each launch has scratch of its own generation."""
    import kingdb_amd as K
    rng = np.random.default_rng(8)
    st = K.Stream()
    a = K.DeviceBatch.g1_long_sizes(rng.integers(512, 4097, 3000).astype(np.uint32), stream=st)
    b = K.DeviceBatch.g1_long_sizes(rng.integers(13, 4097, 2900).astype(np.uint32), first_piece=5000, stream=st)
    a.compress(st)
    b.compress(st)
    a.poison(st)
    a.compress(st)
    st.sync()
    for bt in (a, b):
        cst, _ = bt.status()
        assert (cst == 0).all(), np.flatnonzero(cst)[:10]
        src = bt.src.download(bt.raw_bytes)
        frames = bt.frames.download()
        flen = bt.frame_lens()
        for i in range(bt.n):
            v = src[int(bt.src_off[i]):int(bt.src_off[i]) + int(bt.sizes[i])].tobytes()
            f = frames[int(bt.frame_off[i]):int(bt.frame_off[i]) + int(flen[i])].tobytes()
            assert f == orc.frame(v), (i, len(v), int(flen[i]))
        bt.free()


def test_blocks_entry_point(gpu, orc):
    """compress_blocks: caps >= the bound take the kFrame = false batched kernel
    (hand-off, the helper writes the block size); a cap below the bound takes the
    guard path, which never hands off."""
    import kingdb_amd as K
    vals = [_runs_value(600 + k, 512 + (k * 29) % 3585, k % 3 == 0) for k in range(700)]
    vals += [b"a" * 4096, np.random.default_rng(9).integers(0, 256, 4096, dtype=np.uint8).tobytes()]
    want = [orc.compress(v) for v in vals]
    got = gpu.compress_blocks(vals)
    assert K.last_kernels()[0] == BATCHED_BLOCKS, K.last_kernels()
    for i, ((r, blk), w) in enumerate(zip(got, want)):
        assert r == len(w) and blk == w, (i, r, len(w))
    # every third value with a cap below the bound (some fit, some fail): the guard path
    caps = [orc.compress_bound(len(v)) if i % 3 else max(len(w) - (i % 2) * 7, 1)
            for i, (v, w) in enumerate(zip(vals, want))]
    got = gpu.compress_blocks(vals, caps=caps)
    for i, ((r, blk), v, c) in enumerate(zip(got, vals, caps)):
        w = orc.compress(v, c)
        assert r == (len(w) if w else 0), (i, r, c)
        if w:
            assert blk == w, (i, c)


if __name__ == "__main__":
    sys.exit(_child(sys.argv[1]))

"""A/B timing of library builds on the headline batch, with a correctness gate.

    python tools/ab.py <lib.so> [--mixed] [--text 4096:65536] [--reps 5]

Loads the given libkdb_lz4 build (e.g. kingdb_amd/var/var_<name>.so from
tools/build_variants.sh, or the in-tree library), compresses and decompresses
the 1 Mi x 4 KiB G1-long batch (and with --mixed the 1 Mi mixed batch), times
each kernel pass with HIP events (min and median of --reps), and checks the
frame stream against tests/golden/digests.json (length + CRC32C of the packed
frames) and the round trip: a build whose output differs prints FAIL.

--text SIZE:N adds a seeded batch of Zipf-distributed random words (round-trip
gate only).  For the headline batch and the text batch the tool also prints the
share of consecutive sequences of a value whose match length repeats, from the
oracle's parse of a few hundred values: the rate at which a parse that guesses
a match's end from the value's previous match
guesses right, i.e. how regular the batch is.  (The emitted length, catch-up
included, stands for the forward length such a parse compares; the two differ
only where a match was extended backwards.)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def match_lengths(block):
    """The match lengths of an LZ4 block's sequences, in order."""
    i, out, n = 0, [], len(block)
    while i < n:
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
        if i >= n:
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


def repeat_rate(orc, values):
    """(sequences per value, share of consecutive sequences with equal match length)."""
    seqs = pairs = same = 0
    for v in values:
        m = match_lengths(orc.compress(v))
        seqs += len(m)
        pairs += max(len(m) - 1, 0)
        same += sum(1 for a, b in zip(m, m[1:]) if a == b)
    return seqs / max(len(values), 1), same / max(pairs, 1)


def zipf_text(nbytes, seed=301, vocab=4096, pool_bytes=1 << 25):
    """nbytes of space-separated random lower-case words (2-10 letters), drawn
    from a vocabulary of `vocab` words with Zipf(1.1) frequencies.  A pool of
    pool_bytes is generated and repeated, each copy rotated by another odd
    offset, so equal 4 KiB values do not recur at equal alignment."""
    rng = np.random.default_rng(seed)
    wl = rng.integers(2, 11, vocab).astype(np.int32) + 1              # with the space
    words = rng.integers(ord("a"), ord("z") + 1, (vocab, 11)).astype(np.uint8)
    words[np.arange(vocab), wl - 1] = ord(" ")
    pool_bytes = min(pool_bytes, nbytes)
    nw = pool_bytes // 3 + 1
    idx = np.minimum(rng.zipf(1.1, nw) - 1, vocab - 1).astype(np.int32)
    lens = wl[idx]
    ends = np.cumsum(lens, dtype=np.int64)
    k = int(np.searchsorted(ends, pool_bytes)) + 1
    idx, lens, ends = idx[:k], lens[:k], ends[:k]
    wid = np.repeat(idx, lens)
    pos = (np.arange(len(wid), dtype=np.int64) - np.repeat(ends - lens, lens)).astype(np.int32)
    pool = words[wid, pos][:pool_bytes]
    reps = -(-nbytes // pool_bytes)
    return np.concatenate([np.roll(pool, -1237 * r) for r in range(reps)])[:nbytes]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("so")
    ap.add_argument("--mixed", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--uniform", action="append", default=[],
                    help="SIZE:N extra uniform batch (round-trip gate only, no digest)")
    ap.add_argument("--text", action="append", default=[],
                    help="SIZE:N extra batch of seeded Zipf-distributed random words (round-trip gate only)")
    ap.add_argument("--no-headline", action="store_true")
    ap.add_argument("--exact-max-in", action="store_true",
                    help="decompress told the batch's largest frame (not the slot bound)")
    ap.add_argument("--compress-only", action="store_true",
                    help="time the compress pass alone: no decompress, no digest, no round trip "
                         "(for a timing-only build whose frames are wrong on purpose)")
    a = ap.parse_args()
    from kingdb_amd import _lib
    _lib.load(os.path.abspath(a.so))
    import kingdb_amd as K
    from kingdb_amd.lz4 import DeviceBuffer, lib, mixed_sizes
    import oracle
    orc = oracle.Oracle()
    K.set_device(0)
    dig = json.load(open(os.path.join(ROOT, "tests", "golden", "digests.json")))
    work = [] if a.no_headline else [("g1_long_4k", np.full(1 << 20, 4096, np.uint32))]
    if a.mixed:
        work.append(("mixed_1m", mixed_sizes(1 << 20)))
    for u in a.uniform:
        sz, cnt = (int(x) for x in u.split(":"))
        work.append((f"u{sz}x{cnt}", np.full(cnt, sz, np.uint32)))
    for t in a.text:
        sz, cnt = (int(x) for x in t.split(":"))
        work.append((f"text{sz}x{cnt}", (sz, cnt)))
    for name, sizes in work:
        if name.startswith("text"):
            sz, cnt = sizes
            host = zipf_text(sz * cnt)
            b = K.DeviceBatch.from_host(host, sz)
            sample = [host[i * sz:(i + 1) * sz].tobytes() for i in range(0, cnt, max(cnt // 256, 1))][:256]
        else:
            b = K.DeviceBatch.g1_long_sizes(sizes)
            sample = None
            if name == "g1_long_4k":
                sample = oracle.g1_values(oracle.g1_pool(orc, 512 * 4096), 4096, 512)
        if sample:
            spv, rate = repeat_rate(orc, sample)
            print(f"{'':24s} {name:10s} oracle parse of {len(sample)} values: {spv:.1f} sequences per value, "
                  f"{100 * rate:.1f} % of consecutive sequences repeat their match length", flush=True)
        st = K.Stream()
        b.exact_max_in = a.exact_max_in
        if a.compress_only:
            b.compress(st)
            st.sync()
            e = [K.Event() for _ in range(2)]
            cs = []
            for _ in range(a.reps):
                e[0].record(st)
                b.compress(st)
                e[1].record(st)
                cs.append(e[0].elapsed_ms(e[1]))
            print(f"{os.path.basename(a.so):24s} {name:10s} compress min {min(cs):7.3f} med {np.median(cs):7.3f} "
                  f"max {max(cs):7.3f} ms  reps {' '.join(f'{c:.3f}' for c in cs)}  (compress only, not checked)",
                  flush=True)
            b.free()
            continue
        b.compress(st)
        b.decompress(st)
        st.sync()
        e = [K.Event() for _ in range(3)]
        cs, ds = [], []
        for _ in range(a.reps):
            e[0].record(st)
            b.compress(st)
            e[1].record(st)
            b.decompress(st)
            e[2].record(st)
            cs.append(e[0].elapsed_ms(e[1]))
            ds.append(e[1].elapsed_ms(e[2]))
        dense, doff, tot = DeviceBuffer(b.frames.nbytes), DeviceBuffer(8 * b.n), DeviceBuffer(8)
        _lib.check(lib().kdb_lz4_pack_frames(None, b.frames.ptr, b._p(2), b._p(3), b.n, dense.ptr, doff.ptr,
                                             tot.ptr), "pack")
        total = int(tot.download(8).view(np.uint64)[0])
        crc = orc.crc32c_array(dense.download(total))
        g = dig.get(name)
        ok = (g is None or (total == g["frame_bytes"] and f"0x{crc:08x}" == g["frames_crc32c"])) and b.roundtrip_ok()
        rt = b.raw_bytes / 2**30 / ((np.median(cs) + np.median(ds)) / 1e3)
        print(f"{os.path.basename(a.so):24s} {name:10s} compress min {min(cs):7.3f} med {np.median(cs):7.3f} "
              f"max {max(cs):7.3f} ms  "
              f"decompress min {min(ds):6.3f} med {np.median(ds):6.3f} ms  round trip {rt:6.1f} GiB/s  "
              f"{'OK' if ok else 'FAIL'}", flush=True)
        b.free()


if __name__ == "__main__":
    main()

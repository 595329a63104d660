"""LZ4 blocks built sequence by sequence (no GPU, no C): a third reference for
the decoder, independent of the oracle (oracle/lz4_oracle.c) and of the
reference's own C.

Every other block the suite decodes comes from one compressor's parse.  The
decoders' fast paths (kingdb_amd/csrc/lz4_decompress.hip: decode_block over
LDS, decode_ring over the two rings) branch on properties of a single
sequence -- its literal count, its match length, its offset, how far it is
from the two ends, where its bytes fall in the input ring -- and a parser
does not choose where those fall.  Here a block is written from a list of
``(literal bytes, offset, match length)`` and the final literal run, so a
sequence can be put exactly on each boundary.

* ``encode``       block bytes + the decoded bytes (byte-by-byte copy rule).
* ``well_formed``  the precise meaning of "decodes to ``decoded``" for this
                   decoder (LZ4 r1.3.0's LZ4_decompress_safe_partial).
* ``classify``     per sequence, which side of every fast-path condition it is
                   on; written from the format's rules, not from the kernel.
* ``tally`` / ``REQUIRED_*``  the counts the tests assert (they prove that a
                   set reaches what it claims).
* seeded generators, the deterministic offset sweep, the constructed ring
  refill straddles, the ill-formed classes, and the sets of the GPU tests
  (``set_a`` .. ``set_e``, ``service_cases``).
"""
from __future__ import annotations

import functools
import random
from collections import Counter, namedtuple

MINMATCH, LASTLITERALS, MFLIMIT = 4, 5, 12

# name; block bytes; output size handed to the decoder; the builder's decoded
# bytes (None: ill-formed, the oracle's result is the expectation); the
# sequences and the last run it was built from (None where built from raw
# bytes); kind: "random", "sweep", "far", "straddle", "long", "ill".
Case = namedtuple("Case", "name block size decoded seqs last kind")


# ------------------------------------------------------------------ builder
def _length_bytes(n: int) -> bytes:
    """The 255-chain of a length whose nibble is 15: n = value - 15."""
    out = bytearray()
    while n >= 255:
        out.append(255)
        n -= 255
    out.append(n)
    return bytes(out)


def encode_sequence(lits: bytes, off: int, mlen: int) -> bytes:
    ll, ml = len(lits), mlen - MINMATCH
    assert ml >= 0 and 0 <= off <= 0xFFFF
    out = bytearray([(min(ll, 15) << 4) | min(ml, 15)])
    if ll >= 15:
        out += _length_bytes(ll - 15)
    out += lits
    out += bytes([off & 0xFF, off >> 8])
    if ml >= 15:
        out += _length_bytes(ml - 15)
    return bytes(out)


def encode_last(last: bytes) -> bytes:
    ll = len(last)
    out = bytearray([min(ll, 15) << 4])
    if ll >= 15:
        out += _length_bytes(ll - 15)
    return bytes(out + last)


def encode(seqs, last: bytes):
    """(block, decoded) of sequences [(literal bytes, offset, match length)] and
    the final literal run.  A match copies byte by byte from `offset` back; a
    source byte that does not exist (offset 0 or past the start: an ill-formed
    block) reads as 0 here and makes `decoded` meaningless."""
    block, out = bytearray(), bytearray()
    for lits, off, mlen in seqs:
        block += encode_sequence(lits, off, mlen)
        out += lits
        if off >= mlen and off <= len(out):
            s = len(out) - off
            out += out[s:s + mlen]          # no overlap: the same bytes as the loop below
        else:
            for _ in range(mlen):
                out.append(out[-off] if 0 < off <= len(out) else 0)
    block += encode_last(last)
    out += last
    return bytes(block), bytes(out)


def well_formed(seqs, last: bytes, size: int) -> bool:
    """A block of `seqs` + `last` decodes to encode()'s bytes with output size
    `size` iff every match-bearing sequence's literals end at output position
    <= size - 12 (else the decoder takes them for the last run), every match
    ends at <= size - 5, 1 <= offset <= the output produced so far, and the
    last run ends exactly at `size` (encode() ends it exactly at the block's
    end).  A match end <= size - 5 leaves >= 5 last literals, so the input-side
    rule (literals end at <= block size - 8) follows."""
    op = 0
    for lits, off, mlen in seqs:
        op += len(lits)
        if op > size - MFLIMIT or not 1 <= off <= op or mlen < MINMATCH:
            return False
        op += mlen
        if op > size - LASTLITERALS:
            return False
    return op + len(last) == size and size > 0


def case_from(name, seqs, last, kind="random", size=None) -> Case:
    block, decoded = encode(seqs, last)
    size = len(decoded) if size is None else size
    ok = well_formed(seqs, last, size)
    return Case(name, block, size, decoded if ok else None, list(seqs), last, kind)


# ----------------------------------------------------------------- classify
LIT_EDGES = (0, 14, 15, 60, 61, 269, 270)          # nibble | one byte <= 45 | one byte > 45 | chain
ML_EDGES = (4, 18, 19, 64, 65, 273, 274)           # nibble | one byte <= 254 | chain; one 64-byte step | more
OFF_EDGES = (1, 63, 64, 65, 4031, 4032, 4033, 4095, 4096, 4097)
RING_FAR = 4096 - 64                               # the ring decoder's fast path: off <= kORing - 64


def classify(seqs, size: int, csize: int):
    """One dict per sequence: its fields, its byte positions in the block, and
    the side of each fast-path condition it falls on (full-size target).

      lit_class   "nibble" (<= 14) | "byte<=45" (15..60) | "byte>45" (61..269) | "chain" (>= 270)
      ml_class    "nibble" (<= 18) | "byte<=254" (19..273) | "chain" (>= 274)
      off_class   "periodic" (off < min(mlen, 64)) | "near" (<= 4032) | "far" (> 4032)
      steps       "one" (mlen <= 64) | "many"
      nt          the lane of the next token in the literal load, lit + 2 + (1 if
                  a match-length byte follows), for sequences of the first two
                  literal and match classes (at most 63); else None
      out_not_last / match_fits / in_not_last   the reference's own conditions
                  (literals end <= size - 12, match end <= size - 5, literals
                  end in the block <= csize - 8)
      far_ip / far_op   the ring decoder's coarser bounds: token at <= csize - 8
                  - 62, output position <= min(size - 12 - 60, size - 5 - 60 - 273)
      block_fast / ring_fast   every condition of that decoder's fast loop
      tok_ip, litlen_ip (first, last+1), lit_ip, off_ip, mllen_ip (first, last+1),
      end_ip      input positions; straddle[B] for B in (2048, 4096) names what
                  lies across a multiple of B: "token_last" (the token is the
                  last byte before it), "token_first" (the first after it),
                  "offset" (its two bytes on both sides), "lit_chain",
                  "ml_chain" (length bytes on both sides), "literals" (a literal
                  run copied in pieces)."""
    res = []
    ip = op = 0
    for lits, off, mlen in seqs:
        lit = len(lits)
        tok_ip = ip
        nl = len(_length_bytes(lit - 15)) if lit >= 15 else 0
        nm = len(_length_bytes(mlen - MINMATCH - 15)) if mlen - MINMATCH >= 15 else 0
        lit_ip = tok_ip + 1 + nl
        off_ip = lit_ip + lit
        ml_ip = off_ip + 2
        end_ip = ml_ip + nm
        lit_end, match_end = op + lit, op + lit + mlen
        c = {
            "lit": lit, "mlen": mlen, "off": off, "op": op, "lit_end": lit_end, "match_end": match_end,
            "tok_ip": tok_ip, "litlen_ip": (tok_ip + 1, lit_ip), "lit_ip": lit_ip, "off_ip": off_ip,
            "mllen_ip": (ml_ip, end_ip), "end_ip": end_ip,
            "lit_class": "nibble" if lit <= 14 else "byte<=45" if lit <= 60 else "byte>45" if lit <= 269 else "chain",
            "ml_class": "nibble" if mlen <= 18 else "byte<=254" if mlen <= 273 else "chain",
            "off_class": "periodic" if off < min(mlen, 64) else "near" if off <= RING_FAR else "far",
            "steps": "one" if mlen <= 64 else "many",
            "out_not_last": lit_end <= size - MFLIMIT,
            "match_fits": match_end <= size - LASTLITERALS,
            "in_not_last": off_ip <= csize - 8,
            "far_ip": tok_ip <= csize - 8 - 62,
            "far_op": op <= min(size - MFLIMIT - 60, size - LASTLITERALS - 60 - 273),
        }
        c["nt"] = lit + 2 + (1 if nm else 0) if lit <= 60 and mlen <= 273 else None
        ok = (c["nt"] is not None and c["out_not_last"] and c["match_fits"] and c["in_not_last"]
              and 0 <= off <= lit_end)
        c["block_fast"] = ok
        c["ring_fast"] = ok and c["far_ip"] and c["far_op"] and off <= RING_FAR
        strad = {}
        for B in (2048, 4096):
            s = set()
            if tok_ip % B == B - 1:
                s.add("token_last")
            if tok_ip % B == 0 and tok_ip > 0:
                s.add("token_first")
            if off_ip % B == B - 1:
                s.add("offset")
            if nl >= 2 and (tok_ip + 1) // B != (lit_ip - 1) // B:
                s.add("lit_chain")
            if nm >= 2 and ml_ip // B != (end_ip - 1) // B:
                s.add("ml_chain")
            if lit >= 2 and lit_ip // B != (off_ip - 1) // B:
                s.add("literals")
            strad[B] = s
        c["straddle"] = strad
        res.append(c)
        ip, op = end_ip, match_end
    return res


def tally(cases, counter: Counter | None = None, min_op: int = 0) -> Counter:
    """Counts, over the sequences of the well-formed cases, of each boundary
    value and each side of each condition (the keys of REQUIRED_*)."""
    n = Counter() if counter is None else counter
    for cs in cases:
        if cs.decoded is None or cs.seqs is None:
            continue
        for c in classify(cs.seqs, cs.size, len(cs.block)):
            if c["op"] < min_op:
                continue
            if c["lit"] in LIT_EDGES:
                n["lit=%d" % c["lit"]] += 1
            if c["mlen"] in ML_EDGES:
                n["ml=%d" % c["mlen"]] += 1
            if c["off"] in OFF_EDGES:
                n["off=%d" % c["off"]] += 1
            if -1 <= c["off"] - c["mlen"] <= 1 and c["mlen"] <= 65:
                n["off-ml=%d" % (c["off"] - c["mlen"])] += 1
            n["lit:" + c["lit_class"]] += 1
            n["ml:" + c["ml_class"]] += 1
            n["off:" + c["off_class"]] += 1
            n["steps:" + c["steps"]] += 1
            if c["nt"] is not None and c["nt"] >= 62:
                n["nt=%d" % c["nt"]] += 1
            n["lit_end=size-12" if c["lit_end"] == cs.size - 12 else "lit_end<size-12"] += 1
            n["match_end=size-5" if c["match_end"] == cs.size - 5 else "match_end<size-5"] += 1
            n["ip_lit_end=csize-8" if c["off_ip"] == len(cs.block) - 8 else "ip_lit_end<csize-8"] += 1
            n["far_ip:in" if c["far_ip"] else "far_ip:out"] += 1
            n["far_op:in" if c["far_op"] else "far_op:out"] += 1
            n["block_fast:yes" if c["block_fast"] else "block_fast:no"] += 1
            n["ring_fast:yes" if c["ring_fast"] else "ring_fast:no"] += 1
            if c["off"] > RING_FAR and c["lit"] == 0:
                n["far,lit=0,ml=%d" % c["mlen"]] += 1
            for B, s in c["straddle"].items():
                for k in s:
                    n["straddle%d:%s" % (B, k)] += 1
    return n


# The boundaries of decode_block's fast loop (at least 20 sequences on each side
# of each, asserted per set by the tests): literal-length byte 45|46 (lit
# 60|61), none|one (14|15), one|chain (269|270); match-length byte none|one
# (18|19), 254|255 (273|274), one 64-byte step|more (64|65); offset against the
# match length (mlen - 1, mlen, mlen + 1) and against a step (63|64); the next
# token's lane 62|63; the two ends, exactly on them and inside.
REQUIRED_BLOCK = (
    ["lit=%d" % v for v in LIT_EDGES] + ["ml=%d" % v for v in ML_EDGES] +
    ["off=1", "off=63", "off=64", "off=65", "off-ml=-1", "off-ml=0", "off-ml=1",
     "lit:nibble", "lit:byte<=45", "lit:byte>45", "lit:chain", "ml:nibble", "ml:byte<=254", "ml:chain",
     "off:periodic", "off:near", "steps:one", "steps:many", "nt=62", "nt=63",
     "lit_end=size-12", "lit_end<size-12", "match_end=size-5", "match_end<size-5",
     "ip_lit_end=csize-8", "ip_lit_end<csize-8", "block_fast:yes", "block_fast:no"])
# decode_ring in addition: offset 4032|4033 and the ring's size 4096|4097, its
# coarser distance to the two ends, a sequence in and out of its fast loop.
REQUIRED_RING = REQUIRED_BLOCK + [
    "off=4031", "off=4032", "off=4033", "off=4095", "off=4096", "off=4097", "off:far",
    "far_ip:in", "far_ip:out", "far_op:in", "far_op:out", "ring_fast:yes", "ring_fast:no"]
STRADDLE_KINDS = ("token_last", "token_first", "offset", "lit_chain", "ml_chain", "literals")


# --------------------------------------------------------------- generators
LIT_LIST = [0, 1, 14, 15, 16, 44, 45, 46, 59, 60, 61, 62, 63, 64, 65, 269, 270, 271, 524, 525, 526]
ML_LIST = [4, 5, 18, 19, 20, 63, 64, 65, 66, 127, 128, 129, 272, 273, 274, 275, 527, 528, 529, 530, 1000]
OFF_LIST = list(range(1, 67)) + [127, 128, 255, 256, 257, 4031, 4032, 4033, 4095, 4096, 4097, 8191, 8192, 8193,
                                 65535]
# the values the fast loops turn on, drawn more often than the rest of the lists
LIT_HOT = [0, 0, 0, 14, 15, 59, 60, 60, 61, 269, 270]
ML_HOT = [4, 18, 19, 64, 65, 273, 274]
LIT_DENSE = [0, 14, 14, 15, 15, 59, 60, 60, 61, 61, 269, 270]
ML_DENSE = [4, 4, 18, 18, 19, 19, 64, 64, 65, 65, 273, 274]
OFF_HOT = [1, 63, 64, 65]
OFF_HOT_RING = [4031, 4032, 4033, 4095, 4096, 4097]


def _draw(rng, hot, lst, lo, hi, cap, dense=False):
    """A value <= cap: 30 % from `hot`, 40 % from `lst` (70 % from the boundary
    lists in all; dense: 80 % and 10 %), the rest uniform in lo..hi; None if
    nothing fits."""
    ph, pl = (0.80, 0.90) if dense else (0.30, 0.70)
    for _ in range(8):
        r = rng.random()
        v = rng.choice(hot) if r < ph else rng.choice(lst) if r < pl else rng.randint(lo, hi)
        if v <= cap:
            return v
    return lo if lo <= cap else None


def random_block(rng: random.Random, size: int, name: str, ring: bool = False, rare: bool = False,
                 head=(), exact_end: bool = False, dense: bool = False) -> Case:
    """A well-formed block of exactly `size` output bytes.  ring: the offsets
    around 4 032 and 4 096 are drawn more often; rare: the runs of 2 100 and
    5 000 literals and the match of 5 000 may be drawn; head: sequences the
    block starts with; exact_end: the last sequence's literals end exactly at
    size - 12 and its match at size - 5; dense: for a set of few blocks, the
    values the fast loops turn on are drawn 80 % of the time and the last 420
    output bytes are short sequences, so that many lie past the ring decoder's
    coarse end bounds."""
    assert size >= 1
    seqs = list(head)
    op = sum(len(s[0]) + s[2] for s in seqs)
    while True:
        room_lit = size - MFLIMIT - op                    # literals may end at <= size - 12
        if room_lit < (1 if op == 0 else 0) or (size <= 300 and rng.random() < 0.03):
            break
        tail = dense and room_lit < 420
        if tail:
            lit = rng.randint(0, min(3, room_lit))
        else:
            lit = _draw(rng, LIT_DENSE if dense else LIT_HOT, LIT_LIST, 0, 70, room_lit, dense)
        if rare and rng.random() < 0.03 and room_lit >= 2100:
            lit = 5000 if room_lit >= 5000 and rng.random() < 0.5 else 2100
        if lit is None:
            break
        if op == 0 and lit == 0:
            lit = 1
        room_ml = size - LASTLITERALS - op - lit           # the match may end at <= size - 5
        if room_ml < MINMATCH:
            break
        r = rng.random()
        if (r < 0.14 or exact_end) and (op > 0 or room_lit > 0) and room_lit <= (12 if exact_end else 600):
            # the last sequence, its literals ending exactly at size - 12; a match
            # of 7 then ends exactly at size - 5 and leaves 5 last literals, so
            # the literals also end exactly at csize - 8
            lit, mlen = room_lit, 7 if exact_end else rng.choice([4, 5, 6, 7, 7, 7, 7, 7, 7])
        elif r < 0.16 and room_ml <= 1200 and not exact_end:
            mlen = room_ml                                  # the match ends exactly at size - 5
        else:
            if tail:
                mlen = rng.randint(4, min(8, room_ml))
            else:
                mlen = _draw(rng, ML_DENSE if dense else ML_HOT, ML_LIST, MINMATCH, 80, room_ml, dense)
            if rare and rng.random() < 0.02 and room_ml >= 5000:
                mlen = 5000
            if mlen is None or mlen < MINMATCH:
                break
        p = op + lit
        r = rng.random()
        cand = [o for o in (mlen - 1, mlen, mlen + 1) if 1 <= o <= p]
        if r < 0.22 and cand:
            off = rng.choice(cand)
        else:
            hot = OFF_HOT * (3 if dense else 1) + (OFF_HOT_RING * (3 if dense else 2) if ring else [])
            off = _draw(rng, hot, OFF_LIST, 1, min(p, 300), p, dense)
        seqs.append((rng.randbytes(lit), off, mlen))
        op = p + mlen
    last = size - op
    cs = case_from(name, seqs, rng.randbytes(last), "random")
    assert cs.decoded is not None and cs.size == size, (name, size)
    return cs


def _fill(rng, n):
    return rng.randbytes(n)


def _lead(rng, pos_next_token: int, cur_ip: int, op: int):
    """A sequence (L literals, a 4-byte match) after which the next token sits at
    input position `pos_next_token`: 1 + length bytes + L + 2 = the distance."""
    d = pos_next_token - cur_ip
    for L in range(max(d - 40, 0), d):
        nl = len(_length_bytes(L - 15)) if L >= 15 else 0
        if 1 + nl + L + 2 == d and (op + L) >= 1:
            return (_fill(rng, L), min(op + L, 7) or 1, 4)
    raise AssertionError("no leading run reaches %d from %d" % (pos_next_token, cur_ip))


def straddle_seqs(rng: random.Random, kinds, nbound: int, step: int = 2048) -> list:
    """Sequences that place kinds[(k - 1) % len(kinds)] across input position
    step * k for k = 1 .. nbound (with 2 048, every second one is a multiple of
    4 096), by leading literal runs of the right length (the builder knows
    every byte position)."""
    seqs, ip, op = [], 0, 0
    for k in range(1, nbound + 1):
        edge = step * k
        kind = kinds[(k - 1) % len(kinds)]
        # the input position of the token of the sequence that carries the straddle
        if kind == "token_last":
            tok, s = edge - 1, (_fill(rng, 20), 9, 30)
        elif kind == "token_first":
            tok, s = edge, (_fill(rng, 20), 9, 30)
        elif kind == "offset":
            tok, s = edge - 5, (_fill(rng, 3), 11, 30)           # token, 3 literals, offset low | high
        elif kind == "lit_chain":
            tok, s = edge - 2, (_fill(rng, 600), 300, 30)        # token, 255 | 255, 75
        elif kind == "ml_chain":
            tok, s = edge - 4, (b"", 40, 600)                    # token, offset, 255 | 255, 71
        else:
            raise ValueError(kind)
        lead = _lead(rng, tok, ip, op)
        for q in (lead, s):
            seqs.append(q)
            ip += len(encode_sequence(*q))
            op += len(q[0]) + q[2]
    return seqs


def straddle_block(rng: random.Random, kind: str, nbound: int, name: str) -> Case:
    cs = case_from(name, straddle_seqs(rng, [kind], nbound), _fill(rng, 40), "straddle")
    assert cs.decoded is not None
    return cs


SWEEP_MLENS = (None, 64, 65, 130, 300)     # None: max(4, off + 1)


def sweep_pairs():
    return [(off, max(4, off + 1) if m is None else m) for off in range(1, 64) for m in SWEEP_MLENS]


def sweep_blocks(rng: random.Random, max_out: int, prefix: int, tag: str) -> list:
    """The deterministic offset sweep: each offset 1..63 with match lengths
    max(4, off + 1), 64, 65, 130 and 300, each (a) directly after a match
    (0 literals), (b) with 0 literals as the sequence after one of 60 literals
    and a match-length byte (its token is the one read on lane 63) and (c)
    carrying 60 literals itself.  `prefix` incompressible bytes lead every
    block (the ring decoders' sweep runs past output position 4 096, on a
    wrapped ring); blocks are cut at `max_out` output bytes."""
    out, seqs, op = [], [], 0

    def start():
        nonlocal seqs, op
        seqs = [(_fill(rng, max(prefix, 70)), 33, 8)]
        op = max(prefix, 70) + 8

    def cut():
        out.append(case_from("%s_sweep%d" % (tag, len(out)), seqs, _fill(rng, 12), "sweep"))
        assert out[-1].decoded is not None

    start()
    for off, mlen in sweep_pairs():
        group = [(_fill(rng, 60), 70, 20), (b"", off, mlen),         # (b): token on lane 63
                 (b"", off, mlen),                                   # (a): follows a match
                 (_fill(rng, 60), off, mlen)]                        # (c)
        need = sum(len(s[0]) + s[2] for s in group)
        if op + need + 12 > max_out:
            cut()
            start()
        seqs += group
        op += need
    cut()
    return out


def sweep_seen(cases, min_op: int = 0) -> dict:
    """{(off, mlen): set of "a"/"b"/"c"} over the sweep cases (from classify)."""
    seen = {}
    for cs in cases:
        if cs.kind != "sweep":
            continue
        cl = classify(cs.seqs, cs.size, len(cs.block))
        for i, c in enumerate(cl):
            if i == 0 or c["op"] < min_op:
                continue
            prev = cl[i - 1]
            if c["lit"] == 0 and prev["nt"] == 63:
                seen.setdefault((c["off"], c["mlen"]), set()).add("b")
            elif c["lit"] == 0:
                seen.setdefault((c["off"], c["mlen"]), set()).add("a")
            elif c["lit"] == 60:
                seen.setdefault((c["off"], c["mlen"]), set()).add("c")
    return seen


FAR_OFFS = (4031, 4032, 4033, 4095, 4096, 4097)
FAR_MLENS = (4, 64, 65, 300)


def far_block(rng: random.Random, name: str) -> Case:
    """Matches from 4 031 .. 4 097 back (the ring decoder's fast-path bound and
    the output ring's size), each after 0 literals, with match lengths 4, 64,
    65 and 300."""
    seqs = [(_fill(rng, 4300), 100, 6)]
    for off in FAR_OFFS:
        for m in FAR_MLENS:
            seqs.append((b"", off, m))
    cs = case_from(name, seqs, _fill(rng, 400), "far")
    assert cs.decoded is not None
    return cs


def long_block(rng: random.Random, name: str, lits=(2100, 5000), mlens=(5000,), lead: int = 200) -> Case:
    """Long literal runs (2 100 and 5 000 bytes) and a match of 5 000."""
    seqs = [(_fill(rng, lead), 17, 40)]
    for n in lits:
        seqs.append((_fill(rng, n), 300, 20))
    for m in mlens:
        seqs.append((_fill(rng, 3), 150, m))
    cs = case_from(name, seqs, _fill(rng, 30), "long")
    assert cs.decoded is not None
    return cs


# --------------------------------------------------------------- ill-formed
ILL_CLASSES = ("off_past_start", "match_first", "match_ends_size-4", "lit_past_size", "lit_past_block",
               "litlen_chain_cut", "mllen_chain_in_last5", "size-1", "size+1", "lits_end_past_size-12")


def ill_formed(rng: random.Random, big: bool, tag: str) -> list:
    """One defect per block, at sequence granularity.  big: about 10 000 output
    bytes (the ring decoders take it); else under 300."""
    def body():
        # a well-formed start: `n` output bytes of sequences
        n = 9800 if big else rng.randint(60, 180)
        seqs = []
        while len(seqs) < 2:
            seqs = list(random_block(rng, n + 40, "x", ring=big).seqs)
        op = sum(len(s[0]) + s[2] for s in seqs)
        return seqs, op

    out = []

    def add(cls, seqs, last, size=None, block=None):
        blk, dec = encode(seqs, last)
        out.append(Case("%s_%s" % (tag, cls), blk if block is None else block, len(dec) if size is None else size,
                        None, None, None, "ill"))

    seqs, op = body()
    add("off_past_start", seqs + [(_fill(rng, 5), op + 5 + 1, 20)], _fill(rng, 20))
    seqs, op = body()
    add("match_first", [(b"", 1, 8)] + seqs, _fill(rng, 20))
    seqs, op = body()
    add("match_ends_size-4", seqs + [(_fill(rng, 9), 3, 30)], _fill(rng, 4))
    seqs, op = body()
    mid = len(seqs) * 4 // 5 if big else len(seqs) // 2
    cut = sum(len(s[0]) + s[2] for s in seqs[:mid]) + len(seqs[mid][0])
    add("lit_past_size", seqs, _fill(rng, 20), size=max(cut - 1, 1))
    seqs, op = body()
    blk, dec = encode(seqs, _fill(rng, 20))
    add("lit_past_block", seqs, b"", size=len(dec), block=blk[:-1])
    seqs, op = body()
    blk, dec = encode(seqs, b"")
    add("litlen_chain_cut", seqs, b"", size=len(dec) + 600, block=blk[:-1] + bytes([0xF0]) + b"\xff" * 20)
    seqs, op = body()
    blk, dec = encode(seqs, b"")
    add("mllen_chain_in_last5", seqs, b"", size=len(dec) + 2000,
        block=blk[:-1] + bytes([0x1F, 0x41, 2, 0]) + b"\xff" * 8)
    seqs, op = body()
    blk, dec = encode(seqs, _fill(rng, 20))
    add("size-1", seqs, b"", size=len(dec) - 1, block=blk)
    add("size+1", seqs, b"", size=len(dec) + 1, block=blk)
    # literals that end past size - 12 before a match: both decoders take them
    # for the last run and return their end (32 of the 41-byte case)
    seqs, op = body()
    add("lits_end_past_size-12", seqs + [(_fill(rng, 32), 7, 4)], _fill(rng, 5))
    return out


def ill_fixed() -> list:
    """size = 0 with the blocks `00` and `10 41`, and the 41-byte block of 32
    literals, a 4-byte match and 5 last literals (returns 32)."""
    b41, d41 = encode([(bytes(range(65, 97)), 7, 4)], b"vwxyz")
    assert len(d41) == 41
    return [Case("size0_00", b"\x00", 0, None, None, None, "ill"),
            Case("size0_10_41", b"\x10\x41", 0, None, None, None, "ill"),
            Case("b41", b41, 41, None, None, None, "ill")]


# --------------------------------------------------------------------- sets
def targets_for(size: int) -> list:
    return [1, 64, size // 3, size - 13, size - 1]


def target_of(c: Case) -> int:
    """The partial target the GPU tests give a case (one of targets_for, picked
    by the case itself so that it is the same in every set that holds it)."""
    return targets_for(c.size)[(c.size + len(c.block)) % 5]


@functools.lru_cache(maxsize=None)
def set_a() -> tuple:
    """lz4_decompress_kernel<false, 3u>: outputs 20 .. 2 900 bytes, blocks <= 3 057."""
    rng = random.Random(0xA)
    cases = []
    for i in range(1250):
        size = rng.randint(20, 300) if rng.random() < 0.25 else rng.randint(300, 2900)
        cases.append(random_block(rng, size, "a%d" % i))
    cases.append(long_block(rng, "a_long2100", lits=(2100,), mlens=(), lead=100))
    cases += sweep_blocks(rng, 2900, 0, "a")
    for k in range(3):
        cases += ill_formed(rng, False, "a_ill%d" % k)
    cases += ill_fixed()
    assert all(len(c.block) <= 3057 and c.size <= 2900 for c in cases)
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def set_b_extra() -> tuple:
    rng = random.Random(0xB)
    cases = [random_block(rng, rng.randint(2901, 8192), "b%d" % i, rare=True) for i in range(150)]
    cases.append(random_block(rng, 8192, "b_8192", rare=True))
    cases.append(case_from("b_literals8192", [], rng.randbytes(8192), "long"))
    cases.append(long_block(rng, "b_long", lits=(2100, 5000), mlens=()))
    cases.append(long_block(rng, "b_match5000", lits=(), mlens=(5000,)))
    assert all(c.size <= 8192 for c in cases) and len(cases[-3].block) > 8192
    return tuple(cases)


def set_b() -> tuple:
    """lz4_decompress_kernel<false, 5u>: set (a) plus blocks up to 8 192 bytes of output."""
    return set_a() + set_b_extra()


@functools.lru_cache(maxsize=None)
def set_c() -> tuple:
    """lz4_decompress_mixed_kernel<false>, 4 KiB input ring: its LDS pass
    (outputs <= 4 096) and its ring pass (above), none above 65 546."""
    rng = random.Random(0xC)
    cases = [random_block(rng, rng.randint(100, 4096), "c_s%d" % i) for i in range(300)]
    cases.append(random_block(rng, 4096, "c_s4096"))
    for i in range(150):
        cases.append(random_block(rng, rng.randint(4097, 20000), "c_r%d" % i, ring=True, rare=True))
    cases.append(random_block(rng, 4097, "c_r4097", ring=True))
    cases.append(random_block(rng, 65546, "c_r65546", ring=True, rare=True))
    cases += sweep_blocks(rng, 2900, 0, "c_s")
    cases += sweep_blocks(rng, 20000, 6200, "c_r")
    cases += [far_block(rng, "c_far%d" % i) for i in range(6)]
    cases.append(long_block(rng, "c_long", lead=400))
    # literal runs of one input ring plus ~100 bytes (4 196 and 8 292): the run is
    # copied in pieces across the ring's refills, and the bytes after it sit at
    # the ring slots of the bytes before it -- where a register window loaded
    # before the run would still seem to hold them
    for i, lead in enumerate((200, 700, 1200, 1700)):
        cases.append(long_block(rng, "c_wrap%d" % i, lits=(4196, 8292), mlens=(), lead=lead))
    for kind in STRADDLE_KINDS[:5]:
        cases += [straddle_block(rng, kind, 7, "c_%s%d" % (kind, i)) for i in range(7)]
    for k in range(2):
        cases += ill_formed(rng, False, "c_ill%d" % k)
        cases += ill_formed(rng, True, "c_illbig%d" % k)
    cases += ill_fixed()
    assert max(c.size for c in cases) == 65546
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def set_d_extra() -> tuple:
    rng = random.Random(0xD)
    return (random_block(rng, 70000, "d_r70000", ring=True, rare=True),)


def set_d() -> tuple:
    """The same kernel with the 8 KiB input ring (a value above 65 546 bytes in
    the batch): set (c) plus one block of 70 000 bytes; every value above
    6 144 bytes goes through the whole-step ring stores."""
    return set_c() + set_d_extra()


@functools.lru_cache(maxsize=None)
def set_e() -> tuple:
    """lz4_decompress_big_kernel: three single-block calls."""
    rng = random.Random(0xE)
    heads = {9000: [], 20000: straddle_seqs(rng, ["lit_chain"], 1, 4096),
             70000: straddle_seqs(rng, ["token_last", "offset", "ml_chain", "token_first"], 4, 4096)}
    return tuple(random_block(rng, n, "e_%d" % n, ring=True, head=heads[n], exact_end=True, dense=True)
                 for n in (9000, 20000, 70000))


SETS = {"a": set_a, "b": set_b, "c": set_c, "d": set_d, "e": set_e}


def service_cases() -> list:
    """About 200 blocks of <= 8 192 output bytes from (a) and (b), well-formed
    and ill-formed, for the per-call service."""
    a, b = set_a(), set_b_extra()
    ill = [c for c in a if c.kind == "ill"]
    rnd = [c for c in a if c.kind == "random"][::9]
    swp = [c for c in a if c.kind == "sweep"][::4]
    return ill + rnd + swp + list(b[::6]) + list(b[-4:])


def in_ring_pass(cs: Case, out_small: int) -> bool:
    """The mixed launch's split: a value is the ring decoder's if its output is
    above out_small (4 096 with the 4 KiB input ring, 6 144 with the 8 KiB
    one) or its block above out_small + out_small / 255 + 24."""
    return cs.size > out_small or len(cs.block) > out_small + out_small // 255 + 24


# ------------------------------------------------------- coverage conditions
# One per block at most (its last sequence): a set of three blocks holds three.
END_KEYS = ("lit_end=size-12", "match_end=size-5", "ip_lit_end=csize-8")
MIN_COUNT = 20


def _short(n: Counter, keys, need=MIN_COUNT) -> list:
    return ["%s: %d < %d" % (k, n[k], need) for k in keys if n[k] < need]


def _ill_missing(cases, big: bool) -> list:
    names = [c.name for c in cases if c.kind == "ill"]
    want = "illbig" if big else "ill"
    miss = [cls for cls in ILL_CLASSES
            if not any(nm.endswith("_" + cls) and ("illbig" in nm) == big for nm in names)]
    if not big:
        miss += [nm for nm in ("size0_00", "size0_10_41", "b41") if nm not in names]
    return ["ill-formed class absent (%s): %s" % (want, m) for m in miss]


def coverage_problems(name: str) -> list:
    """The conditions that keep the tests honest, as a list of what fails (empty:
    all hold).  Per set: at least 20 sequences on each side of every boundary
    that applies to its launch (REQUIRED_BLOCK / REQUIRED_RING; in the mixed
    launches counted separately over the values of its ring pass and of its
    LDS pass), every (offset, length) pair of the sweep in each of its three
    positions (for the ring pass at output positions past 4 096), every
    constructed straddle and far match, every ill-formed class, and at least
    90 % of the blocks well-formed.  (e) is three blocks: the three boundaries
    that only a block's last sequence can sit on are counted once per block."""
    cases = SETS[name]()
    bad = []
    wf = sum(1 for c in cases if c.decoded is not None)
    if wf < 0.9 * len(cases):
        bad.append("well-formed: %d of %d" % (wf, len(cases)))
    pairs = set(sweep_pairs())

    def sweep_ok(sub, min_op, what):
        seen = sweep_seen(sub, min_op)
        lack = [p for p in sorted(pairs) if seen.get(p) != {"a", "b", "c"}]
        if lack:
            bad.append("%s: sweep pairs missing %s ..." % (what, lack[:5]))

    if name in ("a", "b"):
        bad += _short(tally(cases), REQUIRED_BLOCK)
        sweep_ok(cases, 0, name)
        bad += _ill_missing(cases, False)
        if name == "b":
            lits = {len(s[0]) for c in cases if c.seqs for s in c.seqs}
            mls = {s[2] for c in cases if c.seqs for s in c.seqs}
            if not ({2100, 5000} <= lits and 5000 in mls):
                bad.append("b: runs of 2 100 / 5 000 literals or the match of 5 000 absent")
    elif name in ("c", "d"):
        out_small, B = (4096, 2048) if name == "c" else (6144, 4096)
        ring = [c for c in cases if in_ring_pass(c, out_small)]
        lds = [c for c in cases if not in_ring_pass(c, out_small)]
        n = tally(ring)
        bad += ["ring pass: " + x for x in _short(n, REQUIRED_RING)]
        bad += ["ring pass: " + x for x in _short(n, ["straddle%d:%s" % (B, k) for k in STRADDLE_KINDS])]
        bad += ["LDS pass: " + x for x in _short(tally(lds), REQUIRED_BLOCK)]
        sweep_ok(ring, 4097, "ring pass")
        sweep_ok(lds, 0, "LDS pass")
        far = {(s[1], s[2]) for c in ring if c.seqs for s in c.seqs if not s[0]}
        lack = [(o, m) for o in FAR_OFFS for m in FAR_MLENS if (o, m) not in far]
        if lack:
            bad.append("ring pass: far matches after 0 literals missing %s" % lack)
        lits = {len(s[0]) for c in ring if c.seqs for s in c.seqs}
        if not {2100, 5000, 4196, 8292} <= lits:
            bad.append("ring pass: runs of 2 100 / 5 000 literals, or of a ring plus 100, absent")
        bad += _ill_missing(lds, False) + _ill_missing(ring, True)
        top = max(c.size for c in cases)
        if top != (65546 if name == "c" else 70000):
            bad.append("largest output %d" % top)
    else:
        n = tally(cases)
        bad += _short(n, [k for k in REQUIRED_RING if k not in END_KEYS])
        bad += _short(n, END_KEYS, len(cases))
        bad += _short(n, ["straddle4096:%s" % k for k in STRADDLE_KINDS], 1)
    return bad


# ------------------------------------------------- the reference's results
def stored_sets() -> dict:
    """The sets tests/golden/foreign_blocks.npz holds results for (b = a + bx,
    d = c + dx; g: the service's cases)."""
    return {"a": set_a(), "bx": set_b_extra(), "c": set_c(), "dx": set_d_extra(), "e": set_e(),
            "g": tuple(service_cases())}


def results(dec, cases) -> dict:
    """{ret, crc, tret, tcrc}: dec.decompress's return code and dec.crc32c of
    its output per case, with the full size as the target and with the partial
    target target_of(case); dec is the oracle or the reference."""
    import numpy as np
    ret, crc, tret, tcrc = [], [], [], []
    for c in cases:
        r, out = dec.decompress(c.block, c.size)
        ret.append(r)
        crc.append(dec.crc32c(out) if r > 0 else 0)
        r, out = dec.decompress(c.block, c.size, target_of(c))
        tret.append(r)
        tcrc.append(dec.crc32c(out) if r > 0 else 0)
    return {"ret": np.array(ret, np.int32), "crc": np.array(crc, np.uint32),
            "tret": np.array(tret, np.int32), "tcrc": np.array(tcrc, np.uint32)}

"""CPU: the oracle's key hashes and the Get and scan models, pinned to the
reference on keys of every length (tests/golden/key_lengths.npz, written by
the reference's ref_db and confirmed by its --verify run: see
tests/golden/make_golden_keylens.py).

  * every row of every offset array the reference wrote carries
    orc.xxh64(key) / orc.murmur3_64(key) of the entry's stored key: the
    reference's own hash of keys with every MurmurHash3 tail (len & 15 =
    0..15, the k1 and the k2 half) behind 0..62 blocks, and of xxHash-64 below
    and from 32 bytes;
  * index_model.Model.get returns, for every distinct key, a value of the
    length and CRC32C the reference's Database::Get returned, which is the
    last value put;
  * scan_model.scan visits exactly the distinct keys, as many as the
    reference's iterator visited.
After this the models are the checkers of tests/test_gpu_key_lengths.py.
"""
import pytest

import index_model as M
import keylens
import scan_model as S
from kingdb_amd import get as G


@pytest.fixture(scope="module")
def sets():
    return keylens.load()


def test_fixture_holds_the_key_set(sets):
    """What the tests of this fixture rely on, so that a later edit of the
    fixture cannot empty them."""
    want = set(range(1, 81)) | {127, 128, 129, 300, 1000} | set(range(252, 261)) | set(range(511, 517))
    for name, s in sets.items():
        lens = {len(k) for k in s["keys"]}
        assert want <= lens and 0 not in lens, name
        assert len(s["files"]) >= 2, name
        spots = set()
        for a, b, at in s["twins"]:
            assert len(a) == len(b) and [i for i in range(len(a)) if a[i] != b[i]] == [at]
            spots.add((len(a), at))
        assert {(16, 0), (67, 66), (255, 254), (256, 255), (257, 256), (259, 255), (260, 256), (513, 512),
                (1000, 998), (66, 65), (514, 513)} <= spots, name
        count = {}
        for k, _, _ in s["puts"]:
            count[k] = count.get(k, 0) + 1
        hot = [(len(k), count[k]) for k in s["hot"]]
        assert hot == ([(19, 70), (258, 130)] if name == "xx" else [(19, 70)])
        for k in s["hot"]:                                   # the overwrites fall in different files
            assert all(any(e.key == k for e in G.read_hstable(f)) for f in s["files"].values())
        assert sum(1 for c in count.values() if c == 2) >= len(count) // 4
        sizes = {len(v) for _, v, _ in s["puts"]}
        assert {0, 1, 13, 100} <= sizes and any(300 <= n <= 2000 for n in sizes)
        assert sum(1 for _, _, ch in s["puts"] if len(ch) == 2) == 1
    assert sets["xx"]["hash_type"] == 1 and sets["murmur"]["hash_type"] == 0


@pytest.mark.parametrize("name", ["xx", "murmur"])
def test_oracle_hash_is_the_reference_hash(sets, orc, name):
    s = sets[name]
    h = orc.xxh64 if s["hash_type"] == 1 else orc.murmur3_64
    tails, long_keys, rows_seen = set(), set(), 0
    for fname, f in s["files"].items():
        rows = M.parse_rows(f)
        ents = G.read_hstable(f)
        assert len(rows) == len(ents)
        for (rh, off), e in zip(rows, ents):
            assert off == e.offset
            assert rh == h(e.key), (name, fname, len(e.key))
            assert e.hashed == rh                            # the entry header holds it too
            tails.add(len(e.key) & 15)
            if len(e.key) >= 32:
                long_keys.add(e.key)
            rows_seen += 1
    assert rows_seen == len(s["puts"])
    assert tails == set(range(16))
    assert len(long_keys) >= 3
    # blocks before the tail: every tail behind 0, 1, 2, 3 and 4 whole blocks
    assert {(len(k) >> 4, len(k) & 15) for k in s["keys"]} >= {(b, t) for b in range(5) for t in range(16)} - {(0, 0)}


@pytest.mark.parametrize("name", ["xx", "murmur"])
def test_model_get_returns_what_the_reference_returned(sets, orc, name):
    s = sets[name]
    m = M.Model(s["files"], orc, s["hash_type"])
    assert set(m.file_status.values()) == {0}
    assert len(m.rows) == len(s["puts"])
    assert sorted(s["last"]) == s["keys"]
    for verify in (0, 2):
        for k, n, c in zip(s["keys"], s["lens"], s["crcs"]):
            st, val, loc = m.get(k, verify)
            assert (st, len(val), orc.crc32c(val)) == (0, int(n), int(c)), (len(k), verify)
            assert val == s["last"][k]
            assert loc >> 32 in [int(f, 16) for f in s["files"]]
    for k in s["keys"]:
        assert m.get(k[:-1])[0] == M.NOTFOUND and m.get(k + b"\0")[0] == M.NOTFOUND
    assert m.get(b"")[0] == M.NOTFOUND


@pytest.mark.parametrize("name", ["xx", "murmur"])
def test_model_scan_is_what_the_reference_iterated(sets, orc, name):
    s = sets[name]
    m = M.Model(s["files"], orc, s["hash_type"])
    assert s["iterator_bad"] == 0 and s["iterated"] == len(s["keys"])
    want = {(k, int(n), int(c)) for k, n, c in zip(s["keys"], s["lens"], s["crcs"])}
    for verify in (0, 2):
        got = S.scan(m, verify)
        assert len(got) == s["iterated"]
        assert sorted(k for k, _, _ in got) == s["keys"]     # exactly the distinct keys, each once
        assert all(st == 0 for _, st, _ in got)
        assert {(k, len(v), orc.crc32c(v)) for k, _, v in got} == want
        assert S.prepare(m, verify) == (len(s["keys"]), sum(map(len, s["keys"])), 1000)
    order = [(rank, off) for rank, off, _, _ in S.live_rows(m)]
    assert order == sorted(order) and len(set(order)) == len(order)

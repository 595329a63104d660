"""A branch table for the put path's multipart policy -- TEST INFRASTRUCTURE ONLY.

classify() names the branches one put takes through Database::PutPartValidSize
(interface/database.cc:128-276) and HSTableManager::WriteOrdersAndFlushFile
(storage/hstable_manager.h:714-847), from what each call handed on: the
results of oracle.put_part, call by call, which carry the compressed offset,
chunk_final, size_value_compressed and the refusal per call.  It follows the
orders the way the manager does for one key of one client thread:

  * a call whose compressed offset is 0 is a first part (util/order.h:44-46)
    and starts an entry, self-contained if it also looks last (:52-59);
  * a later call is written into the entry in progress, and ends it if it
    looks last; with no entry in progress it is dropped
    (hstable_manager.h:787-799);
  * a call that looks last, in either role, forgets the key's entry in
    progress (:821-833), so every call after it is dropped.

The classes are tags, not a partition: a put may carry several.  A test
counts them over a stream to show that the stream reaches every branch.
"""
from __future__ import annotations

# the classes the streams of hstable_streams.npz reach
OLD_CLASSES = (
    "self_contained_one_chunk",     # one call, first and last
    "disable_one_chunk",            # ... whose frame did not fit: 8 zero bytes + raw (database.cc:196-209)
    "multipart_finished_svc",       # an entry finished by a last part that carried size_value_compressed > 0
    "disable_last_chunk",           # several calls, the disable rule fires on the final one
    "multipart_unfinished",         # an entry no call finished: the first-part header stays (kind 2)
    "empty_value_one_chunk",        # size_value 0, chunks [0]
)
# the classes only ragged chunkings reach
RAGGED_CLASSES = (
    "self_contained_chunks_dropped",    # the first call already looks last; later calls dropped
    "early_last_chunks_dropped",        # an entry finished by a call that is not the value's last part
    "multipart_finished_svc0",          # an entry finished with size_value_compressed 0 in its header
    "disable_first_of_several",         # several calls, the disable rule fires on the first
    "disable_middle",                   # ... on a call that is neither first nor final
    "empty_chunk_first",                # several calls, the first empty: the next call is a first part again
    "empty_chunk_middle",
    "empty_chunk_last",
    "last_part_twice",                  # empty final chunks: two or more calls are the value's last part
    "refused",                          # a call returns IOError (database.cc:261-266)
    "dropped_bytes_zero_filled",        # a reserved region keeps zeros where a dropped chunk's bytes would lie
)
CLASSES = OLD_CLASSES + RAGGED_CLASSES


def looks_last(r: dict, size_value: int) -> bool:
    """Order::IsLastPart (util/order.h:52-55) of the order a call queues."""
    end = r["occ"] + len(r["chunk_final"])
    return (r["svc"] == 0 and end == size_value) or (r["svc"] != 0 and end == r["svc"])


def orders(size_value: int, calls: list[dict]) -> tuple[list[dict], list[int]]:
    """(entries, dropped): per first-part order {"first": call, "selfc": bool,
    "fin": the call that finished it or None, "svc": its header's
    size_value_compressed, "parts": calls written into it}, and the calls no
    entry received."""
    entries, dropped = [], []
    cur = None
    for i, r in enumerate(calls):
        if r["rc"] != 0:
            continue
        last = looks_last(r, size_value)
        if r["occ"] == 0:
            e = {"first": i, "selfc": last, "fin": i if last else None, "svc": r["svc"], "parts": [i]}
            entries.append(e)
            cur = None if last else e
        elif cur is None:
            dropped.append(i)
        else:
            cur["parts"].append(i)
            if last:
                cur["fin"], cur["svc"] = i, r["svc"]
                cur = None
    return entries, dropped


def classify(size_value: int, chunks: list[int], calls: list[dict]) -> set[str]:
    """The classes of one put: `chunks` the sizes of its calls, `calls` the
    oracle.put_part results of those calls in order."""
    n = len(calls)
    assert n == len(chunks) and n >= 1
    tags = set()
    entries, dropped = orders(size_value, calls)
    if any(r["rc"] != 0 for r in calls):
        tags.add("refused")
    if n == 1 and entries and entries[0]["selfc"]:
        tags.add("self_contained_one_chunk")
        if calls[0]["mode"] == 1:
            tags.add("disable_one_chunk")
        if size_value == 0:
            tags.add("empty_value_one_chunk")
    if n > 1:
        if calls[0]["mode"] == 1:
            tags.add("disable_first_of_several")
        if any(r["mode"] == 1 for r in calls[1:-1]):
            tags.add("disable_middle")
        if calls[-1]["mode"] == 1:
            tags.add("disable_last_chunk")
        if chunks[0] == 0:
            tags.add("empty_chunk_first")
        if any(c == 0 for c in chunks[1:-1]):
            tags.add("empty_chunk_middle")
        if chunks[-1] == 0:
            tags.add("empty_chunk_last")
    off = 0
    dblast = []                                 # database.cc:149 per call
    for c in chunks:
        dblast.append(off + c == size_value)
        off += c
    if size_value and sum(dblast) > 1:
        tags.add("last_part_twice")
    for e in entries:
        if e["selfc"]:
            if e["first"] < n - 1 and any(calls[j]["rc"] == 0 for j in range(e["first"] + 1, n)) \
                    and all(j in dropped for j in range(e["first"] + 1, n) if calls[j]["rc"] == 0):
                tags.add("self_contained_chunks_dropped")
            continue
        if e["fin"] is None:
            tags.add("multipart_unfinished")
            continue
        tags.add("multipart_finished_svc" if e["svc"] > 0 else "multipart_finished_svc0")
        if not dblast[e["fin"]]:
            tags.add("early_last_chunks_dropped")
        if any(j > e["fin"] and len(calls[j]["chunk_final"]) for j in dropped):
            tags.add("dropped_bytes_zero_filled")
    return tags


def classify_put(orc, key: bytes, value: bytes, chunks: list[int] | None, state=None):
    """classify() of one put through oracle.put_part: (classes, calls).  `state`
    is the client thread's PutState carried from its earlier puts (a fresh
    thread's by default)."""
    import oracle
    chunks = [len(value)] if chunks is None else list(chunks)
    st = oracle.PutState() if state is None else state
    calls, off = [], 0
    for c in chunks:
        calls.append(oracle.put_part(orc, st, key, value[off:off + c], off, len(value)))
        off += c
    return classify(len(value), chunks, calls), calls


def table(orc, puts) -> dict[str, int]:
    """Puts per class over a stream, one client thread."""
    import oracle
    st = oracle.PutState()
    out = {c: 0 for c in CLASSES}
    for k, v, ch in puts:
        for t in classify_put(orc, k, v, ch, st)[0]:
            out[t] += 1
    return out

"""The offset conversions (ByteToCharOffsetsBatchDevice / CharToByteOffsetsBatchDevice) restated sequentially, and the table of cases both tiers run.

The restatement is the header's definition read aloud: a loop over the bytes of a document for C_d, a loop over C_d for B_d, a loop over the items.
Nothing of the index (chunks, masks, prefix sums, searches) appears here.  `table()` lists the cases, `check_table()` asserts what each is there
for, `items_for()` makes the exhaustive positions of a case: every i in -1 .. limit + 1 of every document that has items, as a start and as an end."""
import numpy as np

CHAR, UTF16 = 0, 1
FWD, INV = 0, 1
ENDS_IN_EXCLUSIVE, ENDS_OUT_EXCLUSIVE = 1, 2
BAD = 8                                                       # BfLastStatus bit 3
CANARY32 = -0x5A5A5A5B
UNITS = (CHAR, UTF16)
ALL_FLAGS = (0, 1, 2, 3)
TILE_CHUNKS = 1024                                            # chunks one block of the scan takes


def weight(b, unit):
    if (b & 0xC0) == 0x80:
        return 0
    return 2 if unit == UTF16 and b >= 0xF0 else 1


def c_table(doc, unit):
    """C_d(0 .. n_d)"""
    C = [0]
    for b in doc:
        C.append(C[-1] + weight(b, unit))
    return C


def b_table(C):
    """B_d(0 .. U_d) from C_d"""
    n, U = len(C) - 1, C[-1]
    B = []
    for k in range(U + 1):
        if k == U:
            B.append(n)
            continue
        i = 0
        while not C[i + 1] > k:
            i += 1
        B.append(i)
    return B


def doc_bytes(text, doc_off, d):
    """-> (the document's bytes, bad): a range outside the text or with decreasing offsets reads as empty"""
    b, e = int(doc_off[d]), int(doc_off[d + 1])
    if b < 0 or e < b or e > len(text):
        return b"", True
    return bytes(text[b:e]), False


def restate(text, doc_off, unit, direction, flags=0, starts=None, ends=None, item_off=None, items_cap=None):
    """-> dict(starts, ends: int32 arrays of the n items that are converted, or None; doc_units int32[ndocs]; status; n)"""
    ndocs = len(doc_off) - 1
    status = 0
    F, units = [], []
    for d in range(ndocs):
        doc, bad = doc_bytes(text, doc_off, d)
        if bad:
            status |= BAD
        C = c_table(doc, unit)
        F.append(C if direction == FWD else b_table(C))
        units.append(C[-1])
    given = starts if starts is not None else ends
    n_all = ndocs if item_off is None else int(item_off[ndocs]) if ndocs else 0
    cap = (0 if given is None else len(given)) if items_cap is None else items_cap
    n = min(cap, n_all) if ndocs else 0
    out = {"starts": None if starts is None else np.full(n, CANARY32, dtype=np.int32), "ends": None if ends is None else np.full(n, CANARY32, dtype=np.int32)}
    d = 0
    for i in range(n):
        if item_off is None:
            d = i
        else:
            while not (item_off[d] <= i < item_off[d + 1]):
                d += 1
        f = F[d]
        for name, src, is_end in (("starts", starts, False), ("ends", ends, True)):
            if src is None:
                continue
            v = int(src[i])
            if v < 0:
                out[name][i] = -1
                continue
            x = v + 1 if is_end and not flags & ENDS_IN_EXCLUSIVE else v
            if x > len(f) - 1:
                out[name][i] = -1
                status |= BAD
                continue
            out[name][i] = f[x] - 1 if is_end and not flags & ENDS_OUT_EXCLUSIVE else f[x]
    out.update(doc_units=np.array(units, dtype=np.int32), status=status, n=n)
    return out


# ---- the cases
MIX = "aé€\U0001F600b"                              # 1 + 2 + 3 + 4 + 1 bytes
PATTERN = ("é€\U0001F600a" * 40).encode()           # 10 bytes a period


def filled(total):
    """`total` bytes of valid UTF-8: whole periods of the pattern, then 'x'"""
    k = total // 10
    return PATTERN[:10 * k] + b"x" * (total - 10 * k)


def pack(docs, **more):
    bs = [d.encode() if isinstance(d, str) else bytes(d) for d in docs]
    off = np.zeros(len(bs) + 1, dtype=np.int64)
    if bs:
        off[1:] = np.cumsum([len(b) for b in bs])
    c = dict(text=b"".join(bs), doc_off=off, valid=True, skip=0)
    c.update(more)
    return c


def big_docs():
    """about 70 KB from a short table of documents (as tiny_cases packs its batches), with one document over the edge of the scan's tile"""
    table = [MIX, "", "x", "héllo wörld", "\U0001F600\U0001F600\U0001F600", "plain ascii text of some length. ", "中文文本", "é"]
    docs, total, k = [], 0, 0
    edge = 64 * TILE_CHUNKS
    while total < edge - 700:
        docs.append(table[k % len(table)].encode())
        total += len(docs[-1]); k += 1
    docs.append((MIX * 150).encode())                         # 1650 bytes: from in front of byte 65536 to behind it
    total += len(docs[-1])
    while total < 70000:
        docs.append(table[k % len(table)].encode())
        total += len(docs[-1]); k += 1
    return docs


def table():
    t = []
    t.append(dict(pack([MIX, "\U0001F600\U0001F600", "héllo wörld", "", "z"]), name="mixed"))
    t.append(dict(pack([filled(63), "q", "r", "€és", filled(70)]), name="edge64"))      # documents start at 63, 64, 65; one ends at 64
    t.append(dict(pack([b"x" * 62 + "\U0001F600".encode() + b"xyz"]), name="four_over_edge"))
    t.append(dict(pack(["pre", (MIX * 18).encode() + b"xy", "post"]), name="three_chunks"))
    t.append(dict(pack(["", "", "ab", "", "", "", "é", "", ""]), name="empty_runs"))
    t.append(dict(pack(["", "", ""]), name="no_text"))
    t.append(dict(pack([]), name="no_docs"))
    for total in (63, 64, 65, 64 * 3 + 1, 64 * 3 + 63):
        t.append(dict(pack([filled(total // 2), filled(total - total // 2)]), name="total_%d" % total))
    t.append(dict(pack([b"\x80\x80ab", b"ab\xe2", bytes(range(0xF8, 0x100)), b"\x80\x81\xbf", b"\xf0\x9f", b"a\xff\x80"], valid=False), name="invalid"))
    t.append(dict(pack([MIX, "ab", "éé", "", "q\U0001F600"], skip=2), name="docs_without_items"))
    bad = dict(pack([b"0123456789"]), name="bad_ranges")
    bad["doc_off"] = np.array([0, 4, 2, 12, 10], dtype=np.int64)  # [0, 4) good; [4, 2) decreasing; [2, 12) past the text; [12, 10) both
    bad["bad"] = True
    t.append(bad)
    t.append(dict(pack(big_docs()), name="big"))
    return t


SMALL = [c["name"] for c in table() if c["name"] != "big"]


def case_named(name):
    return next(c for c in table() if c["name"] == name)


def check_table():
    """what each case is there for, asserted on the case itself"""
    by = {c["name"]: c for c in table()}
    lens = sorted({len(ch.encode()) for ch in MIX})
    assert lens == [1, 2, 3, 4] and MIX.encode() in by["mixed"]["text"]
    off = by["edge64"]["doc_off"].tolist()
    assert {63, 64, 65} <= set(off[:-1]) and 64 in off[1:]
    assert by["four_over_edge"]["text"][62:66] == "\U0001F600".encode()
    c = by["three_chunks"]
    assert any((int(e) - 1) // 64 - int(b) // 64 >= 2 for b, e in zip(c["doc_off"][:-1], c["doc_off"][1:]) if e > b)
    lens = np.diff(by["empty_runs"]["doc_off"]).tolist()
    assert lens[:2] == [0, 0] and lens[3:6] == [0, 0, 0] and 1 not in lens[:2] and 2 in lens
    assert 1 in np.diff(by["mixed"]["doc_off"]).tolist()       # a one-byte document
    assert len(by["no_text"]["text"]) == 0 and len(by["no_text"]["doc_off"]) == 4 and len(by["no_docs"]["doc_off"]) == 1
    assert [len(by["total_%d" % n]["text"]) for n in (63, 64, 65, 193, 255)] == [63, 64, 65, 193, 255]
    inv = by["invalid"]
    docs = [doc_bytes(inv["text"], inv["doc_off"], d)[0] for d in range(len(inv["doc_off"]) - 1)]
    assert docs[0][:2] == b"\x80\x80" and docs[1][-1] == 0xE2 and set(docs[2]) == set(range(0xF8, 0x100))
    assert c_table(docs[3], CHAR)[-1] == 0 and b_table(c_table(docs[3], CHAR)) == [len(docs[3])]
    big = by["big"]
    edge = 64 * TILE_CHUNKS
    assert len(big["text"]) > 64 * TILE_CHUNKS + 64 and 69000 < len(big["text"]) < 72000
    assert any(b < edge - 64 and e > edge + 64 for b, e in zip(big["doc_off"][:-1], big["doc_off"][1:]))
    assert by["docs_without_items"]["skip"] == 2 and by["bad_ranges"].get("bad")
    for c in by.values():
        if c["valid"] and not c.get("bad"):
            c["text"].decode()                                 # valid UTF-8 where the case says so
    return True


def items_for(case, unit, direction, beyond=True):
    """the exhaustive positions: for every document that has items (every `skip`-th has none), every position in -1 .. limit + 1 (limit = n_d
    forward, U_d inverse; without `beyond` up to the limit only), the same values as starts and as ends.  -> (values int32, item_off int64)"""
    text, doc_off = case["text"], case["doc_off"]
    vals, off = [], [0]
    for d in range(len(doc_off) - 1):
        doc, _ = doc_bytes(text, doc_off, d)
        limit = len(doc) if direction == FWD else c_table(doc, unit)[-1]
        if not (case["skip"] and d % case["skip"] == 1):
            vals += list(range(-1, limit + (2 if beyond else 1)))
        off.append(len(vals))
    return np.array(vals, dtype=np.int32), np.array(off, dtype=np.int64)


def ends_for(values, flags):
    """the same positions as ends: an inclusive input end e stands for x = e + 1, so the values move down by one (0 becomes -1, "none": x = 0 has no inclusive form)"""
    return values if flags & ENDS_IN_EXCLUSIVE else np.where(values >= 0, values - 1, values).astype(np.int32)


def restate_array(text, doc_off, unit, direction, flags, starts, ends, item_off):
    """the restatement in array form, for batches too large for the loop (every document's range good, every item inside a document):
    held to `restate` on the table by the CPU tier.  -> (starts, ends, doc_units, status)"""
    t = np.frombuffer(bytes(text), dtype=np.uint8) if not isinstance(text, np.ndarray) else text
    w = ((t & 0xC0) != 0x80).astype(np.int64) + (((t >= 0xF0).astype(np.int64)) if unit == UTF16 else 0)
    G = np.concatenate([[0], np.cumsum(w)])
    doc_off = np.asarray(doc_off, dtype=np.int64)
    units = G[doc_off[1:]] - G[doc_off[:-1]]
    n = len(starts if starts is not None else ends)
    d = np.searchsorted(item_off, np.arange(n), side="right") - 1 if item_off is not None else np.arange(n)
    b, nd, Gb, U = doc_off[d], doc_off[d + 1] - doc_off[d], G[doc_off[d]], units[d]
    status, out = 0, []
    for src, is_end in ((starts, False), (ends, True)):
        if src is None:
            out.append(None)
            continue
        v = src.astype(np.int64)
        x = v + 1 if is_end and not flags & ENDS_IN_EXCLUSIVE else v
        limit = nd if direction == FWD else U
        ok = (v >= 0) & (x <= limit)
        xs = np.where(ok, x, 0)
        if direction == FWD:
            y = G[b + xs] - Gb
        else:
            y = np.where(xs == U, nd, np.searchsorted(G, Gb + xs, side="right") - 1 - b)
        if is_end and not flags & ENDS_OUT_EXCLUSIVE:
            y = y - 1
        if ((v >= 0) & ~ok).any():
            status |= BAD
        out.append(np.where(ok, y, -1).astype(np.int32))
    return out[0], out[1], units.astype(np.int32), status

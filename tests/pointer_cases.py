"""Shared TEST helpers for the caller's pointers of the ...BatchDevice calls (tests/test_gpu_caller_pointers.py, GPU tier) and of the flat program's
merge in the simulator (tests/test_flat_emu.py, CPU tier): include/blingfiretokdll_amd.h promises that a device pointer needs nothing beyond
the natural alignment of its element type, that d_text needs no padding and may be d_text + first_byte of a larger buffer, and that no output is
written at or past its capacity.

  place()  an input INSIDE a larger device tensor: [guard >= 4096 B that ends with `front`] [payload] [guard >= 4096 B that begins with `back`],
           the payload's first byte shift_bytes behind a 256-byte boundary; verify() holds every byte of the tensor to what was put there.
  room()   an output inside a canary-filled device tensor (the canaries of tests/test_gpu_secondary_at_scale.py), its first item shift_items items
           behind a 16-byte boundary; untouched(cap) holds everything in front of it and everything at or behind cap to the canary.

An over-read or a stray store of a kernel that is off by a few bytes lands in memory the test owns and shows as a wrong answer or a changed canary;
no payload lies against the true end of an allocation.  The surroundings are chosen to change the answer when they are taken in: the "completing"
one continues a truncated character and a word across both ends of the text.  END_CASES / START_CASES are last / first documents made for that,
and prove() asserts with the CPU checker that each of them does detect it.

No torch at import time: the CPU tier takes the shift lists from here."""
import numpy as np

from test_gpu_secondary_at_scale import CANARY as _CANARY

GUARD = 4096
CANARY = dict(_CANARY)
CANARY[np.dtype(np.int64)] = 0x5A5A5A5A5A5A5A5A

TEXT_SHIFTS = tuple(range(18)) + (31, 32, 33, 63, 65)
# (ids, starts, ends) item shifts behind a 16-byte boundary: k_wp_merge stores whole 16-byte rows where ids_out allows it and may do the same for
# starts_out / ends_out only when they are aligned like ids_out (its rows_ok): 4 of these 16 combinations
OUT_SHIFTS_3 = tuple((i, (i + ds) % 4, (i + de) % 4) for i in range(4) for ds, de in ((0, 0), (1, 0), (0, 2), (1, 3)))
assert len(set(OUT_SHIFTS_3)) == 16 and sum(1 for a, b, c in OUT_SHIFTS_3 if a == b == c) == 4

SURROUNDINGS = {
    # a lead byte in front of the text; its continuation byte, the rest of a word, a U+2581 and a special token behind it
    "completing": (b"these are some plain words and the last word un\xc3", b"\xa9affable \xe2\x96\x81the [UNK] ##ing and more words follow here "),
    "invalid": (b"\xff", b"\xff"),
    "zeros": (b"\x00", b"\x00"),
}
END_MODS = (0, 1, 7, 8, 9, 15)          # the end of the text this many bytes past a multiple of 512 (and so of 16)


def _front_fill(front, n):
    return (front * (n // len(front) + 1))[-n:] if n else b""


def _back_fill(back, n):
    return (back * (n // len(back) + 1))[:n]


# ------------------------------------------------------------------------------------------------
# arenas (torch is imported when one is made)
# ------------------------------------------------------------------------------------------------
class Placed:
    def __init__(self, payload, shift_bytes, front, back):
        import torch
        payload = np.ascontiguousarray(payload)
        assert shift_bytes >= 0 and shift_bytes % payload.dtype.itemsize == 0, "a shift respects the C type of the payload"
        raw = payload.view(np.uint8).reshape(-1)
        nfront = GUARD + shift_bytes
        nback = GUARD + (-(nfront + len(raw))) % 16
        self.host = np.concatenate([np.frombuffer(_front_fill(front, nfront), dtype=np.uint8), raw, np.frombuffer(_back_fill(back, nback), dtype=np.uint8)])
        self.tensor = torch.from_numpy(self.host).to("cuda")
        base = self.tensor.data_ptr()
        assert base % 256 == 0, "the allocator's base is not 256-byte aligned: the shift is not what it claims"
        self.addr = base + nfront
        self.nbytes = len(raw)

    def verify(self, what=""):
        """every byte of the arena, the payload included, is what was put there: inputs are never written"""
        got = self.tensor.cpu().numpy()
        if not np.array_equal(got, self.host):
            bad = int(np.nonzero(got != self.host)[0][0])
            raise AssertionError("%s: input arena changed at byte %d relative to the payload (%d bytes): 0x%02x -> 0x%02x" % (
                what, bad - (self.addr - self.tensor.data_ptr()), self.nbytes, int(self.host[bad]), int(got[bad])))


def place(payload, shift_bytes, front, back):
    return Placed(payload, shift_bytes, front, back)


class Room:
    def __init__(self, dtype, n_items, shift_items):
        import torch
        self.dtype = np.dtype(dtype)
        self.canary = CANARY[self.dtype]
        tdt = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64}[self.dtype]
        g = GUARD // self.dtype.itemsize
        assert shift_items >= 0
        self.n = int(n_items)
        self.first = g + shift_items
        self.tensor = torch.full((self.first + self.n + g,), self.canary, dtype=tdt, device="cuda")
        base = self.tensor.data_ptr()
        assert base % 256 == 0, "the allocator's base is not 256-byte aligned: the shift is not what it claims"
        self.addr = base + self.first * self.dtype.itemsize
        self._host = None

    def fetch(self):
        """copies the arena back (after the caller synchronised)"""
        self._host = self.tensor.cpu().numpy()
        return self

    def result(self):
        if self._host is None:
            self.fetch()
        return self._host[self.first:self.first + self.n]

    def untouched(self, cap, what=""):
        """everything in front of the address and everything at or behind item `cap` still holds the canary"""
        if self._host is None:
            self.fetch()
        front, back = self._host[:self.first], self._host[self.first + cap:]
        assert (front == self.canary).all(), "%s: written %d items in FRONT of the output address" % (what, self.first - int(np.nonzero(front != self.canary)[0][0]))
        assert (back == self.canary).all(), "%s: written at item %d, at or behind the capacity / size %d" % (what, cap + int(np.nonzero(back != self.canary)[0][0]), cap)


def room(dtype, n_items, shift_items):
    return Room(dtype, n_items, shift_items)


def host_place(payload, shift_bytes, front, back, guard=256):
    """the CPU counterpart of place() for a text: (arena, view of the payload inside it that starts shift_bytes behind a 16-byte boundary, a copy of
    the arena to hold it to afterwards)"""
    raw = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
    arena = np.empty(len(raw) + 2 * guard + 32 + shift_bytes, dtype=np.uint8)
    first = -arena.ctypes.data % 16 + guard + shift_bytes
    arena[:first] = np.frombuffer(_front_fill(front, first), dtype=np.uint8)
    arena[first:first + len(raw)] = raw
    arena[first + len(raw):] = np.frombuffer(_back_fill(back, len(arena) - first - len(raw)), dtype=np.uint8)
    view = arena[first:first + len(raw)]
    assert (view.ctypes.data - shift_bytes) % 16 == 0
    return arena, view, arena.copy()


def host_room(n_items, shift_items, dtype=np.int32, guard=64):
    """the CPU counterpart of room(): (whole array, view of n_items items that starts shift_items items behind a 16-byte boundary, its first index)"""
    dtype = np.dtype(dtype)
    whole = np.full(n_items + 2 * guard + 16, CANARY[dtype], dtype=dtype)
    pad = (-whole.ctypes.data % 16) // dtype.itemsize
    first = pad + guard - guard % (16 // dtype.itemsize) + shift_items
    view = whole[first:first + n_items]
    assert (view.ctypes.data - shift_items * dtype.itemsize) % 16 == 0
    return whole, view, first


# ------------------------------------------------------------------------------------------------
# documents whose answer changes when a neighbouring byte is taken in
# ------------------------------------------------------------------------------------------------
def _word(alphabet, nbytes):
    """a word of exactly nbytes bytes out of whole characters of `alphabet`, repeated (no flat word table holds it)"""
    out, i = b"", 0
    while len(out) < nbytes:
        c = alphabet[i % len(alphabet)].encode()
        out += c if len(out) + len(c) <= nbytes else b"s"
        i += 1
    return out


def _end_tails():
    tails = [("lead_2", b" caf\xc3"), ("lead_3", b" x \xe2\x96"), ("lead_4", b" smile \xf0\x9f\x98"), ("un", b" un"), ("th", b" th")]
    tails += [("zq_%d" % k, b" " + b"zqxjkvw"[:k]) for k in range(1, 8)]
    for L in range(1, 21):                                     # the last word inside the last 16 bytes of the text, and just outside
        tails.append(("zqword_%d" % L, b" " + _word("zqxjkvw", L)))
        tails.append(("cafes_%d" % L, b" " + _word("cafés", L)))
    return tails


# (name, the last bytes of the last document, END_MODS entry): the end of the whole text lies that many bytes past a multiple of 512
END_CASES = tuple((name, tail, END_MODS[i % len(END_MODS)]) for i, (name, tail) in enumerate(_end_tails()))
START_CASES = (("continuation", b"\xa9abc def"), ("word_tail", b"affable words"), ("piece", b"##ing along"), ("bom", b"\xef\xbb\xbfhello there"))
# adjacent documents of one batch whose concatenation would be valid, or another word
ADJACENT_PAIRS = ([b"caf\xc3", b"\xa9 au lait"], [b"un", b"affable"], [b"\xe2\x96", b"\x81x"])
_FILL = [b"the quick brown fox", "café naïve".encode(), b"Hello, world! This is a test.", b"unaffable qzxjkvw", "好好好 ok".encode(), b"", b"a", b"e-mail 3,000.50 of U.S.A."]
FILLERS = tuple(_FILL[i % len(_FILL)] + (b" %d" % i if i % 3 else b"") for i in range(70))
_PAD = b"plain words of text and "


def edge_batch(start, tail, mod):
    """[first document] + 35 fillers + the adjacent pairs + 35 fillers + [last document]: the last one is plain words and `tail`, as long as puts the
    end of the text `mod` bytes past a multiple of 512"""
    docs = [start] + list(FILLERS[:35]) + [d for pair in ADJACENT_PAIRS for d in pair] + list(FILLERS[35:])
    before = sum(len(d) for d in docs)
    npad = (mod - before - len(tail)) % 512
    if npad < 48:
        npad += 512                                           # (more than 16 bytes of plain words in front of the tail)
    docs.append((_PAD * (npad // len(_PAD) + 1))[:npad] + tail)
    assert sum(len(d) for d in docs) % 512 == mod and sum(len(d) for d in docs) % 16 == mod
    return docs


def edge_batches():
    """one batch per END_CASE (each is the last document of its own call), the START_CASES in turn"""
    return [(name + "/" + START_CASES[i % len(START_CASES)][0], edge_batch(START_CASES[i % len(START_CASES)][1], tail, mod)) for i, (name, tail, mod) in enumerate(END_CASES)]


def prove(answer):
    """answer(bytes) -> the checker's answer for a document, comparable with ==.  Every END_CASE / START_CASE: the answer for the document alone
    differs from the answer for the document extended by 1 .. 16 of the neighbouring bytes of the completing surrounding (behind the text: every
    such count that does not itself cut a character of the surrounding) -- a kernel that takes neighbouring bytes in cannot give the checker's
    answer for the payload.  Returns the number of comparisons"""
    front, back = SURROUNDINGS["completing"]
    n = 0
    for name, docs in edge_batches():
        last = docs[-1]
        alone = answer(last)
        for k in range(1, 17):
            if (back[k] & 0xC0) == 0x80:
                continue                                      # (10 and 11: inside the U+2581)
            assert answer(last + _back_fill(back, k)) != alone, "end case %s cannot detect an over-read of %d bytes" % (name, k)
            n += 1
    for name, doc in START_CASES:
        alone = answer(doc)
        for k in range(1, 17):
            assert answer(_front_fill(front, k) + doc) != alone, "start case %s cannot detect a read of %d bytes in front of the text" % (name, k)
            n += 1
    for a, b in ADJACENT_PAIRS:
        assert answer(a + b[:1]) != answer(a) or answer(a[-1:] + b) != answer(b), (a, b)
    return n

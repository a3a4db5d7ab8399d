"""Shared TEST helpers of tests/test_w2h.py: the hyphenation fixture and its edited variants, the word lists, the reference's single call
(oracle/_ref) and the stored copies of its answers (bfutil.reference_answers), so that the CPU tier (the host build of the lane programs) and
the GPU tier (the product library) are held to the same bytes."""
import ctypes
import os
import struct

import numpy as np

import bfutil
import ldbedit

FIXTURE_GZ = os.path.join(bfutil.ROOT, "tests", "golden", "w2h", "syllab.bin.gz")


def _fixture():
    """the reference's ldbsrc/ldb/syllab.bin (1,178,952 bytes, unchanged data) is committed gzip-compressed -- it is larger than a committed file
    may be -- and unpacked, byte for byte, into a directory of this user's under the temporary directory: LoadModel takes a path"""
    import gzip
    import tempfile
    data = gzip.open(FIXTURE_GZ, "rb").read()
    assert len(data) == 1178952
    d = os.path.join(tempfile.gettempdir(), "blingfire_amd_w2h_%d" % os.getuid())
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, "syllab.bin")
    if not os.path.exists(path) or open(path, "rb").read() != data:
        tmp = "%s.%d" % (path, os.getpid())
        with open(tmp, "wb") as f:
            f.write(data)
        os.replace(tmp, path)
    return path


FIXTURE = _fixture()
FUNC_W2H = 11
P_MIN_LEN, P_IGNORE_CASE, P_MULTI_MAP, P_LEFT_ANCHOR, P_MIN_LEN2 = 17, 22, 25, 27, 32
BOM = b"\xef\xbb\xbf"
UHYS = (0x2D, 0x2581, 0x1F600, 0)
BAD_UHYS = (-5, 0xD800, 0x110000)
VP, CI = ctypes.c_void_p, ctypes.c_int
CAP = 4096


# ------------------------------------------------------------------------------------------------
# the reference's single call
# ------------------------------------------------------------------------------------------------
class Ref:
    def __init__(self):
        self.L = ctypes.CDLL(bfutil.REF_LIB)
        self.L.LoadModel.restype = VP
        self.L.LoadModel.argtypes = [ctypes.c_char_p]
        self.L.FreeModel.argtypes = [VP]
        self.L.WordHyphenationWithModel.restype = CI
        self.L.WordHyphenationWithModel.argtypes = [ctypes.c_char_p, CI, VP, CI, VP, CI]
        self.fn = self.L.WordHyphenationWithModel

    def load(self, path):
        h = self.L.LoadModel(path.encode())
        assert h, path
        return h

    def free(self, h):
        self.L.FreeModel(VP(h))


def single(fn, h, w, hy, cap=CAP, null=False, first=False):
    """[return value, the buffer as far as it was written] of one WordHyphenationWithModel call (fn: the reference's, the product's, or the
    host build's with the handle first); the buffer is pre-filled with 0x7F and 64 bytes longer than the capacity"""
    buf = None if null else ctypes.create_string_buffer(b"\x7f" * (max(cap, 0) + 64), max(cap, 0) + 64)
    r = fn(VP(h), w, len(w), buf, cap, hy) if first else fn(w, len(w), buf, cap, VP(h), hy)
    if null:
        return [r, ""]
    raw = buf.raw
    assert raw[max(cap, 0):] == b"\x7f" * 64, "written past the capacity"
    end = len(raw.rstrip(b"\x7f"))
    return [r, raw[:end].decode("latin-1")]


def texts_of(fn, h, words, hy, first=False):
    """what the batch form owes per word: the single call's text without the terminator, nothing where it answers 0 or -1"""
    out = []
    for w in words:
        r, s = single(fn, h, w, hy, 8 * len(w) + 16, first=first)
        out.append(s[:r - 1] if r > 0 else "")
    return out


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def table_rows():
    """(word, uHy, capacity) of the issue's table"""
    rows = [(w.encode(), 0x2D, CAP) for w in ("syllabification", "Syllabification", "SYLLABIFICATION", "descomposición", "разбивка", "слога", "на", "a",
                                              "hello world", "co-operate", "naïve\0test")]
    rows += [(BOM + b"syllabification", 0x2D, CAP), (b"x" * 300, 0x2D, CAP), (b"x" * 301, 0x2D, CAP), ("é".encode() * 350, 0x2D, CAP),
             (b"syllabification" * 20, 0x2D, CAP), (b"syllabification" * 21, 0x2D, CAP), (b"x" * 299 + b"\xff", 0x2D, CAP), (b"x" * 300 + b"\xff", 0x2D, CAP)]
    rows += [(b"syllabification", hy, CAP) for hy in (0x2581, 0, -5, 0xD800, 0x110000)]
    rows += [(b"syllabification", 0x2D, 10), (b"", 0x2D, CAP), (BOM, 0x2D, CAP)]
    return rows


def capacity_words():
    return [b"syllabification", "descomposición".encode(), "naïve\0𝄞test-слога".encode()]


def en_words():
    return [w.encode() for w in open(bfutil.WORDS_EN).read().split()]


def corpus_words(limit=20001):
    """distinct words cut at white space from the multilingual corpus (Cyrillic, Greek, CJK, Arabic, Devanagari, Thai beside Latin)"""
    text, _ = bfutil.gen_corpus_multi(400, seed=11, nthreads=1)
    seen = dict.fromkeys(text.tobytes().split())
    return list(seen)[:limit]


def edge_words():
    """[(name, bytes)]"""
    out = [("empty", b""), ("bom_only", BOM), ("a", b"a"), ("ab", b"ab"), ("abc", b"abc"), ("e_acute", "é".encode()), ("cjk2", "音節".encode()), ("clef3", "𝄞𝄞𝄞".encode())]
    units = {1: b"x", 2: "é".encode(), 3: "節".encode(), 4: "𝄞".encode()}
    for nb, u in units.items():
        for n in (298, 299, 300, 301, 302):
            out.append(("%d_chars_of_%d_bytes" % (n, nb), u * n))
        out.append(("syllables_%d_bytes" % nb, (b"syllabi" + u) * 40))
    for n in (296, 299, 300, 303):
        out.append(("bom_%d" % n, BOM + (b"banana" * 60)[:n]))
    for at in (0, 5, 298, 299):                                  # invalid UTF-8 in front of the 300th character: rejected
        for bad in (b"\xff", b"\x80", b"\xc0\xaf", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\xe2\x82"):
            out.append(("invalid_%r_at_%d" % (bad, at), (b"hyphenation" * 40)[:at] + bad + (b"hyphenation" * 40)[at:]))
    for at in (300, 301, 400):                                   # ... behind it: never looked at
        for bad in (b"\xff", b"\x80", b"\xe2\x82"):
            out.append(("invalid_%r_at_%d" % (bad, at), (b"hyphenation" * 40)[:at] + bad + b"tail"))
    out += [("truncated_2", b"abc\xc3"), ("truncated_3", b"abc\xe2\x82"), ("truncated_4", b"abc\xf0\x9f\x98"), ("overlong", b"ab\xc1\x81cd"),
            ("bom_then_invalid", BOM + b"\xffabc"), ("two_boms", BOM + BOM + b"syllable"),
            ("nul_inside", "naïve\0test".encode()), ("nul_first", b"\0hyphen"), ("nuls", b"\0\0\0"),
            ("caret", b"^"), ("carets", b"^^^^"), ("caret_word", b"^syllable^"), ("caret_mid", b"syl^la^ble"), ("hyphen", b"-"), ("hyphens", b"co-operate--now-"),
            ("space", b"hello world"), ("digits", b"1234567890"), ("mixed_case", b"HyPhEnAtIoN"), ("upper", b"HYPHENATION"),
            ("cyrillic", "разбивка".encode()), ("cyrillic_upper", "РАЗБИВКА".encode()), ("greek", "συλλαβισμός".encode()), ("spanish", "descomposición".encode()),
            ("long_en", b"pneumonoultramicroscopicsilicovolcanoconiosis"), ("long_de", "donaudampfschifffahrtsgesellschaftskapitän".encode())]
    return out


def batch_lists():
    """name -> list of words for the batch comparisons (test 4)"""
    en = en_words()
    return {"en": en, "en_upper": [w.upper() for w in en], "en_capitalised": [w.capitalize() for w in en], "corpus": corpus_words(),
            "edge": [w for _, w in edge_words()]}


# ------------------------------------------------------------------------------------------------
# model variants (tests/ldbedit.py on section 11)
# ------------------------------------------------------------------------------------------------
VARIANTS = {"ignore_case": dict(add_boolean=P_IGNORE_CASE), "min_len2_1": dict(set_param=(P_MIN_LEN2, 1)), "min_len2_2": dict(set_param=(P_MIN_LEN2, 2)),
            "min_len2_5": dict(set_param=(P_MIN_LEN2, 5)), "min_len_8": dict(set_param=(P_MIN_LEN, 8)), "min_len_20": dict(set_param=(P_MIN_LEN, 20))}
REFUSED = {"unknown_parameter": dict(set_param=(38, 2)), "zero_anchor": dict(set_param=(P_LEFT_ANCHOR, 0)), "min_len_0": dict(set_param=(P_MIN_LEN, 0))}


def make_variant(name, tmp_path):
    dst = os.path.join(str(tmp_path), name + ".bin")
    return ldbedit.make_variant(FIXTURE, dst, FUNC_W2H, **{**VARIANTS, **REFUSED}[name])


TABLE_VARIANT_WORDS = [b"hello", b"syllabification", b"SYLLABIFICATION"]


def variant_words():
    en = en_words()
    return TABLE_VARIANT_WORDS + en[:3000] + [w.upper() for w in en[:1500]] + [w for _, w in edge_words()]


def make_bad_pattern_value(tmp_path, value=-1):
    """the fixture with the first value of pattern 0 replaced by HYPH_UNKNOWN: the pattern map is a FAMultiMap_pack (uint32 max key, uint32 size of
    offset, big-endian offsets (0 = none, else chain offset + 1), padding to 4, {int32 size of value, int32 max count}, then [count, values] per chain)"""
    dumps = ldbedit.read_ldb(FIXTURE)
    conf = ldbedit.decode_conf(dumps[0])
    which = dict(ldbedit.params(conf[FUNC_W2H]))[P_MULTI_MAP]
    d = bytearray(dumps[which])
    max_key, soo = struct.unpack_from("<II", d, 0)
    chains = 8 + soo * (1 + max_key)
    chains += (-chains) % 4
    sov = struct.unpack_from("<i", d, chains)[0]
    vo = int.from_bytes(d[8:8 + soo], "big")
    assert vo > 0 and sov in (1, 2, 4)
    at = chains + vo - 1 + sov                                   # behind the count
    d[at:at + sov] = int(value).to_bytes(sov, "little", signed=True)
    dumps[which] = bytes(d)
    return ldbedit.write_ldb(os.path.join(str(tmp_path), "bad_pattern_value.bin"), dumps, conf)


# ------------------------------------------------------------------------------------------------
# the reference's answers, live or stored
# ------------------------------------------------------------------------------------------------
def ref_singles(name, path, rows):
    def compute():
        R = Ref()
        h = R.load(path)
        try:
            return [single(R.fn, h, w, hy, cap) for w, hy, cap in rows]
        finally:
            R.free(h)
    return bfutil.reference_answers("word_hyphenation_" + name, compute)


def ref_texts(name, path, words, hys=(0x2D,)):
    """{uHy: [text per word]} (JSON keys are strings)"""
    def compute():
        R = Ref()
        h = R.load(path)
        try:
            return {str(hy): texts_of(R.fn, h, words, hy) for hy in hys}
        finally:
            R.free(h)
    return bfutil.reference_answers("word_hyphenation_" + name, compute)


def pack_texts(texts):
    flat = np.frombuffer("".join(texts).encode("latin-1"), dtype=np.uint8)
    off = np.zeros(len(texts) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in texts], out=off[1:])
    return flat, off

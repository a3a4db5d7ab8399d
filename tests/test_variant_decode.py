"""The integer of BfSetVariant -> named knobs (blingfire_amd/csrc/bf_variant.h), on the host.  The integers are a fixed interface: tests, tools
and bench.py pass them hand-built.  The layout they rely on is stated here a second time, as plain shifts and widths, and the header's decode
functions (tests/hosttest/bf_varianttest.cpp) are held to it: literal cases for every integer the repository itself passes, then a sweep of
every value of every field with the other bits random."""
import ctypes

import numpy as np
import pytest

import bfutil

NF = 32


@pytest.fixture(scope="module")
def V():
    L = ctypes.CDLL(bfutil.HOSTTEST_LIB)
    L.bft_variant_fields.restype = ctypes.c_char_p
    L.bft_variant_decode.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    L.bft_variant_needs_experiments.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    L.bft_bpe_wave_entry.argtypes = [ctypes.c_int, ctypes.c_void_p]
    L.bft_bpe_wave_tune.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.bft_bpe_wave_home.argtypes = [ctypes.c_int, ctypes.c_int]
    names = L.bft_variant_fields().decode().split(",")
    assert len(names) == NF and len(set(names)) == NF

    class Lib:
        fields = names

        @staticmethod
        def decode(variants, words):
            v = np.ascontiguousarray(np.asarray(variants, dtype=np.int64).astype(np.uint32).view(np.int32))
            out = np.empty((len(v), NF), dtype=np.int32)
            L.bft_variant_decode(v.ctypes.data, len(v), 1 if words else 0, out.ctypes.data)
            return out

        @staticmethod
        def needs(variants, wordpiece):
            v = np.ascontiguousarray(np.asarray(variants, dtype=np.int64).astype(np.uint32).view(np.int32))
            out = np.empty(len(v), dtype=np.int32)
            L.bft_variant_needs_experiments(v.ctypes.data, len(v), 1 if wordpiece else 0, out.ctypes.data)
            return out

        @staticmethod
        def four(fn, *args):
            out = np.zeros(4, dtype=np.int32)
            fn(*args, out.ctypes.data)
            return tuple(int(x) for x in out)
        lib = L
    return Lib


# integer, words mode of the lane lexer, the path the repository uses it on, the fields that path reads
g1, g8 = 5 | (1 << 24) | (1 << 12), 5 | (1 << 24) | (8 << 12)
LITERAL = [
    (0, 0, "the wave program whatever the batch, Unigram cut form, BPE fused kernel",
     {"WpChoice.lane_only": 0, "WpChoice.flat_always": 0, "WpChoice.flat_by_size": 0, "WpWaveKnobs.grab": 0, "WpWaveKnobs.per_cu": 0, "BpeWaveKnobs.off": 0, "BpeWaveKnobs.tune": 0,
      "SegKnobs.per_doc_kernels": 0, "SegKnobs.no_local": 0, "SegKnobs.write_arcs": 0, "SegKnobs.cut_off": 0, "SegKnobs.cut_unroll2": 0, "SegKnobs.quick_or_one_kernel": 0,
      "SegKnobs.tune": 0, "SegKnobs.per_cu_cap": 0, "SpPrepKnobs.old_form": 0, "SpPrepKnobs.waves": 0, "LaneLexKnobs.ev_thresh": 0, "LaneLexKnobs.per_cu": 0}),
    (2, 0, "WordPiece: the lane kernels for every model; BPE: the per-document kernels",
     {"WpChoice.lane_only": 1, "WpChoice.flat_always": 0, "WpChoice.flat_by_size": 0, "SegKnobs.per_doc_kernels": 1, "SegKnobs.no_local": 0, "SegKnobs.write_arcs": 0, "SegKnobs.cut_off": 0,
      "LaneLexKnobs.ev_thresh": 0, "LaneLexKnobs.fetch_thresh": 0, "LaneLexKnobs.votes": 0, "LaneLexKnobs.per_cu": 0}),
    (3, 0, "the default of every handle",
     {"WpChoice.lane_only": 0, "WpChoice.flat_always": 0, "WpChoice.flat_by_size": 1, "WpWaveKnobs.grab": 0, "WpWaveKnobs.per_cu": 0, "WpFlatKnobs.per_cu": 0, "WpFlatKnobs.waves_per_simd": 0,
      "WpFlatKnobs.dbg": 0, "WpUnitsKnobs.per_cu": 0, "WpUnitsKnobs.cfg": 0, "BpeWaveKnobs.off": 0, "BpeWaveKnobs.tune": 0, "BpeWaveKnobs.no_word_table": 0, "SpPrepKnobs.old_form": 0,
      "SpPrepKnobs.waves": 0, "SegKnobs.per_doc_kernels": 0, "SegKnobs.no_local": 0, "SegKnobs.write_arcs": 0, "SegKnobs.cut_off": 0, "SegKnobs.cut_unroll2": 0,
      "SegKnobs.quick_or_one_kernel": 0, "SegKnobs.tune": 0, "SegKnobs.per_cu_cap": 0, "WordsKnobs.no_long": 0, "WordsKnobs.thresh_k": 0, "WordsKnobs.small_triples": 0,
      "WordsKnobs.chunks_40": 0, "WordsKnobs.two_level_from_256": 0}),
    (4, 0, "WordPiece: the flat program for every batch; BPE: without the lane-local solve",
     {"WpChoice.lane_only": 0, "WpChoice.flat_always": 1, "WpChoice.flat_by_size": 0, "SegKnobs.per_doc_kernels": 0, "SegKnobs.no_local": 1, "SegKnobs.write_arcs": 0, "SegKnobs.cut_off": 0}),
    (5, 0, "WordPiece: never the flat program; BPE: the instances that write the arc lists",
     {"WpChoice.lane_only": 0, "WpChoice.flat_always": 0, "WpChoice.flat_by_size": 0, "SegKnobs.per_doc_kernels": 0, "SegKnobs.no_local": 0, "SegKnobs.write_arcs": 1, "SegKnobs.cut_off": 0}),
    (6, 0, "Unigram: the forward / backward kernels in place of the cut form",
     {"WpChoice.lane_only": 0, "WpChoice.flat_always": 0, "WpChoice.flat_by_size": 0, "SegKnobs.per_doc_kernels": 0, "SegKnobs.no_local": 0, "SegKnobs.write_arcs": 0, "SegKnobs.cut_off": 1,
      "SegKnobs.cut_unroll2": 0, "SegKnobs.quick_or_one_kernel": 0}),
    (3 | 0x40, 0, "BPE without its wave program: the lane kernels as shipped",
     {"BpeWaveKnobs.off": 1, "SegKnobs.per_doc_kernels": 0, "SegKnobs.no_local": 0, "SegKnobs.write_arcs": 0, "SegKnobs.tune": 0, "SegKnobs.per_cu_cap": 0, "WpChoice.flat_by_size": 0,
      "WpChoice.flat_always": 0, "WpChoice.lane_only": 0}),
    (3 | 0x80, 0, "the byte-per-lane prologue", {"SpPrepKnobs.old_form": 1, "SpPrepKnobs.waves": 0, "BpeWaveKnobs.off": 0, "SegKnobs.cut_off": 0, "SegKnobs.per_doc_kernels": 0}),
    (3 | 0x100000, 0, "the BPE wave program without the word table", {"BpeWaveKnobs.off": 0, "BpeWaveKnobs.tune": 0, "BpeWaveKnobs.no_word_table": 1}),
    (3 | (8 << 8), 0, "the in-order form of the BPE wave program", {"BpeWaveKnobs.off": 0, "BpeWaveKnobs.tune": 8, "BpeWaveKnobs.no_word_table": 0, "SegKnobs.tune": 8}),
    (3 | (8 << 8) | 0x100000, 0, "the in-order form without the word table", {"BpeWaveKnobs.off": 0, "BpeWaveKnobs.tune": 8, "BpeWaveKnobs.no_word_table": 1}),
    (3 | (9 << 8), 0, "the HOME form, units phase to 48", {"BpeWaveKnobs.off": 0, "BpeWaveKnobs.tune": 9, "BpeWaveKnobs.no_word_table": 0}),
    (3 | (6 << 24), 0, "the prologue compiled for six waves", {"SpPrepKnobs.old_form": 0, "SpPrepKnobs.waves": 6, "BpeWaveKnobs.off": 0, "BpeWaveKnobs.tune": 0}),
    (3 | (7 << 24), 0, "the prologue compiled for seven waves", {"SpPrepKnobs.old_form": 0, "SpPrepKnobs.waves": 7, "BpeWaveKnobs.off": 0, "BpeWaveKnobs.tune": 0}),
    (3 | (8 << 12), 0, "the wave program, eight documents per grab", {"WpChoice.flat_by_size": 1, "WpWaveKnobs.grab": 8, "WpWaveKnobs.per_cu": 0, "WpUnitsKnobs.cfg": 0, "WpFlatKnobs.waves_per_simd": 0}),
    (g1, 0, "the wave program, one workgroup per CU, one document per grab",
     {"WpChoice.lane_only": 0, "WpChoice.flat_always": 0, "WpChoice.flat_by_size": 0, "WpWaveKnobs.grab": 1, "WpWaveKnobs.per_cu": 1}),
    (g8, 0, "the wave program, one workgroup per CU, eight documents per grab",
     {"WpChoice.lane_only": 0, "WpChoice.flat_always": 0, "WpChoice.flat_by_size": 0, "WpWaveKnobs.grab": 8, "WpWaveKnobs.per_cu": 1}),
    (1 << 12, 1, "words modes: long documents from 16 characters",
     {"WordsKnobs.no_long": 0, "WordsKnobs.thresh_k": 1, "WordsKnobs.small_triples": 0, "WordsKnobs.chunks_40": 0, "WordsKnobs.two_level_from_256": 0,
      "LaneLexKnobs.ev_thresh": 0, "LaneLexKnobs.fetch_thresh": 0, "LaneLexKnobs.votes": 0, "LaneLexKnobs.per_cu": 0}),
    (0x40000000, 1, "words modes: no long-document path",
     {"WordsKnobs.no_long": 1, "WordsKnobs.thresh_k": 0, "WordsKnobs.small_triples": 0, "WordsKnobs.chunks_40": 0, "WordsKnobs.two_level_from_256": 0,
      "LaneLexKnobs.ev_thresh": 0, "LaneLexKnobs.fetch_thresh": 0, "LaneLexKnobs.votes": 0, "LaneLexKnobs.per_cu": 0}),
    (0x10000000 | (3 << 12), 1, "words modes: room for 40 chunks, long from 64 characters",
     {"WordsKnobs.no_long": 0, "WordsKnobs.thresh_k": 3, "WordsKnobs.small_triples": 0, "WordsKnobs.chunks_40": 1, "WordsKnobs.two_level_from_256": 0,
      "LaneLexKnobs.ev_thresh": 0, "LaneLexKnobs.fetch_thresh": 0, "LaneLexKnobs.votes": 0, "LaneLexKnobs.per_cu": 0}),
    (0x08000000 | (1 << 12), 1, "words modes: the two-level chain from 256 cells",
     {"WordsKnobs.no_long": 0, "WordsKnobs.thresh_k": 1, "WordsKnobs.small_triples": 0, "WordsKnobs.chunks_40": 0, "WordsKnobs.two_level_from_256": 1,
      "LaneLexKnobs.ev_thresh": 0, "LaneLexKnobs.fetch_thresh": 0, "LaneLexKnobs.votes": 0, "LaneLexKnobs.per_cu": 0}),
    (0x20000000 | 0x40000000, 1, "words modes: the small triple buffer on lanes alone",
     {"WordsKnobs.no_long": 1, "WordsKnobs.thresh_k": 0, "WordsKnobs.small_triples": 1, "WordsKnobs.chunks_40": 0, "WordsKnobs.two_level_from_256": 0,
      "LaneLexKnobs.ev_thresh": 0, "LaneLexKnobs.fetch_thresh": 0, "LaneLexKnobs.votes": 0, "LaneLexKnobs.per_cu": 0}),
    (0x28000000 | (1 << 12), 1, "words modes: the small triple buffer in the two-level chain",
     {"WordsKnobs.no_long": 0, "WordsKnobs.thresh_k": 1, "WordsKnobs.small_triples": 1, "WordsKnobs.chunks_40": 0, "WordsKnobs.two_level_from_256": 1,
      "LaneLexKnobs.ev_thresh": 0, "LaneLexKnobs.fetch_thresh": 0, "LaneLexKnobs.votes": 0, "LaneLexKnobs.per_cu": 0}),
    (0x10000000 | (1 << 12), 1, "words modes: room for 40 chunks, long from 16 characters", {"WordsKnobs.no_long": 0, "WordsKnobs.thresh_k": 1, "WordsKnobs.chunks_40": 1, "LaneLexKnobs.ev_thresh": 0, "LaneLexKnobs.per_cu": 0}),
    (0x08000000, 1, "words modes: the two-level chain from 256 cells, threshold by batch", {"WordsKnobs.thresh_k": 0, "WordsKnobs.two_level_from_256": 1, "LaneLexKnobs.ev_thresh": 0, "LaneLexKnobs.per_cu": 0}),
    (0x20000000, 1, "words modes: the small triple buffer", {"WordsKnobs.no_long": 0, "WordsKnobs.thresh_k": 0, "WordsKnobs.small_triples": 1, "LaneLexKnobs.ev_thresh": 0, "LaneLexKnobs.per_cu": 0}),
    (0x20000000 | (1 << 12), 1, "words modes: the small triple buffer, long from 16 characters", {"WordsKnobs.thresh_k": 1, "WordsKnobs.small_triples": 1, "LaneLexKnobs.ev_thresh": 0, "LaneLexKnobs.per_cu": 0}),
    # the Unigram cut form: periods, the short way out, two transitions per trip, fewer waves per CU
    (3 | (1 << 8), 0, "Unigram cut form, period 1", {"SegKnobs.cut_off": 0, "SegKnobs.cut_unroll2": 0, "SegKnobs.quick_or_one_kernel": 0, "SegKnobs.tune": 1, "SegKnobs.per_cu_cap": 0}),
    (3 | (2 << 8), 0, "Unigram cut form, period 2", {"SegKnobs.cut_off": 0, "SegKnobs.cut_unroll2": 0, "SegKnobs.quick_or_one_kernel": 0, "SegKnobs.tune": 2, "SegKnobs.per_cu_cap": 0}),
    (3 | (64 << 8), 0, "Unigram cut form, period 64", {"SegKnobs.cut_off": 0, "SegKnobs.cut_unroll2": 0, "SegKnobs.quick_or_one_kernel": 0, "SegKnobs.tune": 64, "SegKnobs.per_cu_cap": 0}),
    (3 | 0x20, 0, "Unigram cut form, the short way out", {"SegKnobs.cut_off": 0, "SegKnobs.cut_unroll2": 0, "SegKnobs.quick_or_one_kernel": 1, "SegKnobs.tune": 0, "SegKnobs.per_cu_cap": 0}),
    (3 | 0x20 | (1 << 8), 0, "Unigram cut form, the short way out, period 1", {"SegKnobs.cut_off": 0, "SegKnobs.cut_unroll2": 0, "SegKnobs.quick_or_one_kernel": 1, "SegKnobs.tune": 1}),
    (3 | 0x10, 0, "Unigram cut form, two transitions per trip", {"SegKnobs.cut_off": 0, "SegKnobs.cut_unroll2": 1, "SegKnobs.quick_or_one_kernel": 0, "SegKnobs.tune": 0, "SegKnobs.per_cu_cap": 0}),
    (3 | (10 << 16), 0, "Unigram cut form, ten waves per CU", {"SegKnobs.cut_off": 0, "SegKnobs.cut_unroll2": 0, "SegKnobs.quick_or_one_kernel": 0, "SegKnobs.tune": 0, "SegKnobs.per_cu_cap": 10}),
    (3 | (13 << 16) | 0x20, 0, "Unigram cut form, thirteen waves per CU, the short way out", {"SegKnobs.cut_off": 0, "SegKnobs.quick_or_one_kernel": 1, "SegKnobs.tune": 0, "SegKnobs.per_cu_cap": 13}),
    # the same integers left on a WordPiece handle for a later TextToIds call (the known overlap): the lane lexer and the wave program see the bits
    (1 << 12, 0, "ids after a words threshold", {"LaneLexKnobs.ev_thresh": 0x10, "LaneLexKnobs.per_cu": 0, "WpWaveKnobs.grab": 1, "WpWaveKnobs.per_cu": 0}),
    (0x28000000 | (1 << 12), 0, "ids after the words test knobs", {"LaneLexKnobs.ev_thresh": 0x10, "LaneLexKnobs.per_cu": 0x28, "WpWaveKnobs.grab": 1, "WpWaveKnobs.per_cu": 0x28}),
]


@pytest.mark.parametrize("variant,words,path,want", LITERAL, ids=["%#x-%s" % (c[0], "words" if c[1] else "ids") for c in LITERAL])
def test_literal_integers(V, variant, words, path, want):
    row = V.decode([variant], words)[0]
    got = {name: int(row[V.fields.index(name)]) for name in want}
    assert got == want, path


# The layout, stated independently of the header: (field, shift, width, equals).  equals None: the field is the bits themselves; a number: the
# field is "these bits are that number".  In the words modes the lane lexer decodes the integer without bits 12..15 and 27..30.
TABLE = [
    ("WpChoice.lane_only", 0, 8, 2), ("WpChoice.flat_always", 0, 8, 4), ("WpChoice.flat_by_size", 0, 8, 3),
    ("WpWaveKnobs.grab", 12, 4, None), ("WpWaveKnobs.per_cu", 24, 6, None),
    ("WpFlatKnobs.per_cu", 24, 6, None), ("WpFlatKnobs.waves_per_simd", 16, 4, None), ("WpFlatKnobs.dbg", 20, 4, None),
    ("WpUnitsKnobs.per_cu", 24, 6, None), ("WpUnitsKnobs.cfg", 8, 4, None),
    ("LaneLexKnobs.ev_thresh", 8, 8, None), ("LaneLexKnobs.fetch_thresh", 16, 4, None), ("LaneLexKnobs.votes", 20, 4, None), ("LaneLexKnobs.per_cu", 24, 6, None),
    ("WordsKnobs.no_long", 30, 1, None), ("WordsKnobs.thresh_k", 12, 4, None), ("WordsKnobs.small_triples", 29, 1, None), ("WordsKnobs.chunks_40", 28, 1, None),
    ("WordsKnobs.two_level_from_256", 27, 1, None),
    ("SpPrepKnobs.old_form", 7, 1, None), ("SpPrepKnobs.waves", 24, 4, None),
    ("BpeWaveKnobs.off", 6, 1, None), ("BpeWaveKnobs.tune", 8, 4, None), ("BpeWaveKnobs.no_word_table", 20, 1, None),
    ("SegKnobs.per_doc_kernels", 0, 8, 2), ("SegKnobs.no_local", 0, 8, 4), ("SegKnobs.write_arcs", 0, 8, 5), ("SegKnobs.cut_off", 0, 8, 6),
    ("SegKnobs.cut_unroll2", 4, 1, None), ("SegKnobs.quick_or_one_kernel", 5, 1, None), ("SegKnobs.tune", 8, 8, None), ("SegKnobs.per_cu_cap", 16, 8, None),
]
WORDS_REMOVED = 0x7800F000
DRAWS = 200


def _expect(v, words):
    """v: uint32 array -> [len(v), NF] by TABLE"""
    out = np.empty((len(v), NF), dtype=np.int32)
    for col, (name, shift, width, equals) in enumerate(TABLE):
        src = v & np.uint32(~WORDS_REMOVED & 0xffffffff) if words and name.startswith("LaneLexKnobs.") else v
        bits = (src >> np.uint32(shift)) & np.uint32((1 << width) - 1)
        out[:, col] = bits if equals is None else (bits == equals)
    return out


def _draws():
    """for every field of TABLE: every value of its bits, DRAWS times each, all other bits (bit 31 too) from a seeded generator"""
    rng = np.random.default_rng(20240607)
    for name, shift, width, _ in TABLE:
        vals = np.repeat(np.arange(1 << width, dtype=np.uint32), DRAWS)
        mask = np.uint32(((1 << width) - 1) << shift)
        other = rng.integers(0, 1 << 32, size=len(vals), dtype=np.uint64).astype(np.uint32)
        yield name, (other & ~mask) | (vals << np.uint32(shift))


def test_sweep_every_field_against_the_shift_table(V):
    assert [t[0] for t in TABLE] == V.fields
    for name, v in _draws():
        for words in (0, 1):
            got, want = V.decode(v, words), _expect(v, words)
            bad = np.argwhere(got != want)
            assert len(bad) == 0, "sweep of %s, words %d: variant %#x field %s: %d, the table says %d" % (
                name, words, v[bad[0][0]], V.fields[bad[0][1]], got[tuple(bad[0])], want[tuple(bad[0])])


def test_needs_experiments_rule(V):
    for name, v in _draws():
        assert np.array_equal(V.needs(v, True), ((v & np.uint32(0x00FF0F00)) != 0).astype(np.int32)), name
        assert np.array_equal(V.needs(v, False), ((v & np.uint32(0x0F000000)) != 0).astype(np.int32)), name


# tune -> (transitions per round, the units phase ends below, HOME form, BF_EXPERIMENTS builds only): the instances launch_bpe_wave has carried
BPE_WAVE_INSTANCES = {0: (4, 32, 1, 0), 1: (4, 16, 0, 1), 2: (4, 4, 0, 1), 3: (4, 48, 0, 1), 6: (6, 32, 0, 1), 8: (4, 32, 0, 0), 9: (4, 48, 1, 0), 10: (3, 32, 1, 0), 11: (4, 60, 1, 0)}
SHIPPED = (4, 32, 1, 0)


def test_bpe_wave_tune_table(V):
    for tune in range(16):
        entry = V.four(V.lib.bft_bpe_wave_entry, tune)
        assert entry == BPE_WAVE_INSTANCES.get(tune, SHIPPED), tune            # a value without an instance is the shipped one
        for exp in (0, 1):
            runs = V.four(V.lib.bft_bpe_wave_tune, tune, exp)
            assert runs == (SHIPPED if entry[3] and not exp else entry), (tune, exp)
            # the tail follows the kernel: HOME is reported of the instance that runs
            assert V.lib.bft_bpe_wave_home(tune, exp) == runs[2], (tune, exp)
    assert [t for t in range(16) if not V.lib.bft_bpe_wave_home(t, 0)] == [8]
    assert [t for t in range(16) if not V.lib.bft_bpe_wave_home(t, 1)] == [1, 2, 3, 6, 8]

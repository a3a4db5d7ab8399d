"""CPU tier of the call-order tests (tests/order_cases.py, tests/test_gpu_call_order.py): the order visits every ordered pair of steps exactly once,
and the inputs of the steps do what they are for -- proven with the checkers alone, no GPU and not one call into the library under test."""
import numpy as np
import pytest

import bfutil
import flat_cases
import order_cases as oc

KINDS = list(oc.BUILDERS)


@pytest.fixture(scope="module", params=KINDS)
def cat(request):
    c = oc.catalogue(request.param)
    if c is None:
        pytest.skip("the model of the %s catalogue is not present" % request.param)
    return c


def by_name(cat):
    return {s.name: s for s in cat.steps}


@pytest.mark.parametrize("n", range(1, 41))
def test_circuit_has_every_ordered_pair_exactly_once(n):
    for seed in (0, 1, n + 3):
        seq = oc.circuit(n, seed)
        assert len(seq) == n * n + 1 and seq[0] == seq[-1] == seed % n
        pairs = list(zip(seq, seq[1:]))
        assert len(set(pairs)) == n * n and set(pairs) == {(a, b) for a in range(n) for b in range(n)}


def test_big_meets_the_flat_thresholds_and_mixes_document_kinds():
    text, off = oc.big_batch()
    nd = len(off) - 1
    assert nd >= oc.FLAT_MIN_DOCS and len(text) >= oc.FLAT_MIN_BYTES                   # use_flat takes it under the default variant
    assert nd < 2.5 * oc.FLAT_MIN_DOCS and len(text) < 1.2 * oc.FLAT_MIN_BYTES          # ... and it is no larger than that needs
    assert nd % 64 and nd % 4
    docs = flat_cases.docs_of((text, off))
    assert b"" in docs                                                                  # an empty document
    # handed back: a run of more than WF_RUN_MAX bytes without white space or punctuation (tests/test_flat_emu.py test_handed_back)
    assert oc.HANDED_BACK in docs and len(oc.HANDED_BACK.split()[0]) > flat_cases.WF_RUN_MAX and oc.HANDED_BACK.split()[0].isalpha()
    # invalid: bytes of it, no id of it (the reference answers 0 for invalid UTF-8)
    model = bfutil.bert_model_name()
    ids, _, _, ido = oc.ids_answer(model, "big", oc.WP_PAIR)
    d = docs.index(oc.INVALID)
    assert len(docs[d]) > 0 and ido[d + 1] == ido[d]
    with pytest.raises(UnicodeDecodeError):
        docs[d].decode("utf-8")
    assert len(ids) == ido[-1] > nd


def test_small_is_under_the_mapped_limits():
    text, off = oc.small_batch()
    nd = len(off) - 1
    assert nd == 37 and nd <= oc.SMALL_MAX_DOCS and len(text) <= oc.SMALL_MAX_BYTES and len(text) < 8192
    assert nd % 64 and nd % 4
    assert off[-1] > off[-2], "the last document must have bytes: the bad-range steps make it the bad one"


def test_every_catalogue_is_complete(cat):
    names = [s.name for s in cat.steps]
    assert len(set(names)) == len(names) >= 6
    for s in cat.steps:
        assert s.size in ("big", "small") and s.why.startswith("status %d:" % s.status), (s.name, s.why)
        assert s.status in (0, 1, 8) or (s.status == 4 and cat.kind == "i2w"), s.name
        for w in s.want:
            assert not w.array.flags.writeable
    assert any(s.size == "big" for s in cat.steps) and any(s.size == "small" for s in cat.steps)
    if cat.kind in ("wordpiece", "unigram", "bpe"):
        assert any(s.status == 1 for s in cat.steps)
    if cat.kind in ("wordpiece", "w2h"):
        assert any(s.status == 8 for s in cat.steps)


def test_wordpiece_catalogue_has_the_steps_of_the_matrix():
    cat = oc.catalogue("wordpiece")
    if cat is None:
        pytest.skip("no WordPiece model")
    names = set(by_name(cat))
    for program in ("flat", "wave", "lane"):
        for size in ("big", "small"):
            for what in ("ids", "offsets"):
                assert "%s %s %s" % (program, size, what) in names
    assert len(cat.steps) >= 30


def test_overflow_caps_lie_between_the_first_document_and_the_total():
    for kind in ("wordpiece", "unigram", "bpe"):
        cat = oc.catalogue(kind)
        if cat is None:
            continue
        step = next(s for s in cat.steps if s.status == 1)
        ids, ido = step.want[0], step.want[-1].array
        cap = len(ids.array) - oc.TAIL
        first = int(ido[ido > 0][0])
        assert first < cap < ido[-1] and cap in ido, (kind, first, cap, int(ido[-1]))
        assert (ids.array[cap:] == -7).all() and (ids.array[:cap] != -7).all()


def test_long_path_steps_hold_a_long_document_and_no_long_steps_switch_the_path_off():
    cat = oc.catalogue("wordpiece")
    if cat is None:
        pytest.skip("no WordPiece model")
    steps = by_name(cat)
    for name in ("words big", "sentences small"):
        text, off = oc.batch(steps[name].size)
        assert int(np.diff(off).max()) > oc.long_threshold(len(text)), name            # long_caps: thresh = max(16, total_bytes / 24,000)
    # the no_long steps: the knob is bit 30 of the variant they set, and long_caps() answers "no long documents" for it whatever the batch holds --
    # no document of theirs matters to the long-document path
    assert oc.NO_LONG == 0x40000000 and "words small no_long" in steps and "sentences big no_long" in steps


def test_bad_range_steps_leave_every_other_document_its_answer():
    cat = oc.catalogue("wordpiece")
    if cat is None:
        pytest.skip("no WordPiece model")
    step = by_name(cat)["small bad range"]
    _, _, _, ido = oc.ids_answer(bfutil.bert_model_name(), "small", oc.WP_PAIR)
    got = step.want[-1].array
    assert step.status == 8 and np.array_equal(got[:-1], ido[:-1]) and got[-1] == got[-2] and ido[-1] > ido[-2]
    text, off = oc.small_batch()
    bad = oc.bad_range_offsets(off)
    assert bad[-1] > len(text) and np.array_equal(bad[:-1], off[:-1])


def test_row_stage_steps_have_windows_and_an_empty_sequence(cat):
    seen = 0
    for s in cat.steps:
        offs = [w.array for w in s.want if w.label == "row offsets"]
        if not offs:
            continue
        seen += 1
        rows_per_item = np.diff(offs[0])
        L = next(w.where[1] for w in s.want if w.label == "rows")
        rows = next(w.array for w in s.want if w.label == "rows")
        rows = rows[len(rows) - oc.TAIL - int(offs[0][-1]) * L:len(rows) - oc.TAIL].reshape(-1, L)       # (a narrow step has one sentinel entry in front)
        real = (rows != oc.PAD).sum(axis=1)
        starts = offs[0][:-1]
        if "one row" in s.name:
            assert (real == L).any(), s.name                                           # a sequence that fills its row: it was longer than the body, or as long
        else:
            assert (rows_per_item > 1).any(), s.name                                   # a sequence of more than one window
        if hasattr(s, "off_b"):
            assert (np.diff(s.off_b) == 0).any(), s.name                               # a pair whose context is empty
        else:
            assert (real[starts] == 2).any(), s.name                                   # an empty sequence: [CLS] [SEP] and padding
    assert seen >= 1
    if cat.kind == "wordpiece":
        model = bfutil.bert_model_name()
        for size in ("big", "small"):
            ido = oc.ids_answer(model, size, oc.WP_PAIR)[3]
            for L in oc.ROW_LENS:
                assert oc.row_geometry_ok(ido, L), (size, L)

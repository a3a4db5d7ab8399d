"""CPU tier of the call-order tests (tests/order_cases.py, tests/test_gpu_call_order.py): the order visits every ordered pair of steps exactly once,
and the inputs of the steps do what they are for -- proven with the checkers and the restatements alone, no GPU and not one call into the library
under test.  For the model-input steps that means: rows that several sequences share, planes that hold their fill, a sequence split at a row's edge,
a rows_cap that cuts, a bad range that empties one sequence and moves no other, a cap on the predictions that binds in some rows and not in
others, a whole word selected, a denoise step that truncates some rows and not all, no span across an eos -- and the array form of the stream
restatement held to the sequential one on every small step."""
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


# ---- the model-input steps (the "inputs" catalogue, and the two of them the i2w catalogue has)
def inputs_cat():
    c = oc.catalogue("inputs")
    if c is None:
        pytest.skip("no WordPiece model")
    return c


def body_of(want, L, lead=0):
    """the [R, L] cells of a row output in front of its sentinel tail (and behind `lead` sentinel entries)"""
    a = want.array[lead:len(want.array) - oc.TAIL]
    return a.reshape(-1, L)


def test_inputs_catalogue_has_the_eighteen_steps():
    cat = inputs_cat()
    assert [s.name for s in cat.steps] == [
        "wave small offsets", "flat big ids", "TextToIdsBatch small", "packed L=12 small", "packed planes L=12 big", "packed planes L=64 small, narrow",
        "packed planes host L=12 small", "rows planes host L=12 small", "stream L=64 big", "stream L=13 small", "stream L=12 small overflow", "stream small bad range",
        "stream host L=12 small", "mlm mask L=64 small", "mlm predictions L=12 small", "mlm predictions max_pred=0 L=12 small", "denoise L=64 small",
        "denoise L=12 small, truncated"]
    assert sum(s.size == "big" for s in cat.steps) == 3 and len(oc.circuit(len(cat.steps))) == 325
    assert sorted(s.status for s in cat.steps if s.status) == [1, 1, 8]
    i2w = oc.catalogue("i2w")
    if i2w is not None:
        names = by_name(i2w)
        assert len(i2w.steps) == 10 and len(oc.circuit(10)) == 101
        assert names["stream L=12 small"].status == 0 and names["denoise L=12 small, truncated"].status == 1 and any(s.status == 4 for s in i2w.steps)


def test_packed_planes_steps_share_rows_and_hold_the_fill():
    steps = [s for s in inputs_cat().steps if hasattr(s, "plane_lead")]
    assert [s.name for s in steps] == ["packed planes L=12 big", "packed planes L=64 small, narrow", "packed planes host L=12 small"]
    for s in steps:
        first = next(w.array for w in s.want if w.label == "row_first_seq")
        first = first[:len(first) - oc.TAIL]
        assert (np.diff(first) >= 2).any(), s.name                                     # a row that holds at least two sequences
        rows = body_of(next(w for w in s.want if w.label == "packed rows"), s.L)
        planes = [w for w in s.want if w.label.startswith("plane ")]
        assert len(planes) == s.taken == 2
        for k, w in enumerate(planes):
            lead = s.plane_lead if k == 0 else 0
            assert w.where[:2] == ("rows", s.L) and (w.where[2] if len(w.where) > 2 else 0) == lead and (w.array[:lead] == -7).all()
            p = body_of(w, s.L, lead)
            assert p.shape == rows.shape
            holds_id = ~np.isin(rows, (oc.CLS, oc.SEP, oc.PAD))
            assert (p[~holds_id] == s.fill[k]).all() and (~holds_id).any() and (p[holds_id] >= 0).all() and holds_id.any(), (s.name, k)
    narrow = steps[1]
    assert narrow.plane_lead == 1 and (4 * narrow.plane_lead) % 16 == 4 and len(narrow.fill) == 3 and narrow.taken == 2      # plane 0 at 4 mod 16; a third slot whose out is NULL
    assert steps[0].plane_lead == 0 and steps[0].L % 4 == 0                            # the wide form: every plane aligned, row_len a multiple of 4


def stream_steps(cat):
    return [s for s in cat.steps if hasattr(s, "stream")]


@pytest.mark.parametrize("kind", ["inputs", "i2w"])
def test_stream_steps_split_a_sequence_and_the_array_form_is_the_sequential_one(kind):
    import stream_cases
    cat = oc.catalogue(kind)
    if cat is None:
        pytest.skip("the model of the %s catalogue is not present" % kind)
    steps = stream_steps(cat)
    assert len(steps) == (5 if kind == "inputs" else 1)
    for s in steps:
        sp = s.stream
        ids, off, L = sp["ids"], sp["off"], sp["L"]
        ans = oc.stream_answer(ids, off, L, sp["bos"], sp["eos"], sp["flags"])
        if s.size == "small":
            seq = stream_cases.restate(ids, off, L, sp["bos"], sp["eos"], oc.PAD, oc.IGN, sp["flags"], ids_len=len(ids), rows_cap=sp["rows_cap"])
            assert stream_cases.same(ans[:10] + (ans[10] | (1 if sp["R"] > sp["rows_cap"] else 0),), seq), s.name
            assert seq[10] == s.status
        R, T = sp["R"], sp["T"]
        n = np.diff(off)
        assert (n == 0).any(), s.name                                                  # an empty sequence
        w = np.where((n < 0) | (off[1:] > len(ids)), 0, n) + (sp["bos"] >= 0) + (sp["eos"] >= 0)
        W = np.concatenate([[0], np.cumsum(w)])
        assert T == W[-1] and ((W[:-1] // L < (W[1:] - 1) // L) & (w > 0) & (w <= L)).any(), s.name      # a sequence no longer than a row, split at a row's edge
        if sp["flags"] & stream_cases.DROP_LAST:
            assert R * L <= T and R == T // L and T % L, s.name                        # (the dropped tail is not empty)
        else:
            assert R * L > T, s.name                                                   # the last row has padding
    if kind == "inputs":
        by = by_name(cat)
        assert by["stream L=64 big"].stream["flags"] == 0 and by["stream L=64 big"].stream["bos"] >= 0 and by["stream L=64 big"].stream["eos"] >= 0
        drop = by["stream L=13 small"].stream
        assert drop["flags"] == stream_cases.DROP_LAST | stream_cases.LABELS_WITHIN and drop["bos"] < 0 and drop["L"] % 4


def test_stream_overflow_step_writes_nothing_at_or_past_rows_cap():
    s = by_name(inputs_cat())["stream L=12 small overflow"]
    sp = s.stream
    cap, R, L = sp["rows_cap"], sp["R"], sp["L"]
    assert 0 < cap < R and s.status == 1
    full = oc.stream_answer(sp["ids"], sp["off"], L, sp["bos"], sp["eos"], sp["flags"])
    for w, a in zip(s.want[:4], full[:4]):
        assert len(w.array) == cap * L + oc.TAIL and (w.array[cap * L:] == -7).all() and np.array_equal(w.array[:cap * L], a.reshape(-1)[:cap * L]), w.label
    for w, a in zip(s.want[4:6], full[4:6]):
        assert len(w.array) == cap + oc.TAIL and (w.array[cap:] == -7).all() and np.array_equal(w.array[:cap], a[:cap]), w.label
    for w, a in zip(s.want[6:8], full[6:8]):
        assert np.array_equal(w.array[:len(a)], a), w.label                            # the per-sequence outputs are complete
    assert (full[6] >= cap).any()                                                      # ... sequences that begin in a dropped row too
    assert s.want[8].array[:2].tolist() == [R, sp["T"]]


def test_stream_bad_range_step_empties_one_sequence_and_moves_no_other():
    cat = inputs_cat()
    s, good = by_name(cat)["stream small bad range"], by_name(cat)["stream host L=12 small"]
    sp, gp = s.stream, good.stream
    assert s.status == 8 and sp["ids"] is gp["ids"] and (sp["L"], sp["bos"], sp["eos"], sp["flags"]) == (gp["L"], gp["bos"], gp["eos"], gp["flags"])
    bad = (sp["off"][:-1] < 0) | (sp["off"][1:] < sp["off"][:-1]) | (sp["off"][1:] > len(sp["ids"]))
    assert bad.sum() == 1 and bad[-1] and gp["off"][-1] > gp["off"][-2] and np.array_equal(sp["off"][:-1], gp["off"][:-1])
    lost = int(gp["off"][-1] - gp["off"][-2])
    assert sp["T"] == gp["T"] - lost
    for k in (6, 7):                                                                   # seq_row, seq_col: the last one too, its unit begins where it began
        assert np.array_equal(s.want[k].array, good.want[k].array), s.want[k].label


def test_predictions_step_has_rows_the_cap_binds_in_and_a_whole_word():
    import mlm_cases
    import mlmcap_cases
    cat = inputs_cat()
    s, base = by_name(cat)["mlm predictions L=12 small"], by_name(cat)["mlm predictions max_pred=0 L=12 small"]
    m = s.mlm
    P = m["max_pred"]
    assert P == oc.PRED_CAP > 0 and base.mlm["max_pred"] == 0 and all(base.mlm[k] is m[k] for k in ("rows", "seg", "S", "E"))
    sel_kw = {k: m["kw"][k] for k in ("special_ids", "probs", "seed", "epoch")}
    h, selected, w3 = mlmcap_cases.selection(m["rows"], None, m["seg"], m["S"], m["E"], **sel_kw)
    per_row = selected.sum(axis=1)
    assert (per_row > P).any() and ((per_row > 0) & (per_row <= P)).any()              # the cap bites in some rows; others are below it and have predictions
    kept = mlmcap_cases.kept_loop(h, selected, w3, P)
    count = s.want[4].array[:len(per_row)]
    assert np.array_equal(count, kept.sum(axis=1)) and (count < per_row).any() and (count == per_row)[per_row > 0].any()
    assert any(selected[r, a:z + 1].all() for r, runs in enumerate(mlm_cases.unit_runs(h)) for a, z in runs)      # a whole word of at least two cells is selected
    assert any(kept[r, a:z + 1].all() for r, runs in enumerate(mlm_cases.unit_runs(h)) for a, z in runs)          # ... and one is kept
    assert (m["seg"].max(axis=1) >= 2).any()                                           # packed rows: a row of several sequences
    # max_pred == 0 is the base call: restate_mlm, which restate_cap agrees with
    w0 = mlmcap_cases.restate_cap(m["rows"], None, m["seg"], m["S"], m["E"], max_pred=0, **m["kw"])
    L = m["rows"].shape[1]
    assert len(base.want) == 2 and np.array_equal(body_of(base.want[0], L), w0[0]) and np.array_equal(body_of(base.want[1], L), w0[1])
    assert not np.array_equal(body_of(base.want[1], L), body_of(s.want[1], L))


@pytest.mark.parametrize("kind", ["inputs", "i2w"])
def test_denoise_steps_truncate_where_they_say_and_no_span_crosses_an_eos(kind):
    import denoise_cases
    cat = oc.catalogue(kind)
    if cat is None:
        pytest.skip("the model of the %s catalogue is not present" % kind)
    steps = [s for s in cat.steps if hasattr(s, "denoise")]
    assert [s.name for s in steps] == (["denoise L=64 small"] if kind == "inputs" else []) + ["denoise L=12 small, truncated"]
    for s in steps:
        d = s.denoise
        w, L, R = d["answer"], d["L"], len(d["rows"])
        ne, nd = w["enc_count"], w["dec_count"]
        nruns = np.array([len(x) for x in denoise_cases.runs_of(w["noise"])])
        assert not (w["noise"] & np.isin(d["rows"], (oc.SEP, oc.CLS, oc.PAD))).any() and (d["rows"] == oc.SEP).any()      # an eos cell is never noise: no run crosses it
        assert (d["seg"] == 0).any() and not w["present"][d["seg"] == 0].any()           # the padding of the last row is not present
        if s.status == 0:
            assert (d["enc_len"], d["dec_len"]) == (L, L + 2) and not (ne > d["enc_len"]).any() and not (nd > d["dec_len"]).any() and (nruns >= 2).any()
        else:
            lose = (ne > d["enc_len"]) | (nd > d["dec_len"])
            assert s.status == 1 and w["status"] == 1 and lose.any() and not lose.all() and d["dec_len"] == oc.DENOISE_TRUNCATED_DEC
        for want in s.want:                                                            # the rows behind *d_nrows keep the sentinel
            width = want.where[1] if want.where[0] == "rows" else 1
            assert len(want.array) == (R + oc.BEHIND_ROWS) * width + oc.TAIL and (want.array[R * width:] == -7).all() and (want.array[:R * width] != -7).all()
    if kind == "inputs":
        nine = by_name(cat)["stream L=64 big"].stream
        assert (nine["L"], nine["bos"], nine["eos"], nine["flags"]) == (64, oc.CLS, oc.SEP, 0)      # the denoise step's rows are those of this spec on the small batch
        assert np.array_equal(steps[0].denoise["rows"], oc.stream_rows(*oc.offsets_answer(bfutil.bert_model_name(), "small", oc.WP_PAIR)[::3], 64)[0])


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

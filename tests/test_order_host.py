"""CPU tier of the call-order tests (tests/order_cases.py, tests/test_gpu_call_order.py): the order visits every ordered pair of steps exactly once,
and the inputs of the steps do what they are for -- proven with the checkers and the restatements alone, no GPU and not one call into the library
under test.  For the model-input steps that means: rows that several sequences share, planes that hold their fill, a sequence split at a row's edge,
a rows_cap that cuts, a bad range that empties one sequence and moves no other, a cap on the predictions that binds in some rows and not in
others, a whole word selected, a denoise step that truncates some rows and not all, no span across an eos -- and the array form of the stream
restatement held to the sequential one on every small step.  For the `ragged` steps: a sort of more than one block, a cells_cap strictly inside a row
and a batches_cap below the count, the wide and the narrow alignment, a bad range that empties the last sequence alone; sequences over a MinHash
tile's edge, inside a tile and empty, a sig_cap that cuts, pairs that share some slots and not all; a text of several scan blocks with characters
of 2, 3 and 4 bytes, exactly one position beyond its document, the array form of the offsets restatement held to the sequential one; and the two
offsets programs of unigram and of bpe share one answer, object by object."""
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


# ---- the calls over ragged ids and text (the "ragged" catalogue), and the second offsets program of unigram and bpe
def ragged_cat():
    c = oc.catalogue("ragged")
    if c is None:
        pytest.skip("no WordPiece model")
    return c


def flat_of(want, n):
    """the first n entries of an output in front of its sentinel tail"""
    assert len(want.array) >= n + oc.TAIL
    return want.array[:n]


def test_ragged_catalogue_has_the_twenty_steps():
    cat = ragged_cat()
    assert [s.name for s in cat.steps] == [
        "wave small offsets", "flat big ids", "TextToIdsBatch small", "packed L=12 small", "stream L=64 big", "rows L=12 windows small",
        "bucketed max_len=64 big", "bucketed max_len=300 small, narrow, cut", "bucketed small bad range", "bucketed small, size query", "bucketed host small",
        "minhash H=64 r=4 k=5 big", "minhash H=65 k=2 small, cut", "minhash small bad range", "minhash host small", "minhash pairs small", "minhash pairs small, clean",
        "byte to char big, utf16", "char to byte small, one beyond", "byte to char small, units only"]
    assert sum(s.size == "big" for s in cat.steps) == 5 and len(cat.steps) <= 24 and len(oc.circuit(len(cat.steps))) == 401
    assert sorted(s.status for s in cat.steps if s.status) == [1, 1, 8, 8, 8, 8]
    # the inputs are those of the `inputs` catalogue: the checker's ids and byte offsets of the two batches
    model = bfutil.bert_model_name()
    si, ss, se, so = oc.offsets_answer(model, "small", oc.WP_PAIR)
    bi, bs, be, bo = oc.offsets_answer(model, "big", oc.WP_PAIR)
    for s in cat.steps:
        p = getattr(s, "bucketed", None) or getattr(s, "minhash", None)
        if p:
            assert p["ids"] is (bi if s.size == "big" else si) and (p["off"] is (bo if s.size == "big" else so) or s.status == 8), s.name
    big = by_name(cat)["byte to char big, utf16"].charpos
    assert big["starts"] is bs and big["ends"] is be and big["item_off"] is bo and big["text"] is oc.big_batch()[0]


def unit_of(ans, q):
    """the ids of sequence q's row in front of its padding: through seq_pos, the batch that holds the sorted position and the batch's first cell"""
    pos = int(ans["seq_pos"][q])
    b = int(np.searchsorted(ans["first"], pos, side="right")) - 1
    L = int(ans["len"][b])
    at = int(ans["cell"][b]) + (pos - int(ans["first"][b])) * L
    assert ans["order"][pos] == q and 0 <= b < ans["counts"][0] and at + L <= ans["counts"][1]
    return ans["rows"][at:at + L][ans["mask"][at:at + L] == 1]


def test_bucketed_steps_sort_in_blocks_cut_inside_a_row_and_empty_one_sequence():
    import bucketed_cases
    cat = ragged_cat()
    steps = [s for s in cat.steps if hasattr(s, "bucketed")]
    assert [s.name for s in steps] == ["bucketed max_len=64 big", "bucketed max_len=300 small, narrow, cut", "bucketed small bad range", "bucketed small, size query",
                                       "bucketed host small"]
    for s in steps:
        p = s.bucketed
        ans = bucketed_cases.restate(p["ids"], p["off"], p["max_len"], oc.CLS, oc.SEP, oc.PAD, p["multiple"], p["max_cells"])
        B, C = (int(x) for x in ans["counts"])
        assert s.status == (ans["status"] | int((C > p["cells_cap"] and not p["query"]) or B > p["batches_cap"])), s.name
        assert all(np.array_equal(ans[k], p["answer"][k]) for k in oc.BUCKET_OUTS), s.name
        assert (np.diff(p["answer"]["len"][:-1]) <= 0).all() and B >= 2, s.name       # the batches narrow: the widest unit comes first
        assert len(s.want) == (6 if p["query"] else 8) and s.ret == (C if p["host"] else 0), s.name
    big, cut, bad, query, host = steps
    p = big.bucketed
    assert len(p["off"]) - 1 > oc.BUCKET_TILE == 2048 and p["answer"]["counts"][0] > 1            # the sort takes more than one block; more than one batch
    assert p["lead"] == 0 and p["multiple"] % 4 == 0 and (p["multiple"], p["max_cells"]) == (8, 4096)      # 0 mod 16 and whole groups of 4 cells: the wide stores
    assert (big.status, p["cells_cap"], p["batches_cap"]) == (0, p["answer"]["counts"][1], p["answer"]["counts"][0])
    # the cut step: two radix passes from max_len alone, keys with either top digit, the narrow stores, both caps below the counts
    p = cut.bucketed
    ans = p["answer"]
    B, C = (int(x) for x in ans["counts"])
    keys = p["max_len"] - (np.minimum(np.diff(p["off"]), p["max_len"] - 2) + 2)
    assert p["max_len"] > 255 and sorted(set((keys >> 8).tolist())) == [0, 1]
    assert (4 * p["lead"]) % 16 == 4 and p["multiple"] % 4 != 0 and p["multiple"] == 3
    assert cut.status == 1 and C > p["cells_cap"] > 0 and B > p["batches_cap"] == B - 1
    assert p["cells_cap"] not in ans["cell"]
    b = int(np.searchsorted(ans["cell"], p["cells_cap"], side="right")) - 1
    assert (p["cells_cap"] - int(ans["cell"][b])) % int(ans["len"][b]) != 0 and 0 < b < B - 1      # strictly inside a row of a batch in the middle
    rows, mask = cut.want[0].array, cut.want[1].array
    assert rows[0] == -7 and np.array_equal(rows[1:1 + p["cells_cap"]], ans["rows"][:p["cells_cap"]]) and (rows[1 + p["cells_cap"]:] == -7).all()
    assert len(rows) == 1 + p["cells_cap"] + oc.TAIL and np.array_equal(mask[:p["cells_cap"]], ans["mask"][:p["cells_cap"]]) and (mask[p["cells_cap"]:] == 0x7F).all()
    for w, k in zip(cut.want[4:7], oc.BUCKET_OUTS[4:7]):                                # entries 0 .. batches_cap, the sentinel from there on
        assert len(w.array) == B + oc.TAIL and np.array_equal(w.array[:B], ans[k][:B]) and (w.array[B:] == -7).all(), w.label
    assert np.array_equal(flat_of(cut.want[7], 2), [B, C])                              # the counts are complete
    # the bad range: the last sequence alone is empty, every other sequence's row holds what it held (order and seq_pos are the restatement's)
    p, g = bad.bucketed, host.bucketed
    assert bad.status == 8 and p["ids"] is g["ids"] and all(p[k] == g[k] for k in ("max_len", "multiple", "max_cells")) and query.bucketed["off"] is g["off"]
    wrong = (p["off"][:-1] < 0) | (p["off"][1:] < p["off"][:-1]) | (p["off"][1:] > len(p["ids"]))
    assert wrong.sum() == 1 and wrong[-1] and np.array_equal(p["off"][:-1], g["off"][:-1]) and g["off"][-1] > g["off"][-2]
    nseq = len(p["off"]) - 1
    for q in range(nseq - 1):
        assert np.array_equal(unit_of(p["answer"], q), unit_of(g["answer"], q)), q
    assert unit_of(p["answer"], nseq - 1).tolist() == [oc.CLS, oc.SEP] and len(unit_of(g["answer"], nseq - 1)) > 2
    assert not np.array_equal(p["answer"]["order"], g["answer"]["order"])                 # (it moved in the order: it is among the narrowest now)
    assert np.array_equal(flat_of(bad.want[2], nseq), p["answer"]["order"]) and np.array_equal(flat_of(bad.want[3], nseq), p["answer"]["seq_pos"])
    assert (np.minimum(np.diff(g["off"]), g["max_len"] - 2) + 2).max() == g["max_len"]    # a width that reaches max_len: a truncated sequence
    assert [w.label for w in query.want] == [w.label for w in host.want[2:]] and all(np.array_equal(a.array, b.array) for a, b in zip(query.want, host.want[2:]))


def test_minhash_steps_cross_tiles_cut_rows_and_count_partial_pairs():
    import minhash_cases
    cat = ragged_cat()
    by = by_name(cat)
    steps = [s for s in cat.steps if hasattr(s, "minhash")]
    assert [s.name for s in steps] == ["minhash H=64 r=4 k=5 big", "minhash H=65 k=2 small, cut", "minhash small bad range", "minhash host small"]
    big, cut, bad, host = (s.minhash for s in steps)
    off = big["off"]
    n, first, last = np.diff(off), off[:-1] // minhash_cases.TILE, (off[1:] - 1) // minhash_cases.TILE
    assert minhash_cases.TILE == 1024 and off[-1] > 100 * minhash_cases.TILE                # many tiles
    assert ((n > 0) & (last > first)).any() and ((n > 0) & (last == first)).any() and (n == 0).any()      # a sequence over a tile's edge (the atomic path), one inside a tile, an empty one
    assert (big["k"], big["H"], big["r"]) == (5, 64, 4) and len(by["minhash H=64 r=4 k=5 big"].want) == 3 and ((n > 0) & (n < big["k"])).any()
    nseq = len(cut["off"]) - 1
    H, cap = cut["H"], cut["sig_cap"]
    assert 0 < cap < nseq and H % 64 != 0 and (cut["k"], H, cut["r"]) == (2, 65, 0) and steps[1].status == 1
    sig = steps[1].want[0].array
    assert len(sig) == cap * H + oc.TAIL and np.array_equal(sig[:cap * H], cut["answer"]["sig"].reshape(-1)[:cap * H]) and (sig[cap * H:] == -7).all()
    assert np.array_equal(flat_of(steps[1].want[1], nseq), cut["answer"]["nshingles"]) and (cut["answer"]["nshingles"][cap:] > 0).any()      # nshingles is complete
    small = minhash_cases.restate(host["ids"], host["off"], host["k"], host["H"], host["r"], host["seed"])
    assert small["status"] == 0 and host["r"] > 0 and host["host"] and all(np.array_equal(small[k], host["answer"][k]) for k in ("sig", "keys", "nshingles"))
    assert steps[2].status == 8 == bad["answer"]["status"] and all(bad[k] == host[k] for k in ("k", "H", "r", "seed")) and bad["ids"] is host["ids"]
    assert np.array_equal(bad["answer"]["sig"][:-1], small["sig"][:-1]) and (bad["answer"]["sig"][-1] == -1).all() and not (small["sig"][-1] == -1).all()
    assert bad["answer"]["nshingles"][-1] == 0 < small["nshingles"][-1]
    # the pairs steps: the host step's signatures; -1 at the pair out of range and nowhere else, a pair that shares some slots and not all
    p8, p0 = by["minhash pairs small"], by["minhash pairs small, clean"]
    sig, pairs = p8.pairs["sig"], p8.pairs["pairs"]
    assert sig is host["answer"]["sig"] and p0.pairs["sig"] is sig and sig.shape == (nseq, host["H"])
    outside = ((pairs < 0) | (pairs >= nseq)).any(axis=1)
    equal = flat_of(p8.want[0], len(pairs))
    assert p8.status == 8 and outside.sum() >= 1 and np.array_equal(equal == -1, outside)
    assert ((equal > 0) & (equal < host["H"])).any() and (equal == host["H"]).any() and (equal == 0).any()
    assert p0.status == 0 and np.array_equal(p0.pairs["pairs"], pairs[~outside]) and np.array_equal(flat_of(p0.want[0], len(pairs) - outside.sum()), equal[~outside])


def test_char_offset_steps_scan_in_blocks_and_hold_one_position_beyond():
    import charpos_cases as cc
    cat = ragged_cat()
    by = by_name(cat)
    steps = [s for s in cat.steps if hasattr(s, "charpos")]
    assert [s.name for s in steps] == ["byte to char big, utf16", "char to byte small, one beyond", "byte to char small, units only"]
    big = steps[0].charpos
    text = big["text"]
    assert len(text) > cc.TILE_CHUNKS * 64 * 4                                          # the scan of the chunk weights takes several blocks
    lead = text[(text & 0xC0) != 0x80]
    assert all(((lead >= lo) & (lead < hi)).any() for lo, hi in ((0xC0, 0xE0), (0xE0, 0xF0), (0xF0, 0xF8)))      # characters of 2, 3 and 4 bytes
    nd = len(big["doc_off"]) - 1
    u16 = flat_of(steps[0].want[2], nd)
    chars = cc.restate_array(text, big["doc_off"], cc.CHAR, cc.FWD, 0, big["starts"], big["ends"], big["item_off"])[2]
    nbytes = np.diff(big["doc_off"])
    assert big["unit"] == cc.UTF16 and big["direction"] == cc.FWD and (u16 > chars).any() and (chars < nbytes).any() and (u16 != nbytes).any()
    n = len(big["starts"])
    assert steps[0].status == 0 and (flat_of(steps[0].want[0], n) != big["starts"]).any() and len(steps[0].want) == 3
    # the small steps: the array form of the restatement is the sequential one
    for s in steps[1:]:
        p = s.charpos
        r = cc.restate(p["text"], p["doc_off"], p["unit"], p["direction"], p["flags"], p["starts"], p["ends"], p["item_off"])
        assert r["status"] == s.status, s.name
        got = {w.label: w.array for w in s.want}
        for k in ("starts", "ends"):
            assert (r[k] is None) == (k not in got) and (r[k] is None or np.array_equal(got[k][:r["n"]], r[k]) and len(got[k]) == r["n"] + oc.TAIL), (s.name, k)
        assert np.array_equal(got["doc_units"][:len(r["doc_units"])], r["doc_units"]) and (got["doc_units"][len(r["doc_units"]):] == -7).all(), s.name
    beyond = steps[1]
    p = beyond.charpos
    n = len(p["starts"])
    assert beyond.status == 8 and p["direction"] == cc.INV and p["unit"] == cc.CHAR and n == p["item_off"][-1]
    assert (flat_of(beyond.want[0], n) == -1).sum() + (flat_of(beyond.want[1], n) == -1).sum() == 1
    units = steps[2]
    assert [w.label for w in units.want] == ["doc_units"] and units.charpos["starts"] is None and units.charpos["ends"] is None and units.status == 0


@pytest.mark.parametrize("kind,program,variants", [("unigram", "lane", (3, 6)), ("bpe", "lanes", (3, 3 | 0x40))])
def test_both_offsets_programs_take_one_answer(kind, program, variants):
    cat = oc.catalogue(kind)
    if cat is None:
        pytest.skip("the model of the %s catalogue is not present" % kind)
    by = by_name(cat)
    for size in ("big", "small"):
        a, b = by["%s offsets" % size], by["%s %s offsets" % (program, size)]
        assert (a.variant, b.variant) == variants and a.size == b.size == size and a.status == b.status == 0
        assert [w.label for w in a.want] == ["ids", "first bytes", "last bytes", "id offsets"] and len(b.want) == 4
        assert all(x is y and x.array is y.array for x, y in zip(a.want, b.want))        # one answer, two programs

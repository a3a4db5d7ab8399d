"""CPU tier of tests/test_gpu_secondary_at_scale.py: the deterministic edge inputs of tests/secondary_cases.py (features at the last bytes
of a 64-byte window and the first of the next, with and without a byte order mark; first solid token of an id sequence at chosen
positions; tokens of 1 .. 5,000 bytes, 10^5 tokens, runs of spaces; dictionary keys of 0 .. 301 symbols) go through the oracle restatement
and through the compiled reference.  The reference's answers are kept as digests (length + sha256 per case,
tests/golden/ref_answers/secondary_*.json.gz): where oracle/_ref is built the live reference must reproduce them, elsewhere they stand in
for it (bfutil.reference_answers).  The oracle therefore stays a valid stand-in for the GPU tier where oracle/_ref is absent."""
import numpy as np
import pytest

import bfutil
import secondary_cases as sc


def _ref_digests(name, compute):
    """compute(checker) -> {case: digest}; the reference's, live or stored"""
    return bfutil.reference_answers(name, lambda: compute(True))


def _same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert got[k] == want[k], "%s: case %s: oracle [length, sha256] %s, reference %s" % (what, k, got[k], want[k])


def test_normalize_spaces_edges():
    docs = sc.normsp_docs()
    assert sum(1 for _, b in docs if 57000 <= len(b) <= (1 << 20) + 3) > 150 and max(len(b) for _, b in docs) > 1000000

    def compute(use_ref):
        ck = sc.Checker(use_ref)
        return {"%s/%x" % (name, usp): sc.digest(ck.normalize(b, usp)) for usp in sc.USPACES for name, b in docs}
    got = compute(False)
    _same(got, _ref_digests("secondary_normalize_spaces", compute), "NormalizeSpaces")
    # the inputs do what they are for: most documents have an answer, the invalid ones none, 0xD800 only where no uSpace is needed
    assert sum(1 for k, v in got.items() if v[0] > 0 and k.endswith("/2581")) > 150
    assert all(v[0] == 0 for k, v in got.items() if "lone_continuation" in k or "truncated_lead" in k)
    assert 0 < sum(1 for k, v in got.items() if v[0] > 0 and k.endswith("/d800")) < 20


def test_text_to_hashes_edges():
    docs = sc.hash_docs()

    def compute(use_ref):
        ck = sc.Checker(use_ref)
        return {"%s/%d/%d" % (name, ng, bucket): sc.digest(ck.hashes(b, ng, bucket)) for ng, bucket in sc.HASH_PARAMS for name, b in docs}
    got = compute(False)
    _same(got, _ref_digests("secondary_text_to_hashes", compute), "TextToHashes")
    assert got["tokens_100000/4/7"][0] == 400000 and got["empty/3/7"][0] == 3 and got["spaces_64/2/-3"][0] == 130


@pytest.mark.parametrize("model", sc.I2W_MODELS)
def test_ids_to_text_edges(model):
    ntok = sc.i2w_count(model)
    found = {}

    def compute(use_ref):
        ck = sc.Checker(use_ref)
        h = ck.load(model)
        sp = sc.i2w_specials(ck, h, ntok)
        found[use_ref] = sp
        out = {"specials": [sp[k] for k in sorted(sp)]}
        for name, ids in sc.i2t_sequences(sp, ntok):
            for skip in (0, 1):
                out["%s/%d" % (name, skip)] = sc.digest(ck.ids_to_text(h, ids, skip))
        ck.free(h)
        return out
    got = compute(False)
    want = _ref_digests("secondary_ids_to_text_" + model, compute)
    _same(got, want, "IdsToText " + model)
    sp = found[False]
    assert sp["lead"] is not None and sp["outside"] is not None
    # a sequence with an unknown id has no text unless skip_special leaves the id out (tokdll:1712-1721); its neighbours have theirs
    for k, v in got.items():
        if k.startswith("unknown_") and k.endswith("/0"):
            assert v[0] == 0, k
        if k.startswith("good_") or k.startswith("unknown_first_-1/1"):
            assert v[0] > 0, k
    assert got["quiet_never_solid/0" if sp["space"] is not None else "skipped_never_solid/1"][0] == 0


@pytest.mark.parametrize("model", ["gpt2.bin", "xlm_roberta_base.bin"])
def test_dict_get_info_edges(model):
    def compute(use_ref):
        dck = sc.DictChecker(model, use_ref)
        keys = sc.dict_edge_keys(model, dck)
        ret, ids, vals, off = dck.batch(keys)
        dck.close()
        flat, koff = sc.pack([np.array(k, dtype=np.int32) for k in keys], np.int32)
        return {"keys": sc.digest(flat), "key_off": sc.digest(koff), "ret": sc.digest(ret), "ids": sc.digest(ids), "vals": sc.digest(vals),
                "val_off": sc.digest(off), "hits": int((ret > 0).sum())}
    got = compute(False)
    _same(got, _ref_digests("secondary_dict_get_info_" + model, compute), "DictGetInfo " + model)
    assert got["hits"] > 1000


def test_tile_is_the_per_item_gather():
    """the numpy tiling the GPU tier builds its large batches with = the plain per-item loop"""
    items = [b"", b"a", b"bcd", b"", b"efghij", b"k", b"lmnopqrstu"]
    flat, off = sc.pack(items)
    idx = sc.tiling(len(items), 1000, 3)
    t_flat, t_off = sc.tile(flat, off, idx)
    assert set(idx.tolist()) == set(range(len(items)))
    assert t_flat.tobytes() == b"".join(items[i] for i in idx)
    assert t_off.tolist() == np.concatenate([[0], np.cumsum([len(items[i]) for i in idx])]).tolist()

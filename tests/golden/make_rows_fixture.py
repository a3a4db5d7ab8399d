"""Writes tests/golden/rows/encode_ids.json: the compiled reference's TextToIds answers for the documents of the end-to-end row tests
(rows_cases.encode_docs()) under the models of rows_cases.ENCODE_MODELS, at every max_len those tests use.  Needs oracle/_ref (the
build makes it where the reference sources are present); tests/test_rows_host.py re-checks the stored file against the live reference.

    python tests/golden/make_rows_fixture.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import bfutil        # noqa: E402
import rows_cases    # noqa: E402


def reference_ids(ref, h, doc, max_len, unk):
    """the ids the reference writes for one document; an unlimited max_len is asked for as the most ids a document of its size can have"""
    cap = min(max_len, 2 * (len(doc) + 1))
    c, buf = ref.text_to_ids(h, doc, cap, unk)
    return [int(x) for x in buf[:min(max(c, 0), cap)]]


def compute():
    ref = bfutil.reference()
    docs = rows_cases.encode_docs()
    out = {"docs": len(docs), "models": {}}
    for model, par in rows_cases.ENCODE_MODELS.items():
        h = ref.load(bfutil.model_path(model))
        out["models"][model] = {str(m): [reference_ids(ref, h, d, m, par["unk"]) for d in docs]
                                for m in sorted({rows_cases.encode_max_len(L, s, r) for L, s, r, _ in rows_cases.ENCODE_CASES})}
        ref.free(h)
    return out


if __name__ == "__main__":
    if not bfutil.have_ref():
        sys.exit("oracle/_ref is not built: the fixture is made from the compiled reference")
    os.makedirs(os.path.dirname(rows_cases.FIXTURE), exist_ok=True)
    with open(rows_cases.FIXTURE, "w") as f:
        json.dump(compute(), f, separators=(",", ":"))
        f.write("\n")
    print("wrote %s (%d bytes)" % (rows_cases.FIXTURE, os.path.getsize(rows_cases.FIXTURE)))

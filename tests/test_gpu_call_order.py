"""GPU: every ordered pair of calls on ONE handle.  A handle owns one set of grow-only device workspaces and one control block (bf_capi.cpp MiscWords);
nothing in a workspace is cleared between calls and the control words are cleared call by call, so a forgotten clear or a kernel that reads one element
past its own extent shows only in what the NEXT call on the handle computes.  Per kind of handle the steps of tests/order_cases.py -- the tokenizer programs
on a big and a small batch, the host forms, words and sentences, rows, pair rows, planes, packed rows, span cells, MLM, ids-to-text, the dictionary lookup,
hyphenation, calls that end with status 1, 4 or 8; and, as the kind `inputs` on a WordPiece handle of its own, the model-input calls: packed rows with
their planes form, stream rows, the capped MLM call beside the base one, span corruption, and the host-buffer forms of the packed, stream and rows-planes
stages, crossed with each other and with a Device and a host tokenizer call (the i2w kind crosses stream rows and a denoise call of status 1 with
IdsToText's status 4) -- run in the order of order_cases.circuit(), in which every ordered pair, a step behind itself included,
is neighbours exactly once (tests/test_order_host.py asserts that).  Behind every call: its return value, BfLastStatus -- the rule is that it is the call's
OWN, whatever the call before it left -- and every output buffer in full (every element up to the count, the sentinel behind it, the offsets) against the
checker's answer, on the device; a failure names the pair and the first document or row that differs, and ends the walk of that handle.

The growth tests run every step that uses the big batch on a fresh handle between two runs of a small step: every workspace the big step needs grows there
(DevBuf::reserve keeps no contents), in front of and behind a call that left the workspaces small."""
import pytest

import order_cases as oc

pytestmark = pytest.mark.gpu

KINDS = list(oc.BUILDERS)


@pytest.fixture(scope="module")
def cx():
    return oc.Context()


def catalogue(kind):
    cat = oc.catalogue(kind)
    if cat is None:
        pytest.skip("the model of the %s catalogue is not present" % kind)
    return cat


def check(cat, step, before, h, cx):
    """runs `step` and compares everything; returns None or the message of the first difference"""
    outs, ret, status = step.run(h, cx)
    pair = "`%s` -> `%s` (%s handle)" % (before.name if before else "a fresh handle", step.name, cat.kind)
    if ret != step.ret:
        return "%s: returned %d, wanted %d" % (pair, ret, step.ret)
    if status != step.status:
        return "%s: BfLastStatus is %d, the call's own is %d (%s); `%s` ends with %s" % (pair, status, step.status, step.why, before.name if before else "-",
                                                                                     before.status if before else "-")
    assert len(outs) == len(step.want), (pair, len(outs), len(step.want))
    for want, got in zip(step.want, outs):
        if isinstance(got, cx.torch.Tensor):
            same = cx.torch.equal(got.reshape(-1), cx.up(want.array).reshape(-1)) if want.array.size else True
            if not same:
                return "%s: %s" % (pair, oc.describe_difference(want, got.cpu().numpy()))
        elif got.shape != want.array.reshape(-1).shape or (got != want.array.reshape(-1)).any():
            return "%s: %s" % (pair, oc.describe_difference(want, got))
    if step.after:
        why = step.after(h)
        if why:
            return "%s: %s" % (pair, why)
    return None


@pytest.mark.parametrize("kind", KINDS)
def test_a_every_ordered_pair_on_one_handle(kind, cx):
    """one handle, circuit(n): n * n + 1 calls, every ordered pair of steps once"""
    import blingfire_amd as bf
    cat = catalogue(kind)
    order = oc.circuit(len(cat.steps), seed=len(cat.steps) // 2)
    h = cat.load()
    try:
        before = None
        for k, i in enumerate(order):
            step = cat.steps[i]
            why = check(cat, step, before, h, cx)
            assert why is None, "call %d of %d: %s" % (k, len(order), why)
            before = step
    finally:
        bf.free_model(h)
    print("%s: %d steps, %d calls, every ordered pair once" % (kind, len(cat.steps), len(order)))


@pytest.mark.parametrize("kind", KINDS)
def test_b_big_steps_grow_the_workspaces_between_small_ones(kind, cx):
    """per big step B a fresh handle: A (small), B, A again -- A is the next small step behind B in the catalogue"""
    import blingfire_amd as bf
    cat = catalogue(kind)
    n = len(cat.steps)
    loads = 0
    for i, big in enumerate(cat.steps):
        if big.size != "big":
            continue
        small = next(cat.steps[(i + k) % n] for k in range(1, n + 1) if cat.steps[(i + k) % n].size == "small")
        h = cat.load()
        loads += 1
        try:
            before = None
            for step in (small, big, small):
                why = check(cat, step, before, h, cx)
                assert why is None, "fresh handle, %s" % why
                before = step
        finally:
            bf.free_model(h)
    assert loads >= 1
    print("%s: %d big steps, each on a handle of its own" % (kind, loads))

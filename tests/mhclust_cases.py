"""MinHash clusters (MinHashClustersBatchDevice): the specification restated sequentially, and the inputs both tiers share.
live(q): no nshingles, or nshingles[q] > 0.  Per band, f(q, b) = the first live index with q's key in that column; (q, b) with f != q is a
candidate; it is an edge when min_equal == 0 or at least min_equal signature words of q and f agree.  Labels = the smallest index of each
connected component; a sequence that is not live is alone."""
import numpy as np

EMPTY = 0x4D4843454D505459            # MHC_EMPTY of bf_mhclust.h: the key that takes the table's side slot
I64_MIN = -(1 << 63)


def restate(keys, sig=None, min_equal=0, nshingles=None):
    """-> dict(label int32[nseq], keep uint8[nseq], size int32[nseq], counts int64[2], rejected, band_edges: the edges each band gave)"""
    nseq, B = keys.shape
    parent, cand, rejected, band_edges = list(range(nseq)), 0, 0, []

    def find(x):
        while parent[x] != x:
            parent[x] = x = parent[parent[x]]
        return x
    for b in range(B):
        first, edges = {}, []
        for q, k in enumerate(keys[:, b].tolist()):
            if nshingles is not None and nshingles[q] <= 0:
                continue
            f = first.setdefault(k, q)
            if f == q:
                continue
            cand += 1
            if min_equal == 0 or int((sig[q] == sig[f]).sum()) >= min_equal:
                edges.append((f, q))
                x, y = find(q), find(f)
                parent[max(x, y)] = min(x, y)
            else:
                rejected += 1
        band_edges.append(edges)
    label = np.array([find(q) for q in range(nseq)], dtype=np.int32).reshape(nseq)
    size = np.bincount(label, minlength=nseq)[label].astype(np.int32) if nseq else np.zeros(0, np.int32)
    keep = (label == np.arange(nseq)).astype(np.uint8)
    return dict(label=label, keep=keep, size=size, counts=np.array([int(keep.sum()), cand], dtype=np.int64), rejected=rejected, band_edges=band_edges)


def random_case(nseq, B, H, min_equal):
    """keys drawn per band from a range a quarter of nseq wide (buckets collide, components need several bands to connect), signatures of 0 / 1
    words (the equal counts straddle min_equal), about a tenth of the sequences without shingles; -> (keys, sig, nshingles, the restatement),
    after asserting on the restatement what the case is there for"""
    rng = np.random.default_rng(nseq * 1000 + B)
    keys = rng.integers(0, max(2, nseq // 4), size=(nseq, B)).astype(np.int64)
    sig = rng.integers(0, 2, size=(nseq, H)).astype(np.int32)
    nsh = (rng.random(nseq) >= 0.1).astype(np.int32) * 3
    if nseq >= 63:                                              # planted in column 0: a pair no min_equal > 0 accepts, and a sequence without shingles on its key
        nsh[:3] = (3, 3, 0)
        keys[:3, 0] = -5
        sig[1] = 1 - sig[0]
    want = restate(keys, sig, min_equal, nsh)
    if nseq >= 63:
        assert want["label"][2] == 2 and (want["rejected"] >= 1 or min_equal == 0)
        if B >= 5 and (min_equal <= H // 2 or H == 1):          # a component of at least 3 that no single band connects (a band's edges are a forest)
            top = int(np.bincount(want["label"]).argmax())
            members = int(want["size"][top])
            assert members >= 3 and all(members - sum(want["label"][f] == top for f, _ in e) > 1 for e in want["band_edges"])
    return keys, sig, nsh, want


def table():
    """(nseq, bands, num_perm, min_equal): the four lists rotating against each other"""
    NS, BS, HS = (1, 63, 64, 65, 1000, 5000), (1, 5, 32, 256), (1, 20, 64, 65, 256)
    out = []
    for i in range(12):
        H = HS[i % 5]
        out.append((NS[i % 6], BS[(i + i // 6) % 4], H, (0, 1, H // 2, H)[(i + i // 4 + 1) % 4]))
    return out


def named(name, nseq=5000, B=5):
    """-> (keys, what restate must say: dict of clusters / candidates)"""
    q = np.arange(nseq, dtype=np.int64)
    distinct = (q[:, None] + 1) * 1000 + np.arange(B)
    if name == "equal":
        return np.full((nseq, B), 42, dtype=np.int64), dict(clusters=1, candidates=(nseq - 1) * B)
    if name == "distinct":
        return distinct, dict(clusters=nseq, candidates=0)
    if name in ("chain", "chain-reversed"):                     # q and q + 1 share exactly band q % B; reversed: the indices mirrored
        keys = distinct.copy()
        for i in range(nseq - 1):
            x, y = (nseq - 1 - i, nseq - 2 - i) if name == "chain-reversed" else (i, i + 1)
            keys[y, i % B] = keys[x, i % B]
        return keys, dict(clusters=1, candidates=nseq - 1)
    assert name == "special"                                    # 0, -1, INT64_MIN and the empty mark, each twice, in column 0
    keys = distinct.copy()
    keys[:8, 0] = [0, -1, I64_MIN, EMPTY] * 2
    return keys, dict(clusters=nseq - 4, candidates=4)


NAMED = ("equal", "distinct", "chain", "chain-reversed", "special")

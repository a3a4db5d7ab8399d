"""TEST helpers for IdsToPackedRowsPlanesBatch: a restatement of the specification in include/blingfiretokdll_amd.h, written from that text on top
of the sequential restatement of the packed rows (packed_cases.restate) -- deliberately not the formulation of blingfire_amd/csrc/bf_packed.h: the
rows are laid out over ids that are their own element index plus a base above every special, and the cells are mapped back through the sources."""
import numpy as np

import packed_cases as pc

BASE = 1 << 20                     # above cls_id, sep_id and the padding mark of every test; BASE + index fits an int32 for every test's ids
PAD_MARK = 0
FILLS = [-1, -2, 7, 0]
CANARY = -0x35014542


def restate_packed_planes(off, L, cls, sep, src, fill, ids_len=None):
    """-> the list of planes, int32[R, L] each, complete whatever a call's rows_cap is (a caller compares the rows below min(R, rows_cap)).
    ids_len None: the largest offset (the host form reads the ids up to there)."""
    off = [int(x) for x in off]
    n = max([0] + off) if ids_len is None else int(ids_len)
    assert max(cls, sep, PAD_MARK) < BASE and BASE + n < 2 ** 31
    cells = pc.restate(BASE + np.arange(n, dtype=np.int64), off, L, cls, sep, PAD_MARK, ids_len=n)[0].astype(np.int64)
    holds_id = cells >= BASE                                # cls_id, sep_id and padding lie below the base
    planes = []
    for s, f in zip(src, fill):
        s = np.asarray(s, dtype=np.int32)
        plane = np.full(cells.shape, int(f), dtype=np.int32)
        plane[holds_id] = s[cells[holds_id] - BASE]         # an index at or past len(s) would raise: only elements of the source are read
        planes.append(plane)
    return planes


def sources(n, k, seed=0):
    """k arrays parallel to n ids whose values tell the array and the element apart"""
    return [((np.arange(n, dtype=np.int64) * (2 * j + 3) + 1000003 * (j + 1) + seed) % (2 ** 31 - 1)).astype(np.int32) for j in range(k)]


def bad_range_cases():
    """(offsets, ids_len) of test_gpu_packed.py::test_7_bad_ranges"""
    return [([0, 5, 3, 12, 20], 60), ([0, 10, 70, 70, 80], 60), ([0, 10, 20, 35, 60], 30), ([-1, 4, 9], 60)]

"""Host logic of the shared RIR estimate (one group of tied operator rows per recording): the batch plan that never splits a file, the sub-batch
split that never splits a group, and the yaml keys.  No GPU."""
import itertools

import pytest

CHUNK, OVERLAP = 16384, 2048


def _length(n_chunks):
    """a file length that chunk_plan cuts into exactly ``n_chunks`` chunks"""
    return CHUNK if n_chunks == 1 else CHUNK + (n_chunks - 1) * (CHUNK - OVERLAP) - 100


def _check_plan(lengths, batch_size, max_rows):
    from buddy_amd.testing.longform import chunk_plan, pool_plan_shared, run_bounds, shared_groups
    cuts, batches = pool_plan_shared(lengths, CHUNK, OVERLAP, batch_size, max_rows)
    assert cuts == [chunk_plan(L, CHUNK, OVERLAP) for L in lengths]
    want = sorted((f, k) for f in range(len(lengths)) for k in range(len(cuts[f][0])))
    assert sorted(itertools.chain.from_iterable(batches)) == want                       # every (file, chunk) exactly once
    where = {}
    for b, batch in enumerate(batches):
        assert len({cuts[f][1] for f, _ in batch}) == 1                                   # one chunk length per batch
        groups = shared_groups(cuts, batch, max_rows)
        assert groups[0] == 0 and all(d in (0, 1) for d in (y - x for x, y in zip(groups, groups[1:])))
        for (f, k), g in zip(batch, groups):
            where.setdefault(f, []).append((k, b, g))
    for f, L in enumerate(lengths):
        n = len(cuts[f][0])
        rows = sorted(where[f])
        assert [k for k, _, _ in rows] == list(range(n))
        runs = run_bounds(n, max_rows)
        assert runs[0][0] == 0 and runs[-1][1] == n and all(a[1] == b[0] for a, b in zip(runs, runs[1:]))
        assert all(0 < hi - lo <= max_rows for lo, hi in runs)
        assert len(runs) == 1 or n > max_rows                                             # only a file beyond max_rows is cut
        for lo, hi in runs:                                                               # a run is one group inside one batch
            assert len({(b, g) for k, b, g in rows if lo <= k < hi}) == 1
        if len(runs) > 1:                                                                 # and different runs are different groups
            assert len({(b, g) for _, b, g in rows}) == len(runs)
    fits = all(len(c[0]) <= min(batch_size, max_rows) for c in cuts)
    for batch in batches:
        files = {f for f, _ in batch}
        if fits:
            assert len(batch) <= batch_size
        if len(batch) > batch_size:                                                       # only a single file / run larger than batch_size
            assert len(files) == 1 and len(batch) <= max_rows
    return cuts, batches


def test_pool_plan_shared_examples():
    from buddy_amd.testing.longform import pool_plan_shared, shared_groups
    lengths = [40000, 30400, 11200]                                  # 3 chunks, 2 chunks, one short file (the case of the GPU test)
    cuts, batches = _check_plan(lengths, 4, 32)
    assert batches == [[(0, 0), (0, 1), (0, 2)], [(1, 0), (1, 1)], [(2, 0)]]
    cuts, batches = _check_plan(lengths, 8, 32)
    assert batches == [[(0, 0), (0, 1), (0, 2), (1, 0), (1, 1)], [(2, 0)]]
    assert shared_groups(cuts, batches[0], 32) == [0, 0, 0, 1, 1]
    # a file larger than batch_size gets a batch of its own with all its chunks
    cuts, batches = _check_plan([_length(2), _length(7), _length(1), _length(2)], 4, 32)
    assert [len(b) for b in batches] == [2, 7, 3]
    assert {f for f, _ in batches[1]} == {1}
    # a file larger than max_rows is cut into runs of at most max_rows, each a group of its own
    cuts, batches = _check_plan([_length(2), _length(11), _length(3)], 4, 5)
    assert [len(b) for b in batches] == [2, 4, 4, 3, 3]
    assert all({f for f, _ in b} == {1} for b in batches[1:4])
    cuts, batches = _check_plan([_length(11)], 16, 5)                # the runs of one file may share a batch: three groups
    assert len(batches) == 1 and shared_groups(cuts, batches[0], 5) == [0] * 4 + [1] * 4 + [2] * 3
    assert pool_plan_shared([], CHUNK, OVERLAP, 4, 32) == ([], [])
    # short files: as in pool_plan (equal lengths share a batch, every file its own group)
    cuts, batches = _check_plan([5000, CHUNK, 5000, 5001, 5000], 2, 32)
    assert batches == [[(1, 0)], [(0, 0), (2, 0)], [(4, 0)], [(3, 0)]]
    assert shared_groups(cuts, batches[1], 32) == [0, 1]


@pytest.mark.parametrize("batch_size,max_rows", [(1, 32), (3, 32), (4, 4), (8, 3), (5, 2), (64, 6)])
def test_pool_plan_shared_properties(batch_size, max_rows):
    counts = [1, 4, 2, 9, 1, 1, 3, 6, 13, 2]
    lengths = [_length(n) for n in counts] + [7000, 9000, 7000]
    cuts, _ = _check_plan(lengths, batch_size, max_rows)
    assert [len(c[0]) for c in cuts[:len(counts)]] == counts


def test_split_groups():
    from buddy_amd.testing.concurrent import split_groups, split_rows
    cases = [[0, 0, 0, 1, 1, 2], [0, 0, 0, 0], [0], [0, 1, 2, 3], [0, 0, 0, 0, 0, 1], [0, 1, 1, 1, 1, 1, 1, 2], [0, 0, 1, 1, 2, 2, 3, 3, 4]]
    for groups, S in itertools.product(cases, (1, 2, 3, 4)):
        parts = split_groups(groups, S)
        n = len(groups)
        assert 1 <= len(parts) <= S
        assert parts[0][0] == 0 and parts[-1][1] == n and all(a[1] == b[0] for a, b in zip(parts, parts[1:]))     # cover [0, n) in order
        assert all(lo < hi for lo, hi in parts)
        for lo, _ in parts[1:]:
            assert groups[lo] != groups[lo - 1]                                                                     # only on group boundaries
        if len(set(groups)) == 1:
            assert parts == [(0, n)]                                                                                # one group, one part
    assert split_groups([0, 0, 0, 1, 1, 2], 2) == [(0, 3), (3, 6)]
    assert split_groups([0, 0, 0, 0, 0, 1], 2) == [(0, 5), (5, 6)]
    assert split_groups([0, 1, 2, 3], 2) == split_rows(4, 2)               # groups of one: the even split
    assert split_groups([0, 0, 1, 1, 2, 2, 3, 3], 4) == split_rows(8, 4)


def test_yaml_keys():
    from buddy_amd.config import compose
    rr = compose(tester="real_dereverberation_BUDDy").tester.real_recordings
    assert rr.shared_rir is False and rr.shared_rir_max_chunks == 32
    rr = compose(tester="real_dereverberation_BUDDy", overrides=["tester.real_recordings.shared_rir=true",
                                                                 "tester.real_recordings.shared_rir_max_chunks=8"]).tester.real_recordings
    assert rr.shared_rir is True and rr.shared_rir_max_chunks == 8
    # a config written before the keys existed still loads: what the tester reads from it
    from buddy_amd.testing.tester import shared_rir_options
    old = compose(tester="real_dereverberation_BUDDy").tester.real_recordings
    del old["shared_rir"], old["shared_rir_max_chunks"]
    assert "shared_rir" not in old and shared_rir_options(old) == (False, 32)
    assert shared_rir_options(rr) == (True, 8)


def test_library_exports_set_groups():
    from buddy_amd import _lib
    assert "buddy_blindop_set_groups" in _lib.EXPORTED
    assert hasattr(_lib.load(), "buddy_blindop_set_groups")

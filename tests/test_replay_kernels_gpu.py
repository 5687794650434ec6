"""The decode kernels (sknnr_amd/csrc/replay.hip.h) run alone through a replay stream on an attribute-only handle --
predictions off, the decoded neighbours delivered again -- and compared with the numpy restatement (tests/_replay.py) by
``assert_array_equal`` over the WHOLE host buffers: every value and the 64 guard bytes in front of and behind them, which
must keep their pattern (the scheme of test_output_plans_kernels_gpu.py, on the host side where a stream's results land).

Grid: n of {1, 255, 256, 257, 1000} x ks of {1, 5, 8, 9} x k of {ks, 1} in every test, the tests over stored index type
{int32, int64} x stored distances {none, float32, float64} x layout {rows, planes} x ids {off, on}.  k <= 8 takes the
LDS-staged 16-byte stores, k = 9 the 8-byte ones.  The handles hold 1, 2, 300 and 5000 reference rows, in rotation; with ids
their tables hold as many entries -- 5000 is more than the skeleton's 1024 -- among them negative ids and, for int64
storage, ids beyond the int32 range.  One pixel in eight is masked, with garbage in its columns >= 1; wherever the tile has
the pixels, pixel 1 holds an unknown value in column 0, pixel 2 in the last USED column and pixel 4 in the last STORED
column, which counts only when k = ks.  ``sknnr_debug_last_replay`` is checked in every case: the counters, the
instantiation, the skeleton flag and 0 search launches.

Without the feature every test here fails with ``AttributeError`` (``_native`` has no ``TargetIndex``)."""

from __future__ import annotations

import numpy as np
import pytest

import _replay as RP

pytestmark = pytest.mark.gpu

GUARD = 64
PATTERN = 0xA5
NS = (1, 255, 256, 257, 1000)
KSS = (1, 5, 8, 9)
TABLES = (1, 2, 300, 5000)
ID_FILL = -999_999_937  # (in no id table below)


def id_table(n_ref, wide):
    """``n_ref`` unique ids in random order: negative ones, and with ``wide`` ones beyond the int32 range."""
    rng = np.random.default_rng(n_ref)
    pool = np.concatenate([np.arange(-40, 40) * 7, np.arange(6000) * 13 + 1000,
                           (2**31 + np.arange(50) * 3) if wide else (2**31 - 1 - np.arange(50) * 3),
                           (-(2**40) - np.arange(20)) if wide else (-(2**31) + np.arange(20))]).astype(np.int64)
    pool = np.unique(pool)
    assert ID_FILL not in pool
    return rng.permutation(pool)[:n_ref] if n_ref > 2 else rng.permutation(pool[[0, -1, 50]])[:n_ref]


@pytest.fixture(scope="module")
def handles():
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    made = {n: _native.TargetIndex(np.zeros((n, 1))) for n in TABLES}
    yield made
    for ix in made.values():
        ix.close()


def stored_tile(n, ks, k, n_ref, idx_dtype, dist_dtype, table, seed):
    """A row tile of stored neighbours with the masked and unknown pixels of the module docstring; its fill value."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, n_ref, size=(n, ks))
    fill = -1 if table is None else ID_FILL
    idx = (rows if table is None else table[rows]).astype(np.int64)
    absent = n_ref + 3 if table is None else 5  # (no row position / in no table: every id is 1 mod 13, 0 mod 7 or huge)
    if table is not None:
        assert absent not in table
    if n > 1:
        idx[1, 0] = absent
    if n > 2:
        idx[2, k - 1] = -2 if table is None else absent
    if n > 4:
        idx[4, ks - 1] = absent
    idx[3::8, 0] = fill
    idx[3::8, 1:] = 2**31 - 5  # garbage: only the first column decides
    dist = None
    if dist_dtype is not None:
        dist = np.sort(rng.uniform(0.0, 9.0, size=(n, ks)), axis=1).astype(dist_dtype)
        dist[::5, 0] = 0.0
    return idx.astype(idx_dtype), dist, fill


def guarded(shape, dtype, shift=0):
    """A host array of ``shape`` inside a buffer with GUARD pattern bytes on either side; ``shift``: extra bytes in front,
    so that the array's address need not be aligned."""
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    buf = np.full(GUARD + shift + nbytes + GUARD, PATTERN, dtype=np.uint8)
    return buf, buf[GUARD + shift:GUARD + shift + nbytes].view(dtype).reshape(shape)


def expected_buffer(buf, values, shift=0):
    want = np.full_like(buf, PATTERN)
    raw = np.ascontiguousarray(values).view(np.uint8).reshape(-1)
    want[GUARD + shift:GUARD + shift + raw.size] = raw
    return want


def run_case(ix, native, n, ks, k, idx_dtype, dist_dtype, planes, ids, seed, shift=0):
    n_ref = ix.n_ref
    table = id_table(n_ref, np.dtype(idx_dtype) == np.int64) if ids else None
    ix.set_replay_ids(table)
    idx, dist, fill = stored_tile(n, ks, k, n_ref, idx_dtype, dist_dtype, table, seed)
    want_idx, want_dist, masked, unknown = RP.decode(idx, dist, k, n_ref, fill, table)
    shape = (k, n) if planes else (n, k)
    ibuf, out_idx = guarded(shape, np.int64, shift)
    dbuf, out_dist = guarded(shape, np.float64, shift) if dist is not None else (None, None)
    stream = ix.open_replay(k, ks, idx_dtype=idx_dtype, dist_dtype=dist_dtype, fill_index=fill, ids=ids,
                            want_dist=dist is not None, want_pred=False)
    try:
        if planes:
            stream.push_planes(np.ascontiguousarray(idx.T), None if dist is None else np.ascontiguousarray(dist.T),
                               out_idx=out_idx, out_dist=out_dist, need_idx=True)
        else:
            stream.push(idx, dist, out_idx=out_idx, out_dist=out_dist, need_idx=True)
        counts = stream.counts()
    finally:
        stream.close()
    where = (n, ks, k, n_ref)
    np.testing.assert_array_equal(ibuf, expected_buffer(ibuf, want_idx.T if planes else want_idx, shift), err_msg=str(where))
    if dist is not None:
        np.testing.assert_array_equal(dbuf, expected_buffer(dbuf, want_dist.T if planes else want_dist, shift), err_msg=str(where))
    assert counts == dict(pixels=n, masked=int(masked.sum()), unknown=int(unknown.sum()),
                          first_unknown=0 if unknown.any() else -1), where
    rec = ix.debug_last_replay()
    assert rec == dict(pixels=n, masked=int(masked.sum()), unknown=int(unknown.sum()),
                       instance=native.replay_instance(idx_dtype, dist_dtype, planes), skeleton=int(ids), search_launches=0,
                       k=k, ks=ks), where
    return masked, unknown


@pytest.mark.parametrize("ids", [False, True], ids=["positions", "ids"])
@pytest.mark.parametrize("planes", [False, True], ids=["rows", "planes"])
@pytest.mark.parametrize("dist_dtype", [None, np.float32, np.float64], ids=["nodist", "f32", "f64"])
@pytest.mark.parametrize("idx_dtype", [np.int32, np.int64], ids=["i32", "i64"])
def test_decode_equals_the_restatement(handles, idx_dtype, dist_dtype, planes, ids):
    from sknnr_amd import _native

    case = 0
    seen_unused = seen_unknown = 0
    for n in NS:
        for ks in KSS:
            for k in sorted({ks, 1}):
                ix = handles[TABLES[case % len(TABLES)]]
                masked, unknown = run_case(ix, _native, n, ks, k, idx_dtype, dist_dtype, planes, ids, 1000 + case)
                if n > 4 and k < ks:
                    assert not unknown[4], "an unknown value in an unused column must not count"
                    seen_unused += 1
                if n > 2:
                    assert unknown[1] and unknown[2]
                    seen_unknown += 1
                assert masked[3::8].all() and masked.sum() == len(masked[3::8])
                case += 1
    assert seen_unused and seen_unknown


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_a_destination_that_is_not_4_byte_aligned(handles, shift):
    from sknnr_amd import _native

    for planes in (False, True):
        run_case(handles[5000], _native, 257, 5, 5, np.int32, np.float32, planes, True, 77 + shift, shift=shift)
        run_case(handles[300], _native, 1000, 9, 9, np.int64, np.float64, planes, False, 78 + shift, shift=shift)


def test_every_id_of_the_large_table_is_found(handles):
    """All 5000 ids, each stored once: the skeleton's stretches have no gap at their ends."""
    ix = handles[5000]
    table = id_table(5000, True)
    ix.set_replay_ids(table)
    with ix.open_replay(1, 1, idx_dtype=np.int64, ids=True, fill_index=ID_FILL, want_pred=False) as stream:
        out_idx, _, _ = stream.push(np.ascontiguousarray(table.reshape(-1, 1)), need_idx=True)
        assert stream.counts() == dict(pixels=5000, masked=0, unknown=0, first_unknown=-1)
    np.testing.assert_array_equal(out_idx[:, 0], np.arange(5000))


def test_neighbours_leave_retyped_and_as_ids_again(handles):
    """The decoded tile through the unchanged output side: int32 / float32 outputs, and indices as ids again."""
    ix = handles[300]
    table = id_table(300, False)
    ix.set_replay_ids(table)
    idx, dist, fill = stored_tile(257, 5, 5, 300, np.int32, np.float32, table, 5)
    want_idx, want_dist, masked, unknown = RP.decode(idx, dist, 5, 300, fill, table)
    with ix.open_replay(5, 5, idx_dtype=np.int32, dist_dtype=np.float32, fill_index=fill, ids=True, want_dist=True,
                        want_pred=False) as stream:
        stream.set_output(index_dtype=np.int32, distance_dtype=np.float32)
        stream.set_id_table(table, fill_id=-77)
        out_idx, out_dist, _ = stream.push(idx, dist, need_idx=True)
        stream.flush()
    bad = masked | unknown
    np.testing.assert_array_equal(out_idx, np.where(bad[:, None], -77, table[np.maximum(want_idx, 0)]).astype(np.int32))
    np.testing.assert_array_equal(out_dist, want_dist.astype(np.float32))
    np.testing.assert_array_equal(out_idx[~bad], idx[~bad])  # (ids in, the same ids out)


def test_the_first_push_with_unknown_values_is_reported(handles):
    ix = handles[300]
    ix.set_replay_ids(None)
    good = np.zeros((40, 2), dtype=np.int32)
    bad = good.copy()
    bad[7, 1] = 300
    with ix.open_replay(2, 2, idx_dtype=np.int32, want_pred=False) as stream:
        stream.push(good, need_idx=True)
        stream.push(good[:0], need_idx=True)  # (an empty push counts)
        stream.push(bad, need_idx=True)
        stream.push(bad, need_idx=True)
        assert stream.counts() == dict(pixels=120, masked=0, unknown=2, first_unknown=2)


def test_refusals_of_the_stream_entries(handles):
    from sknnr_amd import _native

    ix = handles[300]
    ix.set_replay_ids(None)
    for kwargs, what in ((dict(k=3, ks=2), "outside"), (dict(k=2, ks=2, ids=True), "sknnr_index_set_replay_ids"),
                         (dict(k=2, ks=2, want_dist=True), "want_dist without stored distances"),
                         (dict(k=2, ks=2, weight_mode=_native.WEIGHTS_DISTANCE), "need the stored distances")):
        k, ks = kwargs.pop("k"), kwargs.pop("ks")
        with pytest.raises(_native.HipBackendError, match=what):
            ix.open_replay(k, ks, **kwargs)
    with ix.open_replay(2, 2, idx_dtype=np.int32) as stream:
        with pytest.raises(_native.HipBackendError, match="replay stream has no feature rows to mask"):
            stream.set_nodata(np.zeros(1))
        with pytest.raises(_native.HipBackendError, match="without stored distances"):
            stream.set_tally()
        with pytest.raises(_native.HipBackendError, match="without stored distances"):
            stream.set_domain(np.array([0.0, 1.0]))
        with pytest.raises(_native.HipBackendError, match="a replay stream takes stored neighbours"):
            rows, out = np.zeros((1, 2)), np.zeros((1, 2), dtype=np.int64)
            _native.check(_native.load().sknnr_stream_push_typed(stream._h, rows.ctypes.data, 1, None, out.ctypes.data, None))

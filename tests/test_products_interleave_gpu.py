"""One-shot side-product calls between the pushes of an open stream that carries the same products, on one handle.

A handle keeps one debug record per product (neighbour usage, zonal statistics, distance domain) whose device words are
split in two halves -- one-shot calls, the open stream -- and parks each kind of call's parameter buffers (class table,
percentile table) beside the stream's.  Nothing else in the suite makes a one-shot call while a stream is open, so
nothing else would notice the two kinds of call sharing a buffer.

Set-up: 64 reference rows, d = 8, t = 2, k = 3.  The stream tallies usage, zonal statistics (4 zones; the second column
has 3 classes) and a domain (16-entry table, a threshold); it takes two tiles of 300 rows.  Between them, in host
memory and with other shapes: ``tally_from_neighbors`` (50 rows, k = 2), ``zonal_from_values`` (40 pixels, c = 1, 5
zones, no classes) and ``domain_from_neighbors`` (30 pixels, k = 2, m = 5).  Everything is compared byte for byte with
the same stream on a fresh handle without the calls, and with the same calls on a fresh handle without the stream.

The records: read straight after a one-shot call each reports that call (its rows, its shape, its entries); read after
the second push each reports the stream's 600 pixels in the words its kernels counted on the device (tally: entries
tallied + skipped = 600 k; zonal: entries tallied = 600 c; domain: pixels = 600), and the tally's k and the zonal c are
the stream's again.  The words the HOST keeps are one set per record, not one per half, and are not asserted where the
two kinds of call mix in them: a one-shot call overwrites the running pixel count and the next tile adds to that
(``rows`` reads 50 + 300 = 350 and the zonal ``pixels`` 40 + 300 = 340 here, not 600), and the domain's k / rank / m stay
the call's (2, 2, 5) until the next setter.  The library did so before the records became one type, this test passes on
it unchanged, and the device words beside them are the ones that stay apart.

Measured on an MI355X: 3.9 s when the file runs alone, nearly all of it the first handle's device set-up.
"""

from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_REF, D, T, K = 64, 8, 2, 3
TILE = 300
N_ZONES = 4
N_CLASSES = (0, 3)


def problem():
    rng = np.random.default_rng(59)
    ref = rng.standard_normal((N_REF, D))
    y = np.column_stack([rng.uniform(0.0, 500.0, N_REF), rng.integers(0, 3, N_REF).astype(np.float64)])
    tiles = [rng.standard_normal((TILE, D)) for _ in range(2)]
    zones = [rng.integers(0, N_ZONES, TILE).astype(np.int32) for _ in range(2)]
    table = np.sort(rng.uniform(0.5, 4.0, 16))
    return ref, y, tiles, zones, table


def one_shot_inputs():
    rng = np.random.default_rng(60)
    return dict(
        t_idx=rng.integers(0, N_REF, (50, 2)).astype(np.int64), t_dist=rng.uniform(0.0, 3.0, (50, 2)),
        z_val=rng.uniform(-100.0, 100.0, (40, 1)), z_zones=rng.integers(0, 5, 40).astype(np.int32),
        d_dist=np.sort(rng.uniform(0.0, 3.0, (30, 2)), axis=1), d_table=np.array([0.2, 0.7, 1.1, 1.9, 2.6]))


def open_stream(ix, table):
    from sknnr_amd import _native

    return ix.open_stream(_native.Index.make_opts(K), want_dist=True, want_pred=True, output=dict(pred_dtype=np.int16),
                          tally=True, zonal=(N_ZONES, N_CLASSES), domain=(table, 2, 2.5, False))


def push(st, tile, zones):
    codes = np.empty(TILE, dtype=np.uint8)
    st.next_zones(zones)
    st.next_domain_out(codes)
    idx, dist, pred = st.push(tile)
    return idx, dist, pred, codes


def one_shots(ix, a, records=None):
    """The three calls; ``records``: a list the debug record read behind each call is appended to."""
    out = []
    out.append(ix.tally_from_neighbors_host(a["t_dist"], a["t_idx"]))
    if records is not None:
        records.append(ix.debug_last_tally())
    out.append(ix.zonal_from_values_host(a["z_val"], a["z_zones"], np.int16, 5))
    if records is not None:
        records.append(ix.debug_last_zonal())
    out.append(ix.domain_from_neighbors_host(a["d_dist"], a["d_table"], rank=2, threshold=1.5))
    if records is not None:
        records.append(ix.debug_last_domain())
    return out


def as_bytes(parts):
    return [None if p is None else np.ascontiguousarray(p).tobytes() for group in parts for p in group]


def test_one_shot_calls_between_the_pushes_of_a_stream_with_the_same_products():
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    ref, y, tiles, zones, table = problem()
    a = one_shot_inputs()

    # the stream alone, and the calls alone, each on a handle of its own
    ix = _native.Index(ref, y)
    try:
        st = open_stream(ix, table)
        alone_tiles = [push(st, tiles[i], zones[i]) for i in range(2)]
        alone = [st.tally(), st.zonal(), (st.domain(),)]
        st.close()
    finally:
        ix.close()
    ix = _native.Index(ref, y)
    try:
        calls_alone = one_shots(ix, a)
    finally:
        ix.close()

    # both on one handle: a tile, the three calls, a tile
    ix = _native.Index(ref, y)
    try:
        st = open_stream(ix, table)
        mixed_tiles = [push(st, tiles[0], zones[0])]
        records = []
        calls_mixed = one_shots(ix, a, records)
        mixed_tiles.append(push(st, tiles[1], zones[1]))
        mixed = [st.tally(), st.zonal(), (st.domain(),)]
        after = [ix.debug_last_tally(), ix.debug_last_zonal(), ix.debug_last_domain()]
        st.close()
    finally:
        ix.close()
    print("records behind the calls:", records)
    print("records behind the second push:", after)

    assert as_bytes(mixed) == as_bytes(alone), "the stream's products differ from the same pushes without the calls"
    assert as_bytes(mixed_tiles) == as_bytes(alone_tiles), "the stream's tiles differ from the same pushes without the calls"
    assert as_bytes(calls_mixed) == as_bytes(calls_alone), "the one-shot results differ from the same calls without the stream"
    assert mixed[0][0].sum() == 2 * TILE * K and mixed[2][0][:101].sum() == 2 * TILE  # (the stream did tally both tiles)
    assert mixed[1][1] is not None and calls_mixed[1][1] is None

    rt, rz, rd = records
    assert rt["ran"] == 1 and rt["rows"] == 50 and rt["k"] == 2 and rt["tallied"] + rt["skipped"] == 100, rt
    assert rz["ran"] == 1 and rz["pixels"] == 40 and rz["c"] == 1 and rz["tallied"] + rz["nan"] == 40 and rz["outside"] == 0, rz
    assert rd["ran"] == 1 and rd["pixels"] == 30 and (rd["k"], rd["rank"], rd["m"]) == (2, 2, 5), rd
    rt, rz, rd = after
    assert rt["ran"] == 1 and rt["k"] == K and rt["tallied"] + rt["skipped"] == 2 * TILE * K, rt
    assert rz["ran"] == 1 and rz["c"] == T and rz["tallied"] + rz["nan"] == 2 * TILE * T and rz["outside"] == 0, rz
    assert rd["ran"] == 1 and rd["pixels"] == 2 * TILE and rd["nodata"] == 0, rd

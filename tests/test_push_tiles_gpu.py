"""One push that spans several pipeline tiles, with every per-push array a tile takes a slice of: the zone codes, the
domain's code plane, stored neighbours (rows and planes), row and band-first outputs.

``SKNNR_HOST_CHUNK_ROWS`` is read once per process, so a child runs with 1,024 pixels per pipeline tile -- once ramping
up, once with ``SKNNR_PIPE_NO_RAMP=1`` (a 7,000-pixel push is then seven tiles through the four slots) and once with
``SKNNR_PIPE_WORKERS=0`` (no look-ahead copy-in, the copy-out deferred to the drain).  Only results are compared, never
the cuts.

Set-up (tests/test_products_interleave_gpu.py's): 64 reference rows, d = 8, t = 2, k = 3, random normal rows (no ties);
single pushes of 1, 1,024, 1,025, 2,500 and 7,000 pixels, each once as rows and once band-first, on one handle:

(a) a search stream: indices, distances, int16 predictions, the usage tally, zonal tables (4 zones, the second column
    has 3 classes) and a domain (16-entry table, a threshold, beyond pixels blanked), ``next_zones`` and
    ``next_domain_out`` before every push;
(b) a replay stream on stored int32 indices / float32 distances with ks = 5 > k = 3 and a few pixels holding
    ``fill_index``: predictions, decoded neighbours, tally, zonal tables and the domain's code plane, each size once
    through ``sknnr_replay_push`` and once through ``sknnr_replay_push_planes`` with ``in_stride`` and ``out_stride``
    larger than the push.

Nothing expected comes from the pipeline: the neighbours are ONE device-memory ``kneighbors`` call per k on the same
handle (no HostPipe), and predictions, conversions, usage counts, zonal tables, domain codes and replay counts are the
host restatements (tests/_predict_ref.py, _narrow.py, _usage.py, _zonal.py, _domain.py, _replay.py) applied to them.

Measured on an MI355X: 4 s per parametrisation, nearly all of it the child's start-up and the handle's device set-up.
"""

from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_REF, D, T, K, KS = 64, 8, 2, 3, 5
SIZES = (1, 1024, 1025, 2500, 7000)
N_ZONES, N_CLASSES = 4, (0, 3)
RANK, THRESHOLD = 2, 2.5
FILL_INDEX, FILL_PRED = -3, -9999
PAD_IN, PAD_OUT = 5, 3  # elements between the planes of a replayed band-first push beyond its pixels: stored, delivered


def problem():
    rng = np.random.default_rng(61)
    ref = rng.standard_normal((N_REF, D))
    y = np.column_stack([rng.uniform(0.0, 500.0, N_REF), rng.integers(0, 3, N_REF).astype(np.float64)])
    table = np.sort(rng.uniform(0.5, 4.0, 16))
    # one entry per push of a stream: (pixels, band-first), the rows, the zone codes
    pushes = [(n, bands, rng.standard_normal((n, D)), rng.integers(0, N_ZONES, n).astype(np.int32))
              for bands in (False, True) for n in SIZES]
    return ref, y, table, pushes


def device_neighbors(ix, x, k):
    """One device-memory call on all rows of ``x``: it does not run through the host pipeline."""
    import torch

    xq = torch.as_tensor(x, device="cuda")
    dist = torch.empty((len(x), k), dtype=torch.float64, device="cuda")
    idx = torch.empty((len(x), k), dtype=torch.int64, device="cuda")
    ix.kneighbors_device(xq.data_ptr(), len(x), ix.make_opts(k), dist.data_ptr(), idx.data_ptr())
    torch.cuda.synchronize()
    return dist.cpu().numpy(), idx.cpu().numpy()


def rows_of(a, bands):
    return np.ascontiguousarray(a.T) if bands else a


class Expected:
    """The side products of a stream's pushes, accumulated by the restatements."""

    def __init__(self, table):
        import _zonal as ZN

        self.table = table
        self.counts = self.max_dist = self.dom = None
        self.acc, self.hist = ZN.empty(N_ZONES, T, N_CLASSES)

    def add(self, idx, dist, pred, zones, threshold):
        import _domain as DM
        import _usage as US
        import _zonal as ZN

        self.counts, self.max_dist, _ = US.tally(idx, dist, N_REF, self.counts, self.max_dist)
        ZN.zonal(pred, zones, np.int16, None, None, N_ZONES, N_CLASSES, self.acc, self.hist)
        self.dom = DM.acc(dist, self.table, RANK, threshold, into=self.dom)

    def check(self, st):
        counts, max_dist = st.tally()
        np.testing.assert_array_equal(counts, self.counts)
        np.testing.assert_array_equal(max_dist, self.max_dist)
        acc, hist = st.zonal()
        np.testing.assert_array_equal(acc, self.acc)
        np.testing.assert_array_equal(hist, self.hist)
        np.testing.assert_array_equal(st.domain(), self.dom)


def search_stream(ix, y, table, pushes, dist, idx):
    import _domain as DM
    import _narrow as NR
    import _predict_ref as PR

    st = ix.open_stream(ix.make_opts(K), want_dist=True, want_pred=True, output=dict(pred_dtype=np.int16, fill=FILL_PRED),
                        tally=True, zonal=(N_ZONES, N_CLASSES), domain=(table, RANK, THRESHOLD, True))
    got = []
    for n, bands, x, zones in pushes:
        codes = np.full(n, 77, dtype=np.uint8)
        st.next_zones(zones)
        st.next_domain_out(codes)
        if bands:
            planes = np.ascontiguousarray(x.T)
            got.append(st.push_planes([planes[j] for j in range(D)]) + (codes,))
        else:
            got.append(st.push(x) + (codes,))
    want, preds, r0, blanked = Expected(table), [], 0, 0
    for n, bands, x, zones in pushes:
        d, i = dist[r0:r0 + n], idx[r0:r0 + n]
        preds.append(DM.masked_predictions(PR.sklearn_predict(y, d, i, "uniform"), d, RANK, THRESHOLD))
        blanked += int(np.isnan(preds[-1][:, 0]).sum())
        want.add(i, d, preds[-1], zones, THRESHOLD)
        r0 += n
    want.check(st)  # (flushes: every push's arrays are filled from here on)
    r0 = 0
    for (n, bands, x, zones), pred, (g_idx, g_dist, g_pred, g_codes) in zip(pushes, preds, got):
        d, i = dist[r0:r0 + n], idx[r0:r0 + n]
        assert g_pred.dtype == np.int16 and g_pred.shape == ((T, n) if bands else (n, T))
        np.testing.assert_array_equal(rows_of(g_idx, bands), i)
        np.testing.assert_array_equal(rows_of(g_dist, bands), d)
        np.testing.assert_array_equal(rows_of(g_pred, bands), NR.narrow_values(pred, np.int16, fill=FILL_PRED))
        np.testing.assert_array_equal(g_codes, DM.codes(d, table, RANK))
        r0 += n
    assert st.close() == r0
    assert 0 < blanked < r0  # (the threshold does cut the pixels in two)


def replay_stream(ix, y, table, pushes, dist5, idx5):
    import _domain as DM
    import _narrow as NR
    import _replay as RP
    from sknnr_amd import _native

    lib = _native.load()
    rng = np.random.default_rng(62)
    st = ix.open_replay(K, KS, idx_dtype=np.int32, dist_dtype=np.float32, fill_index=FILL_INDEX, want_dist=True,
                        want_pred=True)
    st.configure(output=dict(pred_dtype=np.int16, fill=FILL_PRED), tally=True, zonal=(N_ZONES, N_CLASSES),
                 domain=(table, RANK, None, False))
    got, stored, r0 = [], [], 0
    for n, bands, x, zones in pushes:
        s_idx, s_dist = idx5[r0:r0 + n].astype(np.int32), dist5[r0:r0 + n].astype(np.float32)
        s_idx[rng.random(n) < 0.02, 0] = FILL_INDEX
        if n == 7000:
            s_idx[[0, 1023, 1024, 6143, 6144, 6999], 0] = FILL_INDEX  # (beside the seams of either set of cuts)
        stored.append((s_idx, s_dist))
        codes = np.full(n, 77, dtype=np.uint8)
        st.next_zones(zones)
        st.next_domain_out(codes)
        if bands:
            # planes in_stride apart in, out_stride apart out: windows of wider arrays whose other columns must stay
            wide_i = np.full((KS, n + PAD_IN), 10**6, dtype=np.int32)
            wide_d = np.full((KS, n + PAD_IN), -1.0, dtype=np.float32)
            wide_i[:, :n], wide_d[:, :n] = s_idx.T, s_dist.T
            outs = [np.full((c, n + PAD_OUT), 55, dtype=dt) for c, dt in ((K, np.int64), (K, np.float64), (T, np.int16))]

            def native(h, tile, nq, od, oi, op, stride, in_stride=n + PAD_IN):
                return lib.sknnr_replay_push_planes(h, _native._host_ptr(tile[0]), _native._host_ptr(tile[1]), nq, in_stride,
                                                    od, oi, op, stride)
            res = st._push(native, (wide_i, wide_d), n, True, outs[0][:, :n], outs[1][:, :n], outs[2][:, :n], True)
            got.append(res + (codes, outs))
        else:
            got.append(st.push(s_idx, s_dist, need_idx=True) + (codes, None))
        r0 += n
    want, masked = Expected(table), 0
    decoded = []
    for (n, bands, x, zones), (s_idx, s_dist) in zip(pushes, stored):
        i64, d64, m, unknown = RP.decode(s_idx, s_dist, K, N_REF, FILL_INDEX)
        assert not unknown.any()
        pred = RP.reduce(y, i64, d64, "uniform")
        want.add(i64, d64, pred, zones, None)
        masked += int(m.sum())
        decoded.append((i64, d64, pred))
    want.check(st)  # (flushes)
    assert st.counts() == {"pixels": r0, "masked": masked, "unknown": 0, "first_unknown": -1}
    for (n, bands, x, zones), (i64, d64, pred), (g_idx, g_dist, g_pred, g_codes, outs) in zip(pushes, decoded, got):
        np.testing.assert_array_equal(rows_of(g_idx, bands), i64)
        np.testing.assert_array_equal(rows_of(g_dist, bands), d64)
        np.testing.assert_array_equal(rows_of(g_pred, bands), NR.narrow_values(pred, np.int16, fill=FILL_PRED))
        np.testing.assert_array_equal(g_codes, DM.codes(d64, table, RANK))
        if outs is not None:
            for a in outs:
                assert (a[:, n:] == 55).all(), "a band-first push wrote between its planes"
    assert masked >= 6 and st.close() == r0


def child():
    from sknnr_amd import _native

    assert _native.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    ref, y, table, pushes = problem()
    x_all = np.concatenate([p[2] for p in pushes])
    ix = _native.Index(ref, y)
    try:
        dist, idx = device_neighbors(ix, x_all, K)
        dist5, idx5 = device_neighbors(ix, x_all, KS)
        for a in (dist, idx, dist5, idx5):
            a.setflags(write=False)
        search_stream(ix, y, table, pushes, dist, idx)
        replay_stream(ix, y, table, pushes, dist5, idx5)
    finally:
        ix.close()
    print("ok", len(x_all))


_CHILD = "import sys; sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r}); import test_push_tiles_gpu as T; T.child()"


@pytest.mark.parametrize("mode", ["ramp", "no_ramp", "no_workers"])
def test_a_push_of_several_tiles_slices_every_per_push_array(mode):
    env = dict(os.environ, SKNNR_HOST_CHUNK_ROWS="1024")
    env.pop("SKNNR_PIPE_NO_RAMP", None)
    env.pop("SKNNR_PIPE_WORKERS", None)
    if mode == "no_ramp":
        env["SKNNR_PIPE_NO_RAMP"] = "1"
    if mode == "no_workers":
        env["SKNNR_PIPE_WORKERS"] = "0"
    run = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))],
                         env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    assert run.stdout.strip().splitlines()[-1] == f"ok {2 * sum(SIZES)}", run.stdout[-500:]

"""Neighbour replay against the search it replaces, on the shape ``bench.py --full`` streams: 50,000 x 32 reference rows,
k = 5, 3 targets, row tiles of 1,000,000 pixels.

One search call (``predict_chunks(..., return_neighbors=True, neighbors_out=...)``) stores the neighbour raster; then, in
alternation and ``--reps`` times each, the search call again and ``predict_neighbors_chunks`` on the stored raster as
(int32 row positions, float32 distances), (int64, float64) and indices alone with uniform weights.  Every call writes into a
preallocated array and ends in the stream's flush, so the host clock around it covers copies in, kernels and copies out.
The replayed predictions are compared with the search call's (bit for bit for full storage).

``--replay-only`` runs the three replays alone, for a kernel trace of their launches:
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/replay_probe.py --replay-only
"""

from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=4)
    ap.add_argument("--tile", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--replay-only", action="store_true")
    args = ap.parse_args()
    import sknnr_amd

    n_ref, d, k, t = 50_000, 32, 5, 3
    n = args.tiles * args.tile
    rng = np.random.default_rng(0)
    X = rng.standard_normal((n_ref, d))
    y = np.column_stack([X[:, 0] * 3.0 + X[:, 1], np.abs(X[:, 2]) * 100.0, rng.integers(0, 12, size=n_ref)])
    px = (X[rng.integers(0, n_ref, size=n)] + 0.05 * rng.standard_normal((n, d))).astype(np.float32)
    cuts = [(a, a + args.tile) for a in range(0, n, args.tile)]
    est_d = sknnr_amd.RawKNNRegressor(n_neighbors=k, weights="distance").fit(X, y)
    est_u = sknnr_amd.RawKNNRegressor(n_neighbors=k, weights="uniform").fit(X, y)
    d64, i64, pred = np.empty((n, k)), np.empty((n, k), dtype=np.int64), np.empty((n, t))
    out = np.empty((n, t))

    def search():
        est_d.predict_chunks((px[a:b] for a, b in cuts), out=pred, return_neighbors=True, neighbors_out=(d64, i64))

    search()
    d32, i32 = d64.astype(np.float32), i64.astype(np.int32)
    pred_u = est_u.predict_chunks((px[a:b] for a, b in cuts))
    flows = {
        "replay int32 + float32 (40 B/pixel in)": lambda: est_d.predict_neighbors_chunks(((d32[a:b], i32[a:b]) for a, b in cuts), out=out),
        "replay int64 + float64 (80 B/pixel in)": lambda: est_d.predict_neighbors_chunks(((d64[a:b], i64[a:b]) for a, b in cuts), out=out),
        "replay int32 alone, uniform (20 B/pixel in)": lambda: est_u.predict_neighbors_chunks((i32[a:b] for a, b in cuts), out=out),
    }
    if not args.replay_only:
        flows = {"search predict_chunks (128 B/pixel in)": search, **flows}
    times = {name: [] for name in flows}
    for name, fn in flows.items():  # warm-up: every shape once
        fn()
    flows["replay int64 + float64 (80 B/pixel in)"]()
    print(f"replay probe: {n_ref} x {d} reference rows, k = {k}, {t} targets; {args.tiles} row tiles of {args.tile} pixels "
          f"(float32 rows); {args.reps} repetitions per flow, alternating; ms per tile of {args.tile} pixels")
    print(f"  replayed (int64, float64) predictions equal the search call's bit for bit: {out.tobytes() == pred.tobytes()}")
    flows["replay int32 alone, uniform (20 B/pixel in)"]()
    print(f"  replayed index-only uniform predictions equal the search call's bit for bit: {out.tobytes() == pred_u.tobytes()}")
    for _ in range(args.reps):
        for name, fn in flows.items():
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3 / args.tiles)
    for name, ms in times.items():
        print(f"  {name:46s} median {np.median(ms):8.2f}   min {min(ms):8.2f}   max {max(ms):8.2f}")
    print(f"  record of the last replayed tile: {est_u.engine_._index.debug_last_replay()}")


if __name__ == "__main__":
    main()

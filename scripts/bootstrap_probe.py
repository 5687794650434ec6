"""The bootstrap stream against the search it rides on, on the shape ``bench.py --full`` streams: 50,000 x 32 reference rows,
k = 5, ``kw`` = 20 candidates, 3 targets, row tiles of 1,000,000 pixels, B of 50, 200 and 1000 replicates.

Flows, in alternation and ``--reps`` times each: ``predict_chunks`` at ``n_neighbors = 5`` (one of the B searches the
bootstrap replaces), ``predict_chunks`` at ``n_neighbors = 20`` (the search the bootstrap rides on), and per B the bootstrap
stream (``predict_chunks(bootstrap=...)``) and the replay-side bootstrap (``bootstrap_neighbors_chunks`` on the
stored int32 + float32 raster of 20 columns).  Every call writes into a preallocated array and ends in the stream's flush,
so the host clock around it covers copies in, kernels and copies out.  Then ``share_short`` at ``kw`` of 12, 16, 20 and 32
next to the binomial estimate: the copies of ``kw`` given rows in one replicate are Binomial(n, kw / n), and the replicate
is short where fewer than k of them turn up.

``--boot-only`` runs the replay-side bootstraps alone, for a kernel trace of their launches:
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/bootstrap_probe.py --boot-only
"""

from __future__ import annotations

import argparse
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def binomial_short(n, kw, k):
    p = kw / n
    return sum(math.comb(n, j) * p**j * (1.0 - p) ** (n - j) for j in range(k))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=2)
    ap.add_argument("--tile", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--boot-only", action="store_true")
    args = ap.parse_args()
    import sknnr_amd

    n_ref, d, k, kw, t = 50_000, 32, 5, 20, 3
    n = args.tiles * args.tile
    rng = np.random.default_rng(0)
    X = rng.standard_normal((n_ref, d))
    y = np.column_stack([X[:, 0] * 3.0 + X[:, 1], np.abs(X[:, 2]) * 100.0, rng.integers(0, 12, size=n_ref)])
    px = (X[rng.integers(0, n_ref, size=n)] + 0.05 * rng.standard_normal((n, d))).astype(np.float32)
    cuts = [(a, a + args.tile) for a in range(0, n, args.tile)]
    est = sknnr_amd.RawKNNRegressor(n_neighbors=k, weights="distance").fit(X, y)
    est_w = sknnr_amd.RawKNNRegressor(n_neighbors=kw, weights="distance").fit(X, y)
    out = np.empty((n, t))
    d32, i32 = np.empty((n, 32), dtype=np.float32), np.empty((n, 32), dtype=np.int32)
    est.kneighbors_chunks((px[a:b] for a, b in cuts), n_neighbors=32, out=(d32, i32), index_dtype=np.int32,
                          distance_dtype=np.float32)
    d20, i20 = np.ascontiguousarray(d32[:, :kw]), np.ascontiguousarray(i32[:, :kw])
    boots = {B: sknnr_amd.Bootstrap(B, seed=B, n_candidates=kw) for B in (50, 200, 1000)}

    def stream(B):
        return lambda: est.predict_chunks((px[a:b] for a, b in cuts), out=out, bootstrap=boots[B])

    def replay(B):
        return lambda: est.bootstrap_neighbors_chunks(((d20[a:b], i20[a:b]) for a, b in cuts), out=out, bootstrap=boots[B])

    base = {} if args.boot_only else {
        "search predict_chunks, n_neighbors = 5": lambda: est.predict_chunks((px[a:b] for a, b in cuts), out=out),
        "search predict_chunks, n_neighbors = 20": lambda: est_w.predict_chunks((px[a:b] for a, b in cuts), out=out)}
    print(f"bootstrap probe: {n_ref} x {d} reference rows, k = {k}, kw = {kw}, {t} targets (boot_se of each), distance weights; "
          f"{args.tiles} row tiles of {args.tile} pixels (float32 rows); per B {args.reps} repetitions per flow, alternating; "
          f"ms per tile of {args.tile} pixels")
    for B in boots:  # (one table at a time: its upload -- once per call sequence with one Bootstrap -- is timed on its own)
        t0 = time.perf_counter()
        est.engine_.set_bootstrap(boots[B]._bind(n_ref))
        print(f"  B = {B}: table drawn, transposed and uploaded in {(time.perf_counter() - t0) * 1e3:.1f} ms")
        flows = dict(base)
        if not args.boot_only:
            flows[f"bootstrap stream, B = {B}"] = stream(B)
        flows[f"bootstrap replay (int32 + float32), B = {B}"] = replay(B)
        times = {name: [] for name in flows}
        for fn in flows.values():  # warm-up: every shape once
            fn()
        if not args.boot_only and B == 200:
            stream(B)()
            a = out.copy()
            stream(B)()
            again = out.tobytes() == a.tobytes()
            replay(B)()
            # (the replay reads float32 distances: equal bits are not expected with distance weights, a close result is)
            with np.errstate(all="ignore"):
                rel = np.nanmax(np.abs(out - a) / np.abs(a))
            print(f"  the stream twice gives equal bits: {again}; the replay from float32 distances differs from it by at most "
                  f"{rel:.3g} relative in boot_se")
        for _ in range(args.reps):
            for name, fn in flows.items():
                t0 = time.perf_counter()
                fn()
                times[name].append((time.perf_counter() - t0) * 1e3 / args.tiles)
        for name, ms in times.items():
            print(f"  {name:48s} median {np.median(ms):8.2f}   min {min(ms):8.2f}   max {max(ms):8.2f}")
        if not args.boot_only:
            one = np.median(times["search predict_chunks, n_neighbors = 5"])
            wide = np.median(times["search predict_chunks, n_neighbors = 20"])
            ms = np.median(times[f"bootstrap stream, B = {B}"])
            print(f"  B = {B:4d}: B searches at k = 5 would take {B * one:10.1f} ms per tile, the bootstrap stream {ms:8.2f}: "
                  f"ratio {B * one / ms:7.1f}; over the search at kw it rides on: {ms - wide:+8.2f} ms ({ms / wide:5.2f} x)")
    print(f"  record of the last reduction: {est.engine_._index.debug_last_bootstrap()}")
    print("  share_short at B = 200 on the first tile, next to the binomial estimate P[Binomial(n, kw / n) < k]:")
    a, b = cuts[0]
    for w in (12, 16, 20, 32):
        bs = sknnr_amd.Bootstrap(200, seed=200)
        est.bootstrap_neighbors_chunks([(d32[a:b], i32[a:b])], out=out[a:b], bootstrap=bs, n_neighbors=w)
        print(f"    kw = {w:3d}: share_short {bs.share_short:.5f}   binomial {binomial_short(n_ref, w, k):.5f}")


if __name__ == "__main__":
    main()

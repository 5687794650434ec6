"""Cost of per-target neighbour summaries on streamed tiles.  A probe, not a test.

    python scripts/neighbor_summary_probe.py [--reps 5] [--out profiles/r12_neighbor_summary.txt]

Workload: the benchmark's index (50,000 x 32 reference rows, k = 5) with three targets -- two continuous, one class code of
seven classes -- and ten tiles of 1M pixels of 32 int16 bands (row tiles), summarised as ``["mean", "std", "mode"]`` into a
preallocated int16 output, scaled per target (the class codes unscaled).  Three flows, interleaved, ``--reps`` repetitions
each, medians and min-max:

  (a) the route without the feature: ``kneighbors_chunks`` streams the (dist, idx) of every pixel back -- k float64 and k
      int64 values each -- and numpy reduces them on the host, then rounds to int16.  The reduction is a hand-written one
      for exactly this workload -- uniform weights, a plain count over the seven known class codes, sums in numpy's default
      order -- which is LIGHTER than the general restatement of the definitions (tests/_neighbor_stats.py: any weights,
      labels found with ``np.unique``, scikit-learn's own mean).  That favours (a): the ratio (a) / (b) is a lower bound
      on what the general host route would give;
  (b) ``predict_chunks(tiles, statistic=["mean", "std", "mode"], out_dtype=int16, ...)``: reduced and narrowed on the device;
  (c) the floor: the same call with ``statistic="mean"`` (the predict kernels alone).

The probe reports (a) / (b), and (b) - (c) against (c)'s own min-max spread: the extra kernel (summary_kernel, k <= 8) reads
(dist, idx) the search just wrote and gathers from targets that fit the L2.
"""

from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

N_REF, D, K, T, TILE, N_TILES, CLASSES = 50_000, 32, 5, 3, 1_000_000, 10, 7
STATISTIC = ["mean", "std", "mode"]
SCALE, OFFSET = np.array([100.0, 100.0, 1.0]), np.zeros(3)


def make_estimator():
    import sknnr_amd

    rng = np.random.default_rng(0)
    x_ref = rng.integers(0, 4000, size=(N_REF, D)).astype(np.float64)
    y = np.stack([rng.standard_normal(N_REF) * 20.0, rng.random(N_REF) * 100.0,
                  rng.integers(0, CLASSES, size=N_REF).astype(np.float64)], axis=1)
    return sknnr_amd.RawKNNRegressor(n_neighbors=K, algorithm="brute").fit(x_ref, y), y


def make_tiles(seed=1):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 4000, size=(TILE, D), dtype=np.int16) for _ in range(N_TILES)]


def to_int16(v, scale, offset):
    return np.clip(np.rint(v * scale + offset), -32768, 32767).astype(np.int16)


def flow_a(est, y, tiles, out):
    """kneighbors_chunks to the host, then numpy: uniform weights, so mean / population std / plain vote."""
    t0 = time.perf_counter()
    idx = est.kneighbors_chunks(iter(tiles), return_distance=False)
    t_search = time.perf_counter() - t0
    t0 = time.perf_counter()
    for a in range(0, idx.shape[0], TILE):
        ii = idx[a:a + TILE]
        v0, v1, v2 = y[ii, 0], y[ii, 1], y[ii, 2]
        out[a:a + TILE, 0] = to_int16(v0.sum(axis=1) / K, SCALE[0], OFFSET[0])
        dv = v1 - (v1.sum(axis=1) / K)[:, None]
        out[a:a + TILE, 1] = to_int16(np.sqrt((dv * dv).sum(axis=1) / K), SCALE[1], OFFSET[1])
        best, best_vote = np.zeros(len(ii)), np.zeros(len(ii))
        for c in range(CLASSES):
            vote = (v2 == c).sum(axis=1)
            best = np.where(vote > best_vote, float(c), best)
            best_vote = np.maximum(vote, best_vote)
        out[a:a + TILE, 2] = to_int16(best, SCALE[2], OFFSET[2])
    return t_search, time.perf_counter() - t0


def flow_b(est, tiles, out, statistic=STATISTIC):
    est.predict_chunks(iter(tiles), out=out, out_dtype=np.int16, scale=SCALE, offset=OFFSET, statistic=statistic)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_neighbor_summary.txt"))
    args = ap.parse_args()
    lines = []

    def log(msg=""):
        print(msg, flush=True)
        lines.append(msg)

    est, y = make_estimator()
    n = N_TILES * TILE
    log(f"neighbour summary probe: {N_REF} x {D} reference rows, k = {K}, {T} targets {STATISTIC}; {N_TILES} tiles of {TILE} pixels x "
        f"{D} int16 bands; int16 output, scaled; {args.reps} repetitions per flow, interleaved; times in ms")
    tiles = make_tiles()
    out_a, out_b, out_c = (np.zeros((n, T), dtype=np.int16) for _ in range(3))
    flow_b(est, tiles[:2], out_b[:2 * TILE])  # (buffers, pinned memory, first launches)
    flow_b(est, tiles[:2], out_c[:2 * TILE], "mean")
    ta, tb, tc, parts = [], [], [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        parts.append(flow_a(est, y, tiles, out_a))
        ta.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        flow_b(est, tiles, out_b)
        tb.append(time.perf_counter() - t0)
        rec = est.engine_._index.debug_last_summary()
        t0 = time.perf_counter()
        flow_b(est, tiles, out_c, "mean")
        tc.append(time.perf_counter() - t0)
    ms = lambda v: 1e3 * np.asarray(v)  # noqa: E731
    fmt = lambda v: f"median {np.median(ms(v)):8.1f}   min {ms(v).min():8.1f}   max {ms(v).max():8.1f}"  # noqa: E731
    p = np.median(ms(parts), axis=0)
    log(f"(a) kneighbors_chunks to host + numpy reduction      {fmt(ta)}   (medians: stream {p[0]:.1f}, numpy {p[1]:.1f})")
    log(f"(b) predict_chunks(statistic=[mean, std, mode])      {fmt(tb)}")
    log(f"(c) floor: predict_chunks(statistic='mean')          {fmt(tc)}")
    med = {k_: float(np.median(ms(v))) for k_, v in (("a", ta), ("b", tb), ("c", tc))}
    spread_c = float(ms(tc).max() - ms(tc).min())
    # (the host route sums in another order than numpy's pairwise sum over k: the mean and the std may differ in the last
    #  bit before rounding to int16, so the flows are compared by how many stored values differ)
    diff = [int((out_a[:, j] != out_b[:, j]).sum()) for j in range(T)]
    log(f"stored values that differ between (a) and (b), per target: {diff} of {n}; mean column of (b) equals (c): "
        f"{np.array_equal(out_b[:, 0], out_c[:, 0])}; last tile of (b): {rec}")
    log(f"(a) / (b) = {med['a'] / med['b']:.2f}x;  (b) - (c) = {med['b'] - med['c']:+.1f} ms against (c)'s min-max spread of "
        f"{spread_c:.1f} ms: {'inside' if med['b'] <= med['c'] + spread_c else 'OUTSIDE'} the floor's run-to-run noise")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

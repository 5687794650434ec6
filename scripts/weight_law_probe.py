"""Cost of a distance-weight law on streamed tiles.  A probe, not a test.

    python scripts/weight_law_probe.py [--reps 5] [--flows abc] [--out profiles/r16_weight_laws.txt]

Workload: the benchmark's index (50,000 x 32 reference rows, k = 5) with three targets and ten tiles of 1M pixels of 32
int16 bands (row tiles), predicted into a preallocated float64 output.  One process, three flows, interleaved, one
warm-up call each, then ``--reps`` repetitions; medians and min-max:

  (a) ``predict_chunks`` with yaImpute's weighting as a plain callable, ``lambda d: 1 / (1 + d)``: the tile-by-tile path --
      every tile's (dist, idx) goes to the host, the callable runs there and the weights come back for the reduction;
  (b) the same with ``sknnr_amd.weights.InverseDistance(1.0)``: one native stream, the weights made on the device by
      weight_law_kernel (16 k bytes of extra traffic per query) in front of the explicit reduction;
  (c) the floor: ``weights="distance"`` on the same build -- the same stream without the law kernel.

The claim to check: (b) lies inside (c)'s own min-max spread.  Also reported: how far (a) is from both, and that (a) and
(b) wrote the same bits.  ``--flows``: which flows run, in which order inside a repetition (``cb``: the floor in front
of the law and no plain callable) -- to tell what a flow costs from what its predecessor leaves behind.
"""

from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

N_REF, D, K, T, TILE, N_TILES = 50_000, 32, 5, 3, 1_000_000, 10


def yaimpute_weights(d):
    return 1.0 / (1.0 + d)


FLOWS = {"a": "(a) predict_chunks, plain callable 1 / (1 + d), tile by tile  ",
         "b": "(b) predict_chunks, InverseDistance(1.0), on the device      ",
         "c": "(c) floor: predict_chunks, weights='distance'                "}


def make_estimators(flows):
    import sknnr_amd
    from sknnr_amd.weights import InverseDistance

    rng = np.random.default_rng(0)
    x_ref = rng.integers(0, 4000, size=(N_REF, D)).astype(np.float64)
    y = np.stack([rng.standard_normal(N_REF) * 20.0, rng.random(N_REF) * 100.0, rng.integers(0, 7, size=N_REF).astype(np.float64)],
                 axis=1)
    weights = {"a": yaimpute_weights, "b": InverseDistance(1.0), "c": "distance"}
    return [sknnr_amd.RawKNNRegressor(n_neighbors=K, algorithm="brute", weights=weights[f]).fit(x_ref, y) for f in flows]


def make_tiles(seed=1):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 4000, size=(TILE, D), dtype=np.int16) for _ in range(N_TILES)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--flows", default="abc", help="the flows to run and their order inside a repetition, e.g. cb")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_weight_laws.txt"))
    args = ap.parse_args()
    lines = []

    def log(msg=""):
        print(msg, flush=True)
        lines.append(msg)

    flows = args.flows
    if not flows or set(flows) - set(FLOWS) or len(set(flows)) != len(flows):
        ap.error("--flows takes each of a, b, c at most once")
    ests = make_estimators(flows)
    n = N_TILES * TILE
    log(f"weight law probe: {N_REF} x {D} reference rows, k = {K}, {T} targets; {N_TILES} tiles of {TILE} pixels x {D} int16 bands; "
        f"float64 output, preallocated; one warm-up call, then {args.reps} repetitions per flow, interleaved in the order {' '.join(flows)}; times in ms")
    tiles = make_tiles()
    outs = [np.zeros((n, T)) for _ in ests]
    for est, out in zip(ests, outs):  # (buffers, pinned memory, first launches)
        est.predict_chunks(iter(tiles), out=out)
    times = [[] for _ in ests]
    recs = [None] * len(ests)
    for _ in range(args.reps):
        for j, (est, out) in enumerate(zip(ests, outs)):
            t0 = time.perf_counter()
            est.predict_chunks(iter(tiles), out=out)
            times[j].append(time.perf_counter() - t0)
            recs[j] = est.engine_._index.debug_last_weight_law()
    ms = lambda v: 1e3 * np.asarray(v)  # noqa: E731
    fmt = lambda v: f"median {np.median(ms(v)):8.1f}   min {ms(v).min():8.1f}   max {ms(v).max():8.1f}"  # noqa: E731
    med, span, out_of = {}, {}, dict(zip(flows, outs))
    for f, v in zip(flows, times):
        log(f"{FLOWS[f]}   {fmt(v)}")
        med[f], span[f] = float(np.median(ms(v))), (float(ms(v).min()), float(ms(v).max()))
    log("last reduction (sknnr_debug_last_weight_law): " + "; ".join(f"({f}) {r}" for f, r in zip(flows, recs)))
    if "a" in med and "b" in med:
        log(f"(a) and (b) wrote the same bits: {np.array_equal(out_of['a'], out_of['b'])};  (a) / (b) = {med['a'] / med['b']:.2f}x"
            + (f",  (a) / (c) = {med['a'] / med['c']:.2f}x" if "c" in med else ""))
    if "b" in med and "c" in med:
        lo, hi = span["c"]
        log(f"(b) - (c) = {med['b'] - med['c']:+.1f} ms; (c)'s min-max {lo:.1f} .. {hi:.1f} ms: (b)'s median is "
            f"{'inside' if lo <= med['b'] <= hi else 'OUTSIDE'} the floor's own spread")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

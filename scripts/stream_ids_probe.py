"""Cost of dataframe ids and of neighbours beside predictions in the streamed raster calls.  A probe, not a test.

    python scripts/stream_ids_probe.py --parent DIR [--reps 5] [--rounds 2] [--out profiles/r14_stream_ids.txt]
    python scripts/stream_ids_probe.py --child --root DIR --reps N      # one process of the above: prints one JSON line

Workload: the benchmark's index (50,000 x 32 reference rows, k = 5) with 3 targets and an int64 dataframe index, ten
windows of 1M pixels of 32 int16 bands (row tiles), every output preallocated.

  (a) ``kneighbors_chunks(return_dataframe_index=True, index_dtype=np.int32)``: the parent commit (ids looked up by the
      host, in place, after the stream) against this change (looked up on the device, inside the index conversion).
      ``--parent`` names a checkout of the parent commit with its library built; processes alternate parent / this
      change, ``--rounds`` times, and each runs ``--reps`` repetitions after a warm-up call.
  (b) this change only: ``kneighbors_chunks`` followed by ``predict_chunks`` (two searches) against one
      ``predict_chunks(return_neighbors=True)`` with the same outputs.
  (c) the floor of each: the same calls with row indices (no ids).

Medians, min and max in ms; the one-call results of (b) are compared with the two-call ones once per process.
"""

from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
N_REF, D, K, T, TILE, N_TILES = 50_000, 32, 5, 3, 1_000_000, 10


def child(root, reps):
    sys.path.insert(0, root)
    import pandas as pd
    import sknnr_amd

    rng = np.random.default_rng(0)
    ids = rng.permutation(N_REF).astype(np.int64) * 3 + 100_000
    x_ref = pd.DataFrame(rng.integers(0, 4000, size=(N_REF, D)).astype(np.float64), index=ids)
    est = sknnr_amd.RawKNNRegressor(n_neighbors=K, algorithm="brute").fit(x_ref, rng.standard_normal((N_REF, T)))
    rng = np.random.default_rng(1)
    tiles = [rng.integers(0, 4000, size=(TILE, D), dtype=np.int16) for _ in range(N_TILES)]
    n = N_TILES * TILE
    dist, idx, pred = np.zeros((n, K)), np.zeros((n, K), dtype=np.int32), np.zeros((n, T))
    has_b = "return_neighbors" in est.predict_chunks.__code__.co_varnames

    def kn(with_ids, t=tiles):
        est.kneighbors_chunks(iter(t), return_dataframe_index=with_ids, index_dtype=np.int32, out=(dist, idx))

    def two(with_ids, t=tiles):
        kn(with_ids, t)
        est.predict_chunks(iter(t), out=pred)

    def one(with_ids, t=tiles):
        est.predict_chunks(iter(t), out=pred, return_neighbors=True, return_dataframe_index=with_ids,
                           index_dtype=np.int32, neighbors_out=(dist, idx))

    flows = {"a_ids": lambda: kn(True), "a_floor": lambda: kn(False)}
    if has_b:
        flows.update({"b_two_calls_ids": lambda: two(True), "b_one_call_ids": lambda: one(True),
                      "b_two_calls_floor": lambda: two(False), "b_one_call_floor": lambda: one(False)})
    kn(True, tiles[:2])  # (buffers, pinned memory, first launches)
    two(True, tiles[:2])
    equal = None
    if has_b:
        two(True)
        want = (dist.copy(), idx.copy(), pred.copy())
        dist[...], idx[...], pred[...] = 0, 0, 0
        one(True)
        equal = all(np.array_equal(g, w) for g, w in zip((dist, idx, pred), want))
    times = {name: [] for name in flows}
    for _ in range(reps):
        for name, run in flows.items():
            t0 = time.perf_counter()
            run()
            times[name].append(1e3 * (time.perf_counter() - t0))
    rec = est.engine_._index.debug_last_narrow()
    print(json.dumps({"times": times, "one_call_equals_two_calls": equal, "last_tile": rec}), flush=True)


def run_child(root, reps):
    """One child process under a time limit of its own; returns its record, or raises with the end of its output."""
    proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--reps", str(reps)],
                          capture_output=True, text=True, timeout=600)
    if proc.returncode != 0:
        raise RuntimeError(f"child on {root} ended with {proc.returncode}: {proc.stderr[-2000:]}")
    return json.loads(proc.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r14_stream_ids.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default=HERE)
    args = ap.parse_args()
    if args.child:
        return child(os.path.abspath(args.root), args.reps)

    lines = []

    def log(msg=""):
        print(msg, flush=True)
        lines.append(msg)

    log(f"stream ids probe: {N_REF} x {D} reference rows, k = {K}, {T} targets, int64 dataframe ids; {N_TILES} row tiles of "
        f"{TILE} pixels x {D} int16 bands; preallocated outputs (float64 distances, int32 ids, float64 predictions); "
        f"{args.reps} repetitions per flow and process, {args.rounds} processes per commit, alternating parent / this "
        "change; times in ms")
    pooled = {}
    for r in range(args.rounds):
        for who, root in (("parent", args.parent), ("this change", HERE)):
            if root is None:
                continue
            rec = run_child(os.path.abspath(root), args.reps)
            for name, v in rec["times"].items():
                pooled.setdefault((who, name), []).extend(v)
                log(f"  {who:12s} process {r + 1}  {name:18s} median {np.median(v):8.1f}   min {min(v):8.1f}   max {max(v):8.1f}")
            log(f"  {who:12s} process {r + 1}  one call equals two calls: {rec['one_call_equals_two_calls']}; last tile: {rec['last_tile']}")
    log("pooled over processes:")
    med = {}
    for (who, name), v in pooled.items():
        med[(who, name)] = float(np.median(v))
        log(f"  {who:12s} {name:18s} median {np.median(v):8.1f}   min {min(v):8.1f}   max {max(v):8.1f}   n = {len(v)}")
    new = "this change"
    if ("parent", "a_ids") in med:
        p, c = med[("parent", "a_ids")], med[(new, "a_ids")]
        log(f"(a) ids as int32: parent {p:.1f}, this change {c:.1f}: {p / c:.2f}x; over their floors (row indices): parent "
            f"{p - med[('parent', 'a_floor')]:+.1f}, this change {c - med[(new, 'a_floor')]:+.1f}")
    if (new, "b_one_call_ids") in med:
        two, one = med[(new, "b_two_calls_ids")], med[(new, "b_one_call_ids")]
        log(f"(b) ids + distances + predictions: two calls {two:.1f}, one call {one:.1f}: ratio {one / two:.2f}; floor (row "
            f"indices): two calls {med[(new, 'b_two_calls_floor')]:.1f}, one call {med[(new, 'b_one_call_floor')]:.1f}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

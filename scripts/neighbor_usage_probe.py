"""Cost of neighbour usage (``usage=``) in the streamed raster calls, against the host alternative and against the plain
one-atomic-per-entry kernel.  A probe, not a test.

    python scripts/neighbor_usage_probe.py --parent DIR [--plain LIB] [--reps 5] [--rounds 2] [--out profiles/r20_neighbor_usage.txt]
    python scripts/neighbor_usage_probe.py --child --root DIR --reps N      # one process of the above: prints one JSON line

Workload (that of profiles/r14_stream_ids.txt): 50,000 x 32 reference rows, k = 5, 3 targets; ten row tiles of 1,000,000
pixels x 32 int16 bands; ``predict_chunks`` into a preallocated int16 raster (scale 100, nodata -32768).

Data laws.  The reference rows are uniform integers in [0, 4000) in both.
  random    every pixel's bands are uniform integers in [0, 4000) (``numpy.random.Generator.integers``): neighbouring pixels
            share nothing, every lane of a wave tallies another reference row.
  coherent  a tile is a 1,000 x 1,000 window, row-major; it is cut into blocks of 40 x 40 pixels, every block takes one
            reference row (drawn at random) as its surface, and every pixel is that row plus uniform integer noise in
            [-3, 3] per band, clipped to [0, 3999]: a smooth field with sharp patch borders, as a classified landscape
            gives.  Runs of 40 consecutive pixels share their neighbours.
The mean run length of equal FIRST neighbours over the first tile is measured and printed for both laws.

Flows, per law:
  (a) predictions only                                                parent commit and this change
  (b) the same call with ``usage=u``                                  this change
  (c) the host alternative on this change: ``return_neighbors=True, index_dtype=np.int32`` into preallocated arrays,
      then ``np.bincount`` per rank and ``np.maximum.at`` over the N * k entries
  (d) flow (b) under a library built with -DSKNNR_TALLY_PLAIN (``--plain``: its path; the plain kernel: one global
      atomic per entry, no LDS table), loaded through SKNNR_HIP_LIBRARY -- never linked over the product library
  kernel  the tally kernel alone on one tile's neighbours in device memory (sknnr_tally_from_neighbors, accumulate = 0:
          two memsets of 2.4 MB included), timed with device events over 20 launches

``--parent`` names a checkout of the parent commit with its library built.  Processes alternate parent / this change
(parent first) / plain, ``--rounds`` times; each runs ``--reps`` repetitions of (a) and (b) after a warm-up call and two
of (c).  Medians, min and max in ms.  Every child runs under a time limit of its own; the first that fails ends the probe.
"""

from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
N_REF, D, K, T, SIDE, N_TILES = 50_000, 32, 5, 3, 1_000, 10
TILE = SIDE * SIDE
BLOCK = 40
LAWS = ("random", "coherent")


def make_tiles(law, x_ref):
    rng = np.random.default_rng({"random": 1, "coherent": 2}[law])
    if law == "random":
        return [rng.integers(0, 4000, size=(TILE, D), dtype=np.int16) for _ in range(N_TILES)]
    tiles = []
    nb = SIDE // BLOCK
    for _ in range(N_TILES):
        owner = rng.integers(0, N_REF, size=(nb, nb))
        owner = np.repeat(np.repeat(owner, BLOCK, axis=0), BLOCK, axis=1).reshape(-1)
        px = x_ref[owner].astype(np.int16) + rng.integers(-3, 4, size=(TILE, D), dtype=np.int16)
        tiles.append(np.clip(px, 0, 3999).astype(np.int16))
    return tiles


def mean_run_length(first):
    return float(len(first) / (1 + np.count_nonzero(first[1:] != first[:-1])))


def child(root, reps):
    sys.path.insert(0, root)
    import sknnr_amd

    rng = np.random.default_rng(0)
    x_ref = rng.integers(0, 4000, size=(N_REF, D)).astype(np.float64)
    est = sknnr_amd.RawKNNRegressor(n_neighbors=K, algorithm="brute").fit(x_ref, rng.standard_normal((N_REF, T)))
    has_usage = hasattr(sknnr_amd, "NeighborUsage")
    n = N_TILES * TILE
    pred = np.zeros((n, T), dtype=np.int16)
    typed = dict(out=pred, out_dtype=np.int16, scale=100.0, out_nodata=-32768)
    out = {"times": {}, "runs": {}, "kernel_ms": {}, "record": {}, "equal": {}}
    for law in LAWS:
        tiles = make_tiles(law, x_ref)
        est.predict_chunks(iter(tiles[:2]), **{**typed, "out": pred[:2 * TILE]})  # (buffers, pinned memory, first launches)

        def flow_a():
            est.predict_chunks(iter(tiles), **typed)

        flows = {"a": flow_a}
        if has_usage:
            dist, idx = np.zeros((n, K)), np.zeros((n, K), dtype=np.int32)
            last = {}

            def flow_b():
                last["u"] = sknnr_amd.NeighborUsage()
                est.predict_chunks(iter(tiles), usage=last["u"], **typed)

            def flow_c():
                est.predict_chunks(iter(tiles), return_neighbors=True, index_dtype=np.int32, neighbors_out=(dist, idx), **typed)
                counts = np.stack([np.bincount(idx[:, j], minlength=N_REF) for j in range(K)], axis=1)
                mx = np.zeros(N_REF)
                np.maximum.at(mx, idx.reshape(-1), dist.reshape(-1))
                last["host"] = (counts, mx)

            flows.update(b=flow_b, c=flow_c)
            est.predict_chunks(iter(tiles[:2]), usage=sknnr_amd.NeighborUsage(), **{**typed, "out": pred[:2 * TILE]})
        for name, run in flows.items():
            times = []
            for _ in range(min(reps, 2) if name == "c" else reps):
                t0 = time.perf_counter()
                run()
                times.append(1e3 * (time.perf_counter() - t0))
            out["times"][f"{law}/{name}"] = times
        if has_usage:
            import torch

            u, (counts, mx) = last["u"], last["host"]
            out["equal"][law] = bool(np.array_equal(u.counts, counts) and  # (NaN: the rows no pixel used)
                                     np.array_equal(u.max_distance, np.where(counts.sum(1) == 0, np.nan, mx), equal_nan=True))
            out["unused"] = out.get("unused", {})
            out["unused"][law] = int(u.unused.sum())
            out["runs"][law] = mean_run_length(idx[:TILE, 0])
            ix = est.engine_._index
            out["record"][law] = ix.debug_last_tally()  # (the stream of the last flow (b): all ten tiles)
            ti = torch.from_numpy(idx[:TILE].astype(np.int64)).cuda()
            td = torch.from_numpy(dist[:TILE].copy()).cuda()
            tc = torch.empty((N_REF, K), dtype=torch.int64, device="cuda")
            tm = torch.empty((N_REF,), dtype=torch.float64, device="cuda")
            st = torch.cuda.current_stream().cuda_stream
            launch = lambda: ix.tally_from_neighbors_device(td.data_ptr(), ti.data_ptr(), TILE, K, tc.data_ptr(),  # noqa: E731
                                                            tm.data_ptr(), False, st)
            launch()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                launch()
            e1.record()
            torch.cuda.synchronize()
            out["kernel_ms"][law] = e0.elapsed_time(e1) / 20
            out["record_tile"] = out.get("record_tile", {})
            out["record_tile"][law] = ix.debug_last_tally()
            del dist, idx
        del tiles
    print(json.dumps(out), flush=True)


def run_child(root, reps, library=None):
    """One child process under a time limit of its own; returns its record, or raises with the end of its output."""
    env = dict(os.environ)
    if library:
        env["SKNNR_HIP_LIBRARY"] = os.path.abspath(library)
    proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--reps", str(reps)],
                          capture_output=True, text=True, timeout=900, env=env)
    if proc.returncode != 0:
        raise RuntimeError(f"child on {root} ended with {proc.returncode}: {proc.stderr[-2000:]}")
    return json.loads(proc.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--plain", default=None, help="a library of this change built with -DSKNNR_TALLY_PLAIN")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r20_neighbor_usage.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default=HERE)
    args = ap.parse_args()
    if args.child:
        return child(os.path.abspath(args.root), args.reps)

    lines = []

    def log(msg=""):
        print(msg, flush=True)
        lines.append(msg)

    log(f"neighbour usage probe: {N_REF} x {D} reference rows, k = {K}, {T} targets; {N_TILES} row tiles of {TILE} pixels x {D} "
        f"int16 bands; predict_chunks into a preallocated int16 raster; {args.reps} repetitions per flow and process (two of "
        f"(c)), {args.rounds} processes per build, alternating parent / this change / plain kernel; times in ms")
    pooled, kernel, runs = {}, {}, {}
    for r in range(args.rounds):
        for who, root, lib in (("parent", args.parent, None), ("this change", HERE, None), ("plain kernel", HERE, args.plain)):
            if root is None or (who == "plain kernel" and lib is None):
                continue
            rec = run_child(os.path.abspath(root), args.reps, lib)
            for name, v in rec["times"].items():
                pooled.setdefault((who, name), []).extend(v)
                log(f"  {who:12s} process {r + 1}  {name:12s} median {np.median(v):8.1f}   min {min(v):8.1f}   max {max(v):8.1f}")
            for law, ms in rec["kernel_ms"].items():
                kernel.setdefault((who, law), []).append(ms)
                runs[law] = rec["runs"][law]
                log(f"  {who:12s} process {r + 1}  {law}: usage equals the host alternative: {rec['equal'][law]} "
                    f"({rec['unused'][law]} of {N_REF} rows unused); tally kernel "
                    f"alone {ms:.3f} ms per tile; record of one tile {rec['record_tile'][law]}; of the stream {rec['record'][law]}")
    log("pooled over processes:")
    med = {}
    for (who, name), v in pooled.items():
        med[(who, name)] = float(np.median(v))
        log(f"  {who:12s} {name:12s} median {np.median(v):8.1f}   min {min(v):8.1f}   max {max(v):8.1f}   n = {len(v)}")
    new = "this change"
    for law in LAWS:
        log(f"{law}: mean run length of equal first neighbours over the first tile: {runs.get(law, float('nan')):.2f}")
        a = med[(new, f"{law}/a")]
        if ("parent", f"{law}/a") in med:
            pv = pooled[("parent", f"{law}/a")]
            log(f"  (a) parent {med[('parent', f'{law}/a')]:.1f} (its own spread {min(pv):.1f} .. {max(pv):.1f}), this change {a:.1f}")
        if (new, f"{law}/b") in med:
            b, c = med[(new, f"{law}/b")], med[(new, f"{law}/c")]
            log(f"  (b) - (a) = {b - a:+.1f}   (c) - (a) = {c - a:+.1f}")
            log(f"  tally kernel alone, LDS table: {np.median(kernel[(new, law)]):.3f} ms per tile")
        if ("plain kernel", f"{law}/b") in med:
            log(f"  (d) plain kernel: (b) {med[('plain kernel', f'{law}/b')]:.1f} against (a) {med[('plain kernel', f'{law}/a')]:.1f} "
                f"in the same processes: {med[('plain kernel', f'{law}/b')] - med[('plain kernel', f'{law}/a')]:+.1f}; "
                f"kernel alone {np.median(kernel[('plain kernel', law)]):.3f} ms per tile")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Cost of zonal statistics (``zones=`` / ``zonal=``) in the streamed raster calls, against the host alternative and against
the plain every-entry-to-global-atomics kernel.  A probe, not a test.

    python scripts/zonal_probe.py --parent DIR [--plain LIB] [--reps 5] [--rounds 2] [--out profiles/r21_zonal.txt]
    python scripts/zonal_probe.py --child --root DIR --reps N      # one process of the above: prints one JSON line

Workload (that of profiles/r20_neighbor_usage.txt): 50,000 x 32 reference rows, k = 5, 3 targets; ten row tiles of
1,000,000 pixels x 32 int16 bands, every band uniform integers in [0, 4000); ``predict_chunks`` into a preallocated int16
raster (scale 100, nodata -32768).  A tile is a 1,000 x 1,000 window, row-major; the raster is the ten windows stacked.

Zone laws, 1,000 zones in both:
  coherent  rectangular blocks of 100 x 100 pixels: 100 blocks per window, a zone of its own each.  Runs of 100
            consecutive pixels share their zone, and a workgroup's ~2,730 pixels touch at most 4 zones.
  random    every pixel's code is uniform in [0, 1000): every lane of a wave tallies another zone.

Flows, per law:
  (a) predictions only                                                parent commit and this change
  (b) the same call with ``zones=`` / ``zonal=``                      this change
  (c) the host alternative on this change: flow (a), then per plane over the written raster ``np.bincount`` of the
      count, the sum and the sum of squares and ``np.minimum.at`` / ``np.maximum.at``
  (d) flow (b) under a library built with -DSKNNR_ZONAL_PLAIN (``--plain``: its path; no LDS table), loaded through
      SKNNR_HIP_LIBRARY -- never linked over the product library
  kernel  the zonal kernel alone on one tile's float64 predictions in device memory (sknnr_zonal_from_values,
          accumulate = 0: the initialisation of 144 KB included), timed with device events over 20 launches

``--parent`` names a checkout of the parent commit with its library built.  Processes alternate parent / this change /
plain, ``--rounds`` times; each runs ``--reps`` repetitions of (a) and (b) after a warm-up call and two of (c).  Medians,
min and max in ms.  Every child runs under a time limit of its own; the first that fails ends the probe.
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
BLOCK, N_ZONES = 100, 1_000
LAWS = ("coherent", "random")


def make_zones(law):
    if law == "random":
        rng = np.random.default_rng(3)
        return [rng.integers(0, N_ZONES, size=TILE, dtype=np.int32) for _ in range(N_TILES)]
    nb = SIDE // BLOCK
    block = np.repeat(np.repeat(np.arange(nb * nb).reshape(nb, nb), BLOCK, axis=0), BLOCK, axis=1).reshape(-1)
    return [(block + i * nb * nb).astype(np.int32) for i in range(N_TILES)]


def child(root, reps):
    sys.path.insert(0, root)
    import sknnr_amd

    rng = np.random.default_rng(0)
    x_ref = rng.integers(0, 4000, size=(N_REF, D)).astype(np.float64)
    est = sknnr_amd.RawKNNRegressor(n_neighbors=K, algorithm="brute").fit(x_ref, rng.standard_normal((N_REF, T)))
    has_zonal = hasattr(sknnr_amd, "ZonalStats")
    n = N_TILES * TILE
    pred = np.zeros((n, T), dtype=np.int16)
    typed = dict(out=pred, out_dtype=np.int16, scale=100.0, out_nodata=-32768)
    rng = np.random.default_rng(1)
    tiles = [rng.integers(0, 4000, size=(TILE, D), dtype=np.int16) for _ in range(N_TILES)]
    est.predict_chunks(iter(tiles[:2]), **{**typed, "out": pred[:2 * TILE]})  # (buffers, pinned memory, first launches)
    out = {"times": {}, "kernel_ms": {}, "record": {}, "record_tile": {}, "equal": {}}
    for law in LAWS:
        zones = make_zones(law)

        def flow_a():
            est.predict_chunks(iter(tiles), **typed)

        flows = {"a": flow_a}
        if has_zonal:
            last = {}
            all_zones = np.concatenate(zones)

            def flow_b():
                last["z"] = sknnr_amd.ZonalStats(N_ZONES)
                est.predict_chunks(iter(tiles), zones=iter(zones), zonal=last["z"], **typed)

            def flow_c():
                est.predict_chunks(iter(tiles), **typed)
                cols = []
                for j in range(T):
                    q = pred[:, j].astype(np.float64)
                    mn, mx = np.full(N_ZONES, np.inf), np.full(N_ZONES, -np.inf)
                    np.minimum.at(mn, all_zones, q)
                    np.maximum.at(mx, all_zones, q)
                    cols.append((np.bincount(all_zones, minlength=N_ZONES), np.bincount(all_zones, weights=q, minlength=N_ZONES),
                                 np.bincount(all_zones, weights=q * q, minlength=N_ZONES), mn, mx))
                last["host"] = cols

            flows.update(b=flow_b, c=flow_c)
            est.predict_chunks(iter(tiles[:2]), zones=iter(zones[:2]), zonal=sknnr_amd.ZonalStats(N_ZONES),
                               **{**typed, "out": pred[:2 * TILE]})
        for name, run in flows.items():
            times = []
            for _ in range(min(reps, 2) if name == "c" else reps):
                t0 = time.perf_counter()
                run()
                times.append(1e3 * (time.perf_counter() - t0))
            out["times"][f"{law}/{name}"] = times
        if has_zonal:
            import torch

            z, cols = last["z"], last["host"]
            out["equal"][law] = bool(all(np.array_equal(z.count[:, j], c[0]) and np.array_equal(z.sum_stored[:, j], c[1])
                                         and np.array_equal(z.min_stored[:, j], c[3]) and np.array_equal(z.max_stored[:, j], c[4])
                                         for j, c in enumerate(cols)))
            ix = est.engine_._index
            out["record"][law] = ix.debug_last_zonal()  # (the stream of the last flow (b): all ten tiles)
            tv = torch.from_numpy(pred[:TILE].astype(np.float64) / 100.0).cuda()
            tz = torch.from_numpy(zones[0]).cuda()
            ta = torch.empty((N_ZONES, T, 6), dtype=torch.int64, device="cuda")
            st = torch.cuda.current_stream().cuda_stream
            scale, offset = np.full(T, 100.0), np.zeros(T)
            launch = lambda: ix.zonal_from_values_device(tv.data_ptr(), tz.data_ptr(), TILE, T, np.dtype(np.int16), N_ZONES,  # noqa: E731
                                                         ta.data_ptr(), 0, scale=scale, offset=offset, stream=st)
            launch()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                launch()
            e1.record()
            torch.cuda.synchronize()
            out["kernel_ms"][law] = e0.elapsed_time(e1) / 20
            out["record_tile"][law] = ix.debug_last_zonal()
    print(json.dumps(out), flush=True)


def run_child(root, reps, library=None):
    """One child process under a time limit of its own; returns its record, or raises with the end of its output."""
    env = dict(os.environ)
    if library:
        env["SKNNR_HIP_LIBRARY"] = os.path.abspath(library)
    proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--reps", str(reps)],
                          capture_output=True, text=True, timeout=600, env=env)
    if proc.returncode != 0:
        raise RuntimeError(f"child on {root} ended with {proc.returncode}: {proc.stderr[-2000:]}")
    return json.loads(proc.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--plain", default=None, help="a library of this change built with -DSKNNR_ZONAL_PLAIN")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r21_zonal.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default=HERE)
    args = ap.parse_args()
    if args.child:
        return child(os.path.abspath(args.root), args.reps)

    lines = []

    def log(msg=""):
        print(msg, flush=True)
        lines.append(msg)

    log(f"zonal probe: {N_REF} x {D} reference rows, k = {K}, {T} targets; {N_TILES} row tiles of {TILE} pixels x {D} int16 "
        f"bands; {N_ZONES} zones; predict_chunks into a preallocated int16 raster; {args.reps} repetitions per flow and process "
        f"(two of (c)), {args.rounds} processes per build, alternating parent / this change / plain kernel; times in ms")
    pooled, kernel = {}, {}
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
                log(f"  {who:12s} process {r + 1}  {law}: zonal tables equal the host alternative: {rec['equal'][law]}; zonal kernel "
                    f"alone {ms:.3f} ms per tile; record of one tile {rec['record_tile'][law]}; of the stream {rec['record'][law]}")
    log("pooled over processes:")
    med = {}
    for (who, name), v in pooled.items():
        med[(who, name)] = float(np.median(v))
        log(f"  {who:12s} {name:12s} median {np.median(v):8.1f}   min {min(v):8.1f}   max {max(v):8.1f}   n = {len(v)}")
    new = "this change"
    for law in LAWS:
        log(f"{law} zones:")
        a = med[(new, f"{law}/a")]
        if ("parent", f"{law}/a") in med:
            pv = pooled[("parent", f"{law}/a")]
            log(f"  (a) parent {med[('parent', f'{law}/a')]:.1f} (its own spread {min(pv):.1f} .. {max(pv):.1f}), this change {a:.1f}")
        if (new, f"{law}/b") in med:
            b, c = med[(new, f"{law}/b")], med[(new, f"{law}/c")]
            log(f"  (b) - (a) = {b - a:+.1f}   (c) - (a) = {c - a:+.1f}")
            log(f"  zonal kernel alone, LDS table: {np.median(kernel[(new, law)]):.3f} ms per tile")
        if ("plain kernel", f"{law}/b") in med:
            log(f"  (d) plain kernel: (b) {med[('plain kernel', f'{law}/b')]:.1f} against (a) {med[('plain kernel', f'{law}/a')]:.1f} "
                f"in the same processes: {med[('plain kernel', f'{law}/b')] - med[('plain kernel', f'{law}/a')]:+.1f}; "
                f"kernel alone {np.median(kernel[('plain kernel', law)]):.3f} ms per tile")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Cost of the distance-domain lane (``domain=`` / ``domain_out=``) in the streamed raster calls, against the host
alternative and against the plain kernel (whole search in global memory, one global atomic per pixel).  A probe, not a test.

    python scripts/distance_domain_probe.py --parent DIR [--plain LIB] [--reps 5] [--rounds 2] [--change-first] [--out profiles/r23_distance_domain.txt]
    python scripts/distance_domain_probe.py --child --root DIR --reps N      # one process of the above: prints one JSON line

Workload (that of scripts/neighbor_usage_probe.py): 50,000 x 32 reference rows, k = 5, 3 targets; ten row tiles of
1,000,000 pixels x 32 int16 bands; ``predict_chunks`` into a preallocated int16 raster (scale 100, nodata -32768).  The
domain is ``est.distance_domain(p=0.05)``: the 50,000 leave-one-out nearest-neighbour distances of the reference rows, the
threshold at their 95th percentile, rank 1.

Data laws.  The reference rows are uniform integers in [0, 4000) in both.
  random    every pixel's bands are uniform integers in [0, 4000): neighbouring pixels share nothing; their distances
            are those of the reference rows among themselves, so the codes spread over all of 0 .. 100.
  coherent  a tile is a 1,000 x 1,000 window, row-major, cut into blocks of 40 x 40 pixels; every block takes one
            reference row (drawn at random) as its surface, and every pixel is that row plus uniform integer noise in
            [-3, 3] per band, clipped to [0, 3999].  Every pixel lies close to a reference row: the codes are all 0, and
            every lane of every wave bumps the same counter.

Flows, per law:
  (a) predictions only                                                parent commit and this change
  (b) the same call with ``domain=d, domain_out=plane``               this change
  (c) the host alternative on this change: ``return_neighbors=True, distance_dtype=np.float32`` into preallocated
      arrays, then ``np.searchsorted`` on the first column, the integer division, ``np.bincount`` and the count above the
      threshold
  (d) flow (b) under a library built with -DSKNNR_DOMAIN_PLAIN (``--plain``: its path), loaded through
      SKNNR_HIP_LIBRARY -- never linked over the product library
  kernel  the domain kernel on float64 distances in device memory (sknnr_domain_from_neighbors, codes and tallies).
          Every call of that entry also waits for its stream and uploads the table (0.1 ms, more than the kernel takes on
          one tile), so 20 calls on all 10,000,000 pixels are timed against 20 calls on 1 pixel with device events; the
          difference, divided by ten, is the kernel's time per tile of 1,000,000 pixels
The codes and the accumulators of (b) are compared with the numpy statement of the contract on the FLOAT64 distances of
an untimed pass (flow (c)'s float32 distances round some scores across a table entry; how many codes that moves is
printed too).

``--parent`` names a checkout of the parent commit with its library built.  Processes alternate parent / this change
(parent first; ``--change-first`` swaps the two) / plain, ``--rounds`` times; each runs ``--reps`` repetitions of (a) and (b) after a warm-up call and two
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


def child(root, reps):
    sys.path.insert(0, root)
    import sknnr_amd

    rng = np.random.default_rng(0)
    x_ref = rng.integers(0, 4000, size=(N_REF, D)).astype(np.float64)
    est = sknnr_amd.RawKNNRegressor(n_neighbors=K, algorithm="brute").fit(x_ref, rng.standard_normal((N_REF, T)))
    has_domain = hasattr(sknnr_amd, "DistanceDomain")
    n = N_TILES * TILE
    pred = np.zeros((n, T), dtype=np.int16)
    typed = dict(out=pred, out_dtype=np.int16, scale=100.0, out_nodata=-32768)
    out = {"times": {}, "kernel_ms": {}, "call_ms": {}, "record": {}, "equal": {}, "moved32": {}, "share": {}, "codes": {}}
    if has_domain:
        proto = est.distance_domain(p=0.05)
        out["m"] = int(proto.table.size)
        out["threshold"] = proto.threshold
    for law in LAWS:
        tiles = make_tiles(law, x_ref)
        est.predict_chunks(iter(tiles[:2]), **{**typed, "out": pred[:2 * TILE]})  # (buffers, pinned memory, first launches)

        def flow_a():
            est.predict_chunks(iter(tiles), **typed)

        flows = {"a": flow_a}
        if has_domain:
            dist32, idx = np.zeros((n, K), dtype=np.float32), np.zeros((n, K), dtype=np.int64)
            plane = np.zeros(n, dtype=np.uint8)
            last = {}
            table, m, thr = proto.table, proto.table.size, proto.threshold

            def flow_b():
                last["d"] = sknnr_amd.DistanceDomain(table, threshold=thr)
                est.predict_chunks(iter(tiles), domain=last["d"], domain_out=plane, **typed)

            def flow_c():
                est.predict_chunks(iter(tiles), return_neighbors=True, distance_dtype=np.float32, neighbors_out=(dist32, idx),
                                   **typed)
                s = dist32[:, 0]
                codes = ((100 * np.searchsorted(table, s, side="left")) // m).astype(np.uint8)
                last["host"] = (codes, np.bincount(codes, minlength=101), int(np.count_nonzero(s > thr)))

            flows.update(b=flow_b, c=flow_c)
            est.predict_chunks(iter(tiles[:2]), domain=sknnr_amd.DistanceDomain(table, threshold=thr),
                               domain_out=plane[:2 * TILE], **{**typed, "out": pred[:2 * TILE]})
        for name, run in flows.items():
            times = []
            for _ in range(min(reps, 2) if name == "c" else reps):
                t0 = time.perf_counter()
                run()
                times.append(1e3 * (time.perf_counter() - t0))
            out["times"][f"{law}/{name}"] = times
        if has_domain:
            import torch

            ix = est.engine_._index
            out["record"][law] = ix.debug_last_domain()  # (the stream of the last flow (b): all ten tiles)
            # the check: the contract in numpy on the float64 distances of an untimed pass
            dist64 = np.zeros((n, K))
            est.predict_chunks(iter(tiles), return_neighbors=True, neighbors_out=(dist64, idx), **typed)
            want = proto.percent(dist64[:, 0])
            d = last["d"]
            out["equal"][law] = bool(np.array_equal(plane, want) and np.array_equal(d.hist, np.bincount(want, minlength=101))
                                     and d.n_beyond == int(np.count_nonzero(dist64[:, 0] > thr)) and d.n_nodata == 0)
            out["moved32"][law] = int(np.count_nonzero(last["host"][0] != want))
            out["share"][law] = d.share_beyond
            out["codes"][law] = int(np.count_nonzero(d.hist))
            td = torch.from_numpy(dist64).cuda()
            tc = torch.empty((n,), dtype=torch.uint8, device="cuda")
            ta = torch.empty((103,), dtype=torch.int64, device="cuda")
            st = torch.cuda.current_stream().cuda_stream

            def per_call(pixels):
                launch = lambda: ix.domain_from_neighbors_device(td.data_ptr(), pixels, K, table, 1, thr,  # noqa: E731
                                                                 tc.data_ptr(), ta.data_ptr(), False, st)
                launch()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    launch()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / 20

            small, full = per_call(1), per_call(n)
            out["call_ms"][law] = [small, full]
            out["kernel_ms"][law] = (full - small) / N_TILES
            out["record_tile"] = out.get("record_tile", {})
            out["record_tile"][law] = ix.debug_last_domain()
            del dist32, dist64, idx, plane
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
    ap.add_argument("--plain", default=None, help="a library of this change built with -DSKNNR_DOMAIN_PLAIN")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--change-first", action="store_true", help="every round runs this change in front of the parent")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r23_distance_domain.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default=HERE)
    args = ap.parse_args()
    if args.child:
        return child(os.path.abspath(args.root), args.reps)

    lines = []

    def log(msg=""):
        print(msg, flush=True)
        lines.append(msg)

    log(f"distance domain probe: {N_REF} x {D} reference rows, k = {K}, {T} targets; {N_TILES} row tiles of {TILE} pixels x {D} "
        f"int16 bands; predict_chunks into a preallocated int16 raster; {args.reps} repetitions per flow and process (two of "
        f"(c)), {args.rounds} processes per build, alternating parent / this change / plain kernel; times in ms")
    pooled, kernel = {}, {}
    for r in range(args.rounds):
        order = [("parent", args.parent, None), ("this change", HERE, None), ("plain kernel", HERE, args.plain)]
        if args.change_first:
            order[0], order[1] = order[1], order[0]
        for who, root, lib in order:
            if root is None or (who == "plain kernel" and lib is None):
                continue
            rec = run_child(os.path.abspath(root), args.reps, lib)
            if "m" in rec and r == 0 and who == "this change":
                log(f"  the domain: m = {rec['m']} leave-one-out distances, threshold {rec['threshold']:.6g} (p = 0.05), rank 1")
            for name, v in rec["times"].items():
                pooled.setdefault((who, name), []).extend(v)
                log(f"  {who:12s} process {r + 1}  {name:12s} median {np.median(v):8.1f}   min {min(v):8.1f}   max {max(v):8.1f}")
            for law, ms in rec["kernel_ms"].items():
                kernel.setdefault((who, law), []).append(ms)
                small, full = rec["call_ms"][law]
                log(f"  {who:12s} process {r + 1}  {law}: codes and tallies of (b) equal the contract on float64 distances: "
                    f"{rec['equal'][law]} ({rec['codes'][law]} of 101 codes occur, share beyond {rec['share'][law]:.4f}; flow (c)'s "
                    f"float32 distances move {rec['moved32'][law]} codes); one-shot call {small:.3f} ms on 1 pixel, {full:.3f} ms on "
                    f"{N_TILES * TILE}: kernel {ms:.4f} ms per tile; record of that call {rec['record_tile'][law]}; of the stream "
                    f"{rec['record'][law]}")
    log("pooled over processes:")
    med = {}
    for (who, name), v in pooled.items():
        med[(who, name)] = float(np.median(v))
        log(f"  {who:12s} {name:12s} median {np.median(v):8.1f}   min {min(v):8.1f}   max {max(v):8.1f}   n = {len(v)}")
    new = "this change"
    for law in LAWS:
        log(f"{law}:")
        a = med[(new, f"{law}/a")]
        if ("parent", f"{law}/a") in med:
            pv = pooled[("parent", f"{law}/a")]
            log(f"  (a) parent {med[('parent', f'{law}/a')]:.1f} (its own spread {min(pv):.1f} .. {max(pv):.1f}), this change {a:.1f}")
        if (new, f"{law}/b") in med:
            b, c = med[(new, f"{law}/b")], med[(new, f"{law}/c")]
            log(f"  (b) - (a) = {b - a:+.1f}   (c) - (a) = {c - a:+.1f}")
            log(f"  domain kernel alone, LDS form: {np.median(kernel[(new, law)]):.4f} ms per tile")
        if ("plain kernel", f"{law}/b") in med:
            log(f"  (d) plain kernel: (b) {med[('plain kernel', f'{law}/b')]:.1f} against (a) {med[('plain kernel', f'{law}/a')]:.1f} "
                f"in the same processes: {med[('plain kernel', f'{law}/b')] - med[('plain kernel', f'{law}/a')]:+.1f}; "
                f"kernel alone {np.median(kernel[('plain kernel', law)]):.4f} ms per tile")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

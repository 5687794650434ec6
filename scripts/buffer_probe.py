"""Cost of buffered leave-out (``buffer=``) beside the leave-group-out call it extends.  A probe, not a test.

    python scripts/buffer_probe.py --parent DIR [--reps 5] [--rounds 2] [--bench-steps 30] [--out profiles/r22_spatial_buffer.txt]
    python scripts/buffer_probe.py --child --root DIR --reps N      # one process of the above: prints one JSON line

Workload: 50,000 x 32 reference rows (integers in [0, 4000), as the raster probes use), k = 5, the expanded formula;
groups of three consecutive rows; positions uniform in a 100 km square and a radius of 564 m, inside which five other
plots lie on average.

Flows, each a whole ``independent_kneighbors`` call on host arrays (codes and positions already on the handle, counts
cached: what a second call with the same masks costs), timed with ``perf_counter``; beside each, the scan launch alone between the device events
the library records around it (``last_kernel_ms``):
  groups        ``independent_kneighbors(groups)``                       parent commit and this change
  buffer        ``independent_kneighbors(buffer=...)``                   this change
  both          ``independent_kneighbors(groups, buffer=...)``           this change
  first buffer  the first buffered call of a process: upload of the positions, the count launch, then the scan
  counts        the handle's ``set_buffer`` with a radius not seen before, then ``buffer_counts()``: upload, the n x n
                count launch, the copy back of 50,000 int64
and the headline: ``python bench.py --gpus 1 --steps S --warmup 2`` in each checkout, its JSON line as printed.

``--parent`` names a checkout of the parent commit with its library built.  Processes alternate parent / this change,
``--rounds`` times; each runs ``--reps`` repetitions per flow after a warm-up call.  Medians, min and max in ms.  Every
child runs under a time limit of its own; the first that fails ends the probe.
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
N_REF, D, K, T = 50_000, 32, 5, 3
SIDE, RADIUS = 100_000.0, 564.0  # pi * 564^2 / 100000^2 * 50000 = 5.0 other rows inside the radius on average


def child(root, reps):
    sys.path.insert(0, root)
    import inspect

    import sknnr_amd

    rng = np.random.default_rng(0)
    x_ref = rng.integers(0, 4000, size=(N_REF, D)).astype(np.float64)
    est = sknnr_amd.RawKNNRegressor(n_neighbors=K, algorithm="brute").fit(x_ref, rng.standard_normal((N_REF, T)))
    groups = np.arange(N_REF) // 3
    coords = np.random.default_rng(1).uniform(0.0, SIDE, (N_REF, 2))
    has_buffer = "buffer" in inspect.signature(est.independent_kneighbors).parameters
    out = {"times": {}, "record": {}}

    def timed(run, n, scan=None):
        v = []
        for _ in range(n):
            t0 = time.perf_counter()
            run()
            v.append(1e3 * (time.perf_counter() - t0))
            if scan is not None:  # the scan launch alone, between the device events the library records around it
                scan.append(est.engine_._index.stats()["last_kernel_ms"])
        return v

    flows = {"groups": lambda: est.independent_kneighbors(groups)}
    if has_buffer:
        t0 = time.perf_counter()
        est.independent_kneighbors(buffer=(coords, RADIUS))
        out["times"]["first buffer"] = [1e3 * (time.perf_counter() - t0)]
        flows["buffer"] = lambda: est.independent_kneighbors(buffer=(coords, RADIUS))
        flows["both"] = lambda: est.independent_kneighbors(groups, buffer=(coords, RADIUS))
    for name, run in flows.items():
        run()  # (upload, first launch of the instantiation)
        scan = []
        out["times"][name] = timed(run, reps, scan)
        out["times"][name + ": scan kernel"] = scan
        out["record"][name] = est.engine_._index.debug_last_grouped()
        if has_buffer:
            out["record"][name + "/masks"] = est.engine_._index.debug_last_buffer()
    if has_buffer:
        ix = est.engine_._index
        radii = iter(RADIUS + 1.0 + np.arange(2 * reps + 2))

        def counts():
            ix.set_buffer(coords, float(next(radii)))
            counts.last = ix.buffer_counts()

        def upload():
            ix.set_buffer(coords, float(next(radii)))

        counts()
        out["times"]["counts"] = timed(counts, reps)
        out["times"]["counts: upload alone"] = timed(upload, reps)
        out["excluded"] = [int(counts.last.min()), float(counts.last.mean()), int(counts.last.max())]
    print(json.dumps(out), flush=True)


def run_child(root, reps):
    """One child process under a time limit of its own; returns its record, or raises with the end of its output."""
    proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--reps", str(reps)],
                          capture_output=True, text=True, timeout=600)
    if proc.returncode != 0:
        raise RuntimeError(f"child on {root} ended with {proc.returncode}: {proc.stderr[-2000:]}")
    return json.loads(proc.stdout.strip().splitlines()[-1])


def run_bench(root, steps):
    """The headline of a checkout: the last JSON line ``bench.py`` prints."""
    proc = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "2"], cwd=root,
                          capture_output=True, text=True, timeout=900)
    if proc.returncode != 0:
        raise RuntimeError(f"bench.py in {root} ended with {proc.returncode}: {proc.stderr[-2000:]}")
    return [ln for ln in proc.stdout.strip().splitlines() if ln.startswith("{")][-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--bench-steps", type=int, default=30, help="0: skip the headline")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r22_spatial_buffer.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default=HERE)
    args = ap.parse_args()
    if args.child:
        return child(os.path.abspath(args.root), args.reps)

    lines = []

    def log(msg=""):
        print(msg, flush=True)
        lines.append(msg)

    log(f"buffer probe: {N_REF} x {D} reference rows, k = {K}, expanded formula; groups of 3 rows; positions uniform in a "
        f"{SIDE / 1000:.0f} km square, radius {RADIUS:.0f} m; {args.reps} repetitions per flow and process, {args.rounds} processes "
        f"per build, alternating parent / this change; whole independent_kneighbors calls on host arrays, times in ms")
    pooled = {}
    for r in range(args.rounds):
        for who, root in (("parent", args.parent), ("this change", HERE)):
            if root is None:
                continue
            rec = run_child(os.path.abspath(root), args.reps)
            for name, v in rec["times"].items():
                pooled.setdefault((who, name), []).extend(v)
                log(f"  {who:12s} process {r + 1}  {name:24s} median {np.median(v):8.2f}   min {min(v):8.2f}   max {max(v):8.2f}")
            for name, record in rec["record"].items():
                log(f"  {who:12s} process {r + 1}  record of {name}: {record}")
            if "excluded" in rec:
                log(f"  {who:12s} process {r + 1}  excluded[] at the last radius: min {rec['excluded'][0]}, mean {rec['excluded'][1]:.2f}, "
                    f"max {rec['excluded'][2]}")
    log("pooled over processes:")
    med = {}
    for (who, name), v in pooled.items():
        med[(who, name)] = float(np.median(v))
        log(f"  {who:12s} {name:24s} median {np.median(v):8.2f}   min {min(v):8.2f}   max {max(v):8.2f}   n = {len(v)}")
    new = "this change"
    g = med[(new, "groups")]
    if ("parent", "groups") in med:
        pv = pooled[("parent", "groups")]
        where = "inside" if min(pv) <= g <= max(pv) else ("below (faster than)" if g < min(pv) else "ABOVE (slower than)")
        log(f"groups-only call: parent {med[('parent', 'groups')]:.2f} (its own spread {min(pv):.2f} .. {max(pv):.2f}), this change "
            f"{g:.2f}: {where} the parent's spread")
        spread = max(pv) - min(pv)
    else:
        spread = max(pooled[(new, "groups")]) - min(pooled[(new, "groups")])
    gk = med[(new, "groups: scan kernel")]
    for name in ("buffer", "both"):
        extra, extra_k = med[(new, name)] - g, med[(new, name + ": scan kernel")] - gk
        log(f"{name} - groups = {extra:+.2f} ms ({100.0 * extra / g:+.1f} %) for the call, {extra_k:+.3f} ms ({100.0 * extra_k / gk:+.1f} %) "
            f"for the scan kernel alone, against a spread of {spread:.2f} ms in the parent's groups-only call")
    log(f"buffer_counts after a new radius: {med[(new, 'counts')]:.2f} ms, of which the upload of the positions "
        f"{med[(new, 'counts: upload alone')]:.2f} ms")
    if args.bench_steps > 0:
        # (parent, this, this, parent: a drift of the device over the four runs does not favour one build)
        for who, root in (("parent", args.parent), ("this change", HERE), ("this change", HERE), ("parent", args.parent)):
            if root is not None:
                log(f"headline, {who}: {run_bench(os.path.abspath(root), args.bench_steps)}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

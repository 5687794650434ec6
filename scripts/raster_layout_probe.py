"""Cost of the raster layout on streamed tiles: band-first windows in, a band-first output raster out.  A probe, not a test.

    python scripts/raster_layout_probe.py [--reps 7] [--out profiles/r10_raster_layout.txt]
    python scripts/raster_layout_probe.py --kernel-only    # a few band-first tiles only: the child of the kernel trace

Workload: the benchmark's index (50,000 x 32 reference rows, k = 5) with three targets, ten windows of 1M pixels of 32
int16 bands, ``predict_chunks`` into a preallocated ``(targets, 10M)`` float64 output.  Three flows, interleaved,
``--reps`` repetitions each, medians and min-max:

  (a) today's flow: ``np.ascontiguousarray(np.moveaxis(win, 0, -1).reshape(-1, bands))`` per window on the host, the row
      stream, then a transposed store of the ``(n, targets)`` rows into the band-first output;
  (b) ``predict_chunks(windows, out=out, layout="bands")``: both transpositions on the device (planes.hip.h);
  (c) the floor: the row stream on rows transposed before the clock starts, results left row-major.

The two kernels' times come from one ``rocprofv3 --kernel-trace --stats`` run of ``--kernel-only`` (a child process under
its own time limit, the program directly after ``--``), the GB/s from the bytes each kernel must move.
"""

from __future__ import annotations

import argparse
import csv
import glob
import os
import shutil
import signal
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

N_REF, D, K, T, TILE, N_TILES = 50_000, 32, 5, 3, 1_000_000, 10
KERNEL_TILES = 4


def make_estimator():
    import sknnr_amd

    rng = np.random.default_rng(0)
    x_ref = rng.integers(0, 4000, size=(N_REF, D)).astype(np.float64)
    y = rng.standard_normal((N_REF, T))
    return sknnr_amd.RawKNNRegressor(n_neighbors=K, algorithm="brute").fit(x_ref, y)


def make_windows(n_tiles, seed=1):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 4000, size=(D, 1000, TILE // 1000), dtype=np.int16) for _ in range(n_tiles)]


def to_rows(win):
    return np.ascontiguousarray(np.moveaxis(win, 0, -1).reshape(-1, D))


def flow_a(est, windows, out):
    t_in = 0.0
    # (tile by tile as a user's loop does; one streamed call, so the pipeline stays full across the tiles)
    def tiles():
        nonlocal t_in
        for w in windows:
            t0 = time.perf_counter()
            r = to_rows(w)
            t_in += time.perf_counter() - t0
            yield r
    t0 = time.perf_counter()
    pred = est.predict_chunks(tiles())
    t_call = time.perf_counter() - t0 - t_in
    t0 = time.perf_counter()
    for a in range(0, pred.shape[0], TILE):
        out[:, a:a + TILE] = pred[a:a + TILE].T
    t_out = time.perf_counter() - t0
    return t_in, t_call, t_out


def flow_b(est, windows, out):
    est.predict_chunks(iter(windows), out=out, layout="bands")


def flow_c(est, rows, out_rows):
    est.predict_chunks(iter(rows), out=out_rows)


def kernel_only():
    est = make_estimator()
    windows = make_windows(KERNEL_TILES)
    out = np.empty((T, KERNEL_TILES * TILE))
    for _ in range(2):
        flow_b(est, windows, out)


def traced_kernels(log):
    """One rocprofv3 --kernel-trace --stats run of --kernel-only; returns {kernel: [(calls, average ns), ...]}."""
    prof = shutil.which("rocprofv3")
    if not prof:
        log("rocprofv3 not found: kernel times not recorded")
        return {}
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [prof, "--kernel-trace", "--stats", "-d", tmp, "-o", "planes", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--kernel-only"]
        # (no ramp-up in the child: every tile is a full window, so the averages are per 1M-pixel tile)
        # A session of its own, so that a time-out ends the profiler AND the python child that holds the GPU.
        proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True,
                                env=dict(os.environ, SKNNR_PIPE_NO_RAMP="1"))
        try:
            _, err = proc.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            os.killpg(proc.pid, signal.SIGKILL)
            proc.communicate()
            log("rocprofv3 run timed out after 240 s and was killed: kernel times not recorded")
            return {}
        if proc.returncode != 0:
            log(f"rocprofv3 run failed ({proc.returncode}): {err[-400:]}")
            return {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as fh:
                for row in csv.DictReader(fh):
                    name = row.get("Name", "")
                    for key in ("planes_to_rows_kernel", "rows_to_planes_kernel"):
                        if key in name:
                            out.setdefault(key, []).append((name, int(row["Calls"]), float(row["AverageNs"])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_raster_layout.txt"))
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    if args.kernel_only:
        return kernel_only()

    lines = []

    def log(msg=""):
        print(msg, flush=True)
        lines.append(msg)

    est = make_estimator()
    n = N_TILES * TILE
    log(f"raster layout probe: {N_REF} x {D} reference rows, k = {K}, {T} targets; {N_TILES} windows of {TILE} pixels x {D} int16 "
        f"bands; predict_chunks into a preallocated output; {args.reps} repetitions per flow, interleaved; times in ms")
    windows = make_windows(N_TILES)
    rows = [to_rows(w) for w in windows]
    out_a, out_b, out_c = np.zeros((T, n)), np.zeros((T, n)), np.zeros((n, T))
    flow_b(est, windows[:2], np.zeros((T, 2 * TILE)))  # (buffers, pinned memory, first launches)
    flow_c(est, rows[:2], out_c[:2 * TILE])
    ta, tb, tc, parts = [], [], [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        parts.append(flow_a(est, windows, out_a))
        ta.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        flow_b(est, windows, out_b)
        tb.append(time.perf_counter() - t0)
        rec = est.engine_._index.debug_last_planes()
        t0 = time.perf_counter()
        flow_c(est, rows, out_c)
        tc.append(time.perf_counter() - t0)
    same = np.array_equal(out_a, out_b) and np.array_equal(out_b, out_c.T)
    ms = lambda v: 1e3 * np.asarray(v)  # noqa: E731
    fmt = lambda v: f"median {np.median(ms(v)):8.1f}   min {ms(v).min():8.1f}   max {ms(v).max():8.1f}"  # noqa: E731
    p = np.median(ms(parts), axis=0)
    log(f"(a) host moveaxis + row stream + transposed store   {fmt(ta)}   (medians: moveaxis copies {p[0]:.1f}, stream {p[1]:.1f}, "
        f"transposed store {p[2]:.1f})")
    log(f"(b) layout='bands'                                  {fmt(tb)}")
    log(f"(c) floor: rows transposed beforehand, row results  {fmt(tc)}")
    med = {k_: float(np.median(ms(v))) for k_, v in (("a", ta), ("b", tb), ("c", tc))}
    spread_c = float(ms(tc).max() - ms(tc).min())
    log(f"results equal across the flows: {same}; last tile of (b): {rec}")
    log(f"(a) / (b) = {med['a'] / med['b']:.2f}x;  (b) - (c) = {med['b'] - med['c']:+.1f} ms against (c)'s min-max spread of "
        f"{spread_c:.1f} ms: {'inside' if med['b'] <= med['c'] + spread_c else 'OUTSIDE'} the floor's run-to-run noise")
    kern = traced_kernels(log)
    if kern:
        moved = {"planes_to_rows_kernel": 2 * TILE * D * 2, "rows_to_planes_kernel": 2 * TILE * T * 8}
        log(f"kernels (rocprofv3 --kernel-trace --stats; {2 * KERNEL_TILES} band-first tiles of {TILE} x {D} int16 in, {T} float64 "
            "planes out, no ramp-up):")
        for key, found in sorted(kern.items()):
            for name, calls, avg_ns in found:
                log(f"  {name[:60]:60s} calls {calls:3d}   average {avg_ns / 1e3:8.1f} us   {moved[key] / avg_ns:7.1f} GB/s "
                    f"({moved[key] / 1e6:.1f} MB moved)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

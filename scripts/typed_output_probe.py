"""Cost of the output side of streamed raster tiles: float64 predictions against int16 ones converted on the device.
A probe, not a test.

    python scripts/typed_output_probe.py [--reps 7] [--out profiles/r11_typed_outputs.txt]
    python scripts/typed_output_probe.py --kernel-only    # a few typed tiles only: the child of the kernel trace

Workload: the benchmark's index (50,000 x 32 reference rows, k = 5) with 25 targets, ten windows of 1M pixels of 32
int16 bands, ``predict_chunks`` into a preallocated output.  Three flows for each layout (rows, bands), interleaved,
``--reps`` repetitions each, medians and min-max:

  (a) today's flow: float64 out, then the host's ``rint`` / ``clip`` / ``astype(int16)`` pass, window by window;
  (b) float64 out alone;
  (c) ``out_dtype=np.int16``: the conversion on the device (narrow.hip.h), int16 out.

The conversion kernels' times come from one ``rocprofv3 --kernel-trace --stats`` run of ``--kernel-only`` (a child process
under its own time limit, the program directly after ``--``), the GB/s from the bytes each kernel must move.
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

N_REF, D, K, T, TILE, N_TILES = 50_000, 32, 5, 25, 1_000_000, 10
KERNEL_TILES = 4
SCALE, OFFSET = 1000.0, 0.0  # targets ~ N(0, 1): stored in thousandths


def make_estimator():
    import sknnr_amd

    rng = np.random.default_rng(0)
    x_ref = rng.integers(0, 4000, size=(N_REF, D)).astype(np.float64)
    y = rng.standard_normal((N_REF, T))
    return sknnr_amd.RawKNNRegressor(n_neighbors=K, algorithm="brute").fit(x_ref, y)


def make_windows(n_tiles, seed=1):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 4000, size=(D, TILE), dtype=np.int16) for _ in range(n_tiles)]


def host_pass(src, dst, bands):
    """What a user runs today over the float64 result, window by window."""
    t0 = time.perf_counter()
    for a in range(0, N_TILES * TILE, TILE):
        s = src[:, a:a + TILE] if bands else src[a:a + TILE]
        d = dst[:, a:a + TILE] if bands else dst[a:a + TILE]
        d[...] = np.clip(np.rint(s * SCALE + OFFSET), -32768, 32767).astype(np.int16)
    return time.perf_counter() - t0


def stream(est, tiles, out, bands, typed):
    kw = dict(out_dtype=np.int16, scale=SCALE, offset=OFFSET) if typed else {}
    est.predict_chunks(iter(tiles), out=out, layout="bands" if bands else "rows", **kw)


def kernel_only():
    est = make_estimator()
    windows = make_windows(KERNEL_TILES)
    rows = [np.ascontiguousarray(w.T) for w in windows]
    for _ in range(2):
        stream(est, rows, np.empty((KERNEL_TILES * TILE, T), dtype=np.int16), False, True)
        stream(est, windows, np.empty((T, KERNEL_TILES * TILE), dtype=np.int16), True, True)


def traced_kernels(log):
    """One rocprofv3 --kernel-trace --stats run of --kernel-only; returns [(kernel, calls, average ns), ...]."""
    prof = shutil.which("rocprofv3")
    if not prof:
        log("rocprofv3 not found: kernel times not recorded")
        return []
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [prof, "--kernel-trace", "--stats", "-d", tmp, "-o", "narrow", "--output-format", "csv", "--",
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
            return []
        if proc.returncode != 0:
            log(f"rocprofv3 run failed ({proc.returncode}): {err[-400:]}")
            return []
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as fh:
                for row in csv.DictReader(fh):
                    name = row.get("Name", "")
                    if "narrow_" in name or "rows_to_planes_kernel" in name:
                        out.append((name, int(row["Calls"]), float(row["AverageNs"])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_typed_outputs.txt"))
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
    log(f"typed output probe: {N_REF} x {D} reference rows, k = {K}, {T} targets; {N_TILES} windows of {TILE} pixels x {D} int16 "
        f"bands; predict_chunks into a preallocated output; {args.reps} repetitions per flow, interleaved; times in ms")
    log(f"bytes per window: {TILE * D * 2 / 1e6:.0f} MB in, {TILE * T * 8 / 1e6:.0f} MB out as float64, {TILE * T * 2 / 1e6:.0f} MB out as int16")
    windows = make_windows(N_TILES)
    rows = [np.ascontiguousarray(w.T) for w in windows]
    ms = lambda v: 1e3 * np.asarray(v)  # noqa: E731
    fmt = lambda v: f"median {np.median(ms(v)):8.1f}   min {ms(v).min():8.1f}   max {ms(v).max():8.1f}"  # noqa: E731
    for bands in (False, True):
        tiles = windows if bands else rows
        shape = (T, n) if bands else (n, T)
        out64, out16, host16 = np.zeros(shape), np.zeros(shape, dtype=np.int16), np.zeros(shape, dtype=np.int16)
        small = (T, 2 * TILE) if bands else (2 * TILE, T)
        stream(est, tiles[:2], np.zeros(small), bands, False)  # (buffers, pinned memory, first launches)
        stream(est, tiles[:2], np.zeros(small, dtype=np.int16), bands, True)
        ta, tb, tc, t_host = [], [], [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            stream(est, tiles, out64, bands, False)
            t_host.append(host_pass(out64, host16, bands))
            ta.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            stream(est, tiles, out64, bands, False)
            tb.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            stream(est, tiles, out16, bands, True)
            tc.append(time.perf_counter() - t0)
            rec = est.engine_._index.debug_last_narrow()
        same = np.array_equal(out16, host16)
        log(f"layout = {'bands' if bands else 'rows'}")
        log(f"  (a) float64 out + host rint / clip / astype   {fmt(ta)}   (median of the host pass alone {np.median(ms(t_host)):.1f})")
        log(f"  (b) float64 out alone                         {fmt(tb)}")
        log(f"  (c) int16 out, converted on the device        {fmt(tc)}")
        med = {k_: float(np.median(ms(v))) for k_, v in (("a", ta), ("b", tb), ("c", tc))}
        spread_b = float(ms(tb).max() - ms(tb).min())
        log(f"  device result equals the host pass: {same}; last tile of (c): {rec}")
        log(f"  (a) / (c) = {med['a'] / med['c']:.2f}x;  (c) - (b) = {med['c'] - med['b']:+.1f} ms against (b)'s min-max spread of "
            f"{spread_b:.1f} ms: expectation (c) <= (b) + spread {'MET' if med['c'] <= med['b'] + spread_b else 'MISSED'}")
        del out64, out16, host16
    kern = traced_kernels(log)
    if kern:
        moved = TILE * T * (8 + 2)
        log(f"kernels (rocprofv3 --kernel-trace --stats; {2 * KERNEL_TILES} row tiles and {2 * KERNEL_TILES} band-first tiles of "
            f"{TILE} x {T} float64 -> int16, no ramp-up; {moved / 1e6:.0f} MB moved per tile):")
        for name, calls, avg_ns in sorted(kern):
            log(f"  {name[:90]:90s} calls {calls:3d}   average {avg_ns / 1e3:8.1f} us   {moved / avg_ns:7.1f} GB/s")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

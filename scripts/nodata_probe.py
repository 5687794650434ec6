"""Cost of nodata handling on streamed raster tiles: the host flow a user of the unmasked call needs (compare and
``X[valid]`` on the host, ``kneighbors_chunks``, scatter of the answers on the host) against ``kneighbors_chunks(...,
nodata=)``, which masks, compacts and expands on the device (sknnr_amd/csrc/mask.hip.h).  A probe, not a test.

    python scripts/nodata_probe.py [--rows 10000000] [--out profiles/r09_nodata.txt]
    python scripts/nodata_probe.py --kernel-only      # device-resident masked calls only: the child of the kernel trace

Workload: 50,000 x 32 reference rows, a stream of int16 tiles of 1M x 32 rows, k = 5, nodata -32768; masked fractions 0 %,
30 % in contiguous blobs, 100 %.  Every flow is timed end to end (host tiles in, full-layout host arrays out), best of
``--reps``.  The three kernels' times come from one ``rocprofv3 --kernel-trace --stats`` run of ``--kernel-only`` (a child
process under its own time limit), the GB/s from the bytes each kernel must move.
"""

from __future__ import annotations

import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

N_REF, D, K, TILE = 50_000, 32, 5, 1_000_000
NODATA = -32768
KERNEL_ROWS, KERNEL_REPS = 1_000_000, 5


def blob_mask(nq, fraction, seed=0, mean_len=20_000):
    rng = np.random.default_rng(seed)
    m = np.zeros(nq, dtype=bool)
    if fraction >= 1.0:
        m[:] = True
    target = int(fraction * nq)
    while m.sum() < target:
        a = int(rng.integers(0, nq))
        m[a:a + int(rng.integers(1, 2 * mean_len))] = True
    return m


def make_estimator():
    import sknnr_amd

    rng = np.random.default_rng(0)
    x_ref = rng.integers(0, 4000, size=(N_REF, D)).astype(np.float64)
    y = rng.standard_normal((N_REF, 2))
    return sknnr_amd.RawKNNRegressor(n_neighbors=K, algorithm="brute").fit(x_ref, y)


def make_rows(n, fraction, seed=1):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 4000, size=(n, D), dtype=np.int16)
    masked = blob_mask(n, fraction, seed)
    rows = np.flatnonzero(masked)
    x[rows, rng.integers(0, D, size=rows.size)] = NODATA
    return x, masked


def tiles_of(x):
    return (x[a:a + TILE] for a in range(0, x.shape[0], TILE))


def best_of(fn, reps):
    best, out = None, None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, out


def host_flow(est, x):
    """What the unmasked call asks of its user: compare and compact on the host, call, scatter on the host."""
    t0 = time.perf_counter()
    valid = (x != NODATA).all(axis=1)
    xv = x[valid]
    t1 = time.perf_counter()
    if xv.shape[0]:
        dist_v, idx_v = est.kneighbors_chunks(tiles_of(xv))
    t2 = time.perf_counter()
    idx = np.full((x.shape[0], K), -1, dtype=np.int64)
    dist = np.full((x.shape[0], K), np.nan)
    if xv.shape[0]:
        idx[valid] = idx_v
        dist[valid] = dist_v
    t3 = time.perf_counter()
    return dist, idx, (t1 - t0, t2 - t1, t3 - t2)


def kernel_only():
    """Masked device-memory calls on a resident 1M x 32 int16 tile, 30 % masked in blobs (the traced child)."""
    import torch

    est = make_estimator()
    eng = est.engine_
    x, _ = make_rows(KERNEL_ROWS, 0.3)
    xt = torch.as_tensor(x, device="cuda")
    nodata = np.full(D, float(NODATA))
    for _ in range(KERNEL_REPS):
        eng.kneighbors(xt, K, formula=est._formula(), nodata=nodata)
    torch.cuda.synchronize()


def traced_kernels(log):
    """One rocprofv3 --kernel-trace --stats run of --kernel-only; returns {kernel: (calls, average ns)}."""
    prof = shutil.which("rocprofv3")
    if not prof:
        log("rocprofv3 not found: kernel times not recorded")
        return {}
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [prof, "--kernel-trace", "--stats", "-d", tmp, "-o", "nodata", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--kernel-only"]
        proc = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
        if proc.returncode != 0:
            log(f"rocprofv3 run failed ({proc.returncode}): {proc.stderr[-400:]}")
            return {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as fh:
                for row in csv.DictReader(fh):
                    name = row.get("Name", "")
                    for key in ("row_mask_kernel", "mask_scan_kernel", "row_compact_kernel", "row_expand_kernel"):
                        if key in name:
                            out[key] = (int(row["Calls"]), float(row["AverageNs"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_nodata.txt"))
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    if args.kernel_only:
        return kernel_only()

    lines = []

    def log(msg=""):
        print(msg, flush=True)
        lines.append(msg)

    est = make_estimator()
    n = args.rows
    log(f"nodata probe: {N_REF} x {D} reference rows, {n} x {D} int16 rows in tiles of {TILE}, k = {K}, nodata {NODATA}; "
        f"host arrays in, full-layout host arrays out; best of {args.reps}; times in ms")
    warm, _ = make_rows(TILE, 0.3, seed=9)
    est.kneighbors_chunks(tiles_of(warm), nodata=NODATA)  # (buffers, pinned memory, first launches)
    est.kneighbors_chunks(tiles_of(warm))
    for fraction in (0.0, 0.3, 1.0):
        x, masked = make_rows(n, fraction)
        t_new, (dist, idx) = best_of(lambda: est.kneighbors_chunks(tiles_of(x), nodata=NODATA), args.reps)
        rec = est.engine_._index.debug_last_mask()
        t_host, (dist_h, idx_h, parts) = best_of(lambda: host_flow(est, x), args.reps)
        same = np.array_equal(idx, idx_h) and np.array_equal(dist, dist_h, equal_nan=True)
        log(f"masked {100 * masked.mean():5.1f} %: device mask {1e3 * t_new:8.1f}   host flow {1e3 * t_host:8.1f} "
            f"(compare + X[valid] {1e3 * parts[0]:.1f}, kneighbors_chunks {1e3 * parts[1]:.1f}, scatter {1e3 * parts[2]:.1f})   "
            f"speed-up {t_host / t_new:5.2f}x   results equal: {same}   last tile path {rec['path']}")
        if fraction == 0.0:
            t_plain, _ = best_of(lambda: est.kneighbors_chunks(tiles_of(x)), args.reps)
            log(f"fully valid stream: unmasked call {1e3 * t_plain:8.1f}, with nodata= {1e3 * t_new:8.1f}: "
                f"the mask costs {1e3 * (t_new - t_plain):+.1f} ms ({100 * (t_new / t_plain - 1):+.1f} %) over {n // TILE} tiles "
                f"(mask kernel + scan + one 8-byte read per tile; no compaction, no expansion: path {rec['path']})")
        del x, dist, idx, dist_h, idx_h
    kern = traced_kernels(log)
    if kern:
        x, masked = make_rows(KERNEL_ROWS, 0.3)
        nq, nv, rb = KERNEL_ROWS, int((~masked).sum()), 2 * D
        moved = {"row_mask_kernel": nq * rb + nq, "mask_scan_kernel": 8 * ((nq + 255) // 256),
                 "row_compact_kernel": nq + 2 * nv * rb + 4 * nq, "row_expand_kernel": 5 * nq + 16 * K * (nv + nq)}
        log(f"kernels (rocprofv3 --kernel-trace --stats; device-resident {nq} x {D} int16 tile, {nq - nv} rows masked in blobs):")
        for name, (calls, avg_ns) in sorted(kern.items()):
            log(f"  {name:20s} calls {calls:3d}   average {avg_ns / 1e3:9.1f} us   {moved[name] / avg_ns:8.1f} GB/s "
                f"({moved[name] / 1e6:.1f} MB moved)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

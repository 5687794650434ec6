"""End-to-end rows/s of RFNNRegressor / GBNNRegressor.predict on raw query rows: the device forest map against the host
path it replaces (scikit-learn's apply on the host, float64 node ids to the device), Moscow-shaped forests.

    python scripts/forest_map_probe.py [n_rows] [host_rows]          # the comparison, one JSON line per estimator
    python scripts/forest_map_probe.py --kernel-only [n_rows]       # forest_apply alone (run under rocprofv3 --kernel-trace --stats)

Query rows are Moscow rows with 1 % noise, float32, resident on the host.  The host path is timed on ``host_rows`` rows and
reported per row, with the forests' own default (n_jobs=None: one thread) and with n_jobs=16.  ``visits`` counts the
nodes read per row (leaf depth + 1, summed over the trees, on the rows actually queried), for a node-visit rate.
"""

from __future__ import annotations

import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import sknnr_amd  # noqa: E402
from sknnr_amd.datasets import load_moscow_stjoes  # noqa: E402


def make_rows(X, n, seed=0):
    rng = np.random.default_rng(seed)
    base = X[rng.integers(0, len(X), n)]
    return (base * (1.0 + 0.01 * rng.standard_normal(base.shape))).astype(np.float32)


def node_depths(image):
    off = image["tree_offset"]
    depth = np.zeros(off[-1], dtype=np.int64)
    for t in range(off.size - 1):
        a = off[t]
        for i in range(off[t + 1] - a):
            lc = image["left"][a + i]
            if lc != -1:
                depth[a + lc] = depth[a + i] + 1
                depth[a + image["right"][a + i]] = depth[a + i] + 1
    return depth


def fit(cls):
    X, y = load_moscow_stjoes(return_X_y=True)
    return cls(random_state=42).fit(X, y), X


def best_of(fn, reps=3):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return min(times)


def compare(n_rows, host_rows):
    for name, cls in (("RFNN", sknnr_amd.RFNNRegressor), ("GBNN", sknnr_amd.GBNNRegressor)):
        est, X = fit(cls)
        q = make_rows(X, n_rows)
        est.predict(q[:1000])  # warm-up (library, workspace)
        t_dev = best_of(lambda: est.predict(q))
        image = est.transformer_.forest_image()
        depth = node_depths(image)
        ids = est.regressor_.engine_.forest_apply(q[:20000]).astype(np.int64)
        visits = float((depth[image["tree_offset"][:-1][None, :] + ids] + 1).sum(axis=1).mean())
        qh = q[:host_rows]
        host = {}
        for jobs in (None, 16):
            for f in est.transformer_.estimators_:
                f.n_jobs = jobs
            t = best_of(lambda: est.regressor_.predict(np.ascontiguousarray(est.transformer_.transform(qh), dtype=np.float64)), 1)
            host[str(jobs)] = host_rows / t
        np.testing.assert_array_equal(est.predict(qh), est.regressor_.predict(est.transformer_.transform(qh).astype(np.float64)))
        print(json.dumps({"estimator": name, "trees": int(est.regressor_.engine_.d), "rows": n_rows, "d_in": int(X.shape[1]),
                          "device_rows_per_s": n_rows / t_dev, "device_s": t_dev,
                          "host_rows_per_s_n_jobs_none": host["None"], "host_rows_per_s_n_jobs_16": host["16"],
                          "speedup_vs_n_jobs_none": n_rows / t_dev / host["None"],
                          "speedup_vs_n_jobs_16": n_rows / t_dev / host["16"],
                          "mean_node_visits_per_row": visits, "max_tree_depth": int(depth.max())}), flush=True)


def kernel_only(n_rows):
    import torch

    for cls in (sknnr_amd.RFNNRegressor, sknnr_amd.GBNNRegressor):
        est, X = fit(cls)
        qd = torch.as_tensor(make_rows(X, n_rows)).cuda()
        eng = est.regressor_.engine_
        for _ in range(3):
            eng.forest_apply(qd)
        torch.cuda.synchronize()
        print(cls.__name__, "forest_apply x3 on", n_rows, "rows,", eng.d, "trees", flush=True)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--kernel-only" in sys.argv:
        kernel_only(int(args[0]) if args else 1 << 18)
    else:
        compare(int(args[0]) if args else 1_000_000, int(args[1]) if len(args) > 1 else 20000)

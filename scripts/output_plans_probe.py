"""Output plans: one ``predict_chunks(outputs=...)`` call with four planes of one target against four
``predict_chunks(statistic=...)`` calls and one plain ``predict_chunks`` -- wall times of 7 interleaved repetitions after two
warm-up runs each (medians, min, max), one JSON line.  1M query rows in eight tiles, 50,000 reference rows, 32 features,
k = 5, t = 3.  ``python scripts/output_plans_probe.py`` from the repository root; profiles/r17_output_plans.txt holds a run."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import json
import statistics
import time

import numpy as np
import torch

import sknnr_amd

rng = np.random.default_rng(0)
ref = rng.standard_normal((50_000, 32))
y = np.stack([rng.standard_normal(50_000) * 50 + 100, rng.integers(0, 5, 50_000) * 40.0 + 3, rng.random(50_000) * 200], axis=1)
X = rng.standard_normal((1_000_000, 32))
tiles = [X[i:i + 125_000] for i in range(0, len(X), 125_000)]
est = sknnr_amd.RawKNNRegressor(n_neighbors=5, algorithm="brute").fit(ref, y)
PLAN = [(0, "mean"), (0, "std"), (0, ("quantile", .1)), (0, ("quantile", .9))]
out4 = np.empty((len(X), 4))
out3 = np.empty((len(X), 3))


def plan():
    est.predict_chunks(iter(tiles), out=out4, outputs=PLAN)


def four():
    for s in ("mean", "std", "min", "max"):
        est.predict_chunks(iter(tiles), out=out3, statistic=s)


def plain():
    est.predict_chunks(iter(tiles), out=out3)


runs = {"plan": plan, "four": four, "plain": plain}
for f in runs.values():
    f()
    f()
times = {k: [] for k in runs}
for rep in range(7):
    for name, f in runs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        times[name].append((time.perf_counter() - t0) * 1e3)
res = {k: dict(median_ms=round(statistics.median(v), 2), min_ms=round(min(v), 2), max_ms=round(max(v), 2)) for k, v in times.items()}
res["device"] = torch.cuda.get_device_name(0)
print(json.dumps(res))

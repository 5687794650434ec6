"""Readers of the tree-tie fixtures (tests/golden/tree_*.npz, written by make_golden.py's ``make_tree_ties``): the
reference's kd_tree / ball_tree answers on integer lattices, where exact ties at the k-th distance are the rule, and
its explicit ball_tree on continuous data.  Shared by test_tree_ties_oracle.py (CPU) and test_tree_ties_gpu.py."""

from __future__ import annotations

import numpy as np

from conftest import load_golden

LATTICE = ["d6", "d8_dup", "leaf5", "ball"]  # every tie-heavy reference case (kd_tree, kd_tree, kd_tree leaf 5, ball_tree)
CONTINUOUS = [8, 32]  # explicit ball_tree on sknnr_amd.synth data


def lattice_case(name):
    """fit rows, targets, query rows, fit method, leaf size and the stored neighbours of one lattice case."""
    g = load_golden(f"tree_ties_{name}.npz")
    src = load_golden(f"tree_ties_{str(g['source'])}.npz") if "source" in g else g
    nq = int(g["n_queries"]) if "n_queries" in g else src["X"].shape[0]
    return {"fit_X": src["fit_X"], "X": src["X"][:nq], "y": src["y"], "fit_method": str(g["fit_method"]),
            "leaf_size": int(g["leaf_size"]), "g": g, "ks": (1, 5) if "tgt_k1_nn" in g else (5,)}


def continuous_case(d):
    from sknnr_amd import synth

    g = load_golden(f"tree_ball_continuous_d{d}.npz")
    x_ref, y, x_q = synth.make_problem(1000, 500, d, t=3, n_dup_queries=20)
    return {"fit_X": x_ref, "X": x_q, "y": y, "fit_method": str(g["fit_method"]), "leaf_size": 30, "g": g, "ks": (5,)}


def expected(g, q, k, deterministic):
    """The reference's ``(dist, idx)`` for ``q`` = "tgt" (X given) or "ref" (X=None): lattice distances are stored as the
    integer d2 they are the square root of, the tree's own order (no deterministic reorder) as a permutation of the
    deterministic columns."""
    key = f"{q}_k1" if k == 1 else f"{q}_k{k}_det"
    idx = g[key + "_nn"].astype(np.int64)
    dist = np.sqrt(g[key + "_d2"].astype(np.float64)) if key + "_d2" in g else g[key + "_dist"]
    if k > 1 and not deterministic:
        perm = g[f"{q}_k{k}_nd_perm"].astype(np.int64)
        idx, dist = np.take_along_axis(idx, perm, 1), np.take_along_axis(dist, perm, 1)
    return dist, idx


def tie_rows(d2_probe, kk, deterministic):
    """Rows whose answer depends on the choice among exactly tied rows, from a search for ``kk + 1`` neighbours
    ordered by (d2, index): a tie across the last kept slot, or -- without the deterministic reorder, which fixes the
    order of the kept rows -- anywhere among them."""
    if deterministic:
        return d2_probe[:, kk - 1] == d2_probe[:, kk]
    return (d2_probe[:, :-1] == d2_probe[:, 1:]).any(axis=1)


def modes(case):
    for q in ("tgt", "ref"):
        for k in case["ks"]:
            for det in ((True,) if k == 1 else (True, False)):
                yield q, k, det

"""The forest image RFNN / GBNN hand to the device (TreeNodeTransformer.forest_image) and the host structure check that
guards it (check_forest_image), without a GPU: a small numpy walk over the image reproduces scikit-learn's apply."""

from __future__ import annotations

import numpy as np
import pytest
from sklearn.ensemble import (GradientBoostingClassifier, GradientBoostingRegressor, RandomForestClassifier,
                              RandomForestRegressor)

from sknnr_amd.transformers import GBNodeTransformer, RFNodeTransformer
from sknnr_amd.transformers._tree_nodes import check_forest_image


def walk(image, X):
    """Node ids (n, n_trees) of the rows X through the image: x as float32, x <= threshold goes left."""
    X32 = np.asarray(X, dtype=np.float32).astype(np.float64)
    off, thr, feat, left, right = (image[k] for k in ("tree_offset", "threshold", "feature", "left", "right"))
    out = np.zeros((X32.shape[0], off.size - 1), dtype=np.int64)
    for t in range(off.size - 1):
        a = off[t]
        node = np.zeros(X32.shape[0], dtype=np.int64)
        while True:
            inner = left[a + node] != -1
            if not inner.any():
                break
            g = a + node[inner]
            go_left = X32[np.flatnonzero(inner), feat[g]] <= thr[g]
            node[inner] = np.where(go_left, left[g], right[g])
        out[:, t] = node
    return out


def _data(n=300, d=6, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d))
    y_num = X[:, 0] * 2 + rng.normal(size=n)
    return X, y_num, rng


def _forests():
    X, y_num, rng = _data()
    y_str = np.where(X[:, 1] > 0, "up", "down")
    y3 = np.array(["a", "b", "c"])[rng.integers(0, 3, len(X))]
    return X, [
        ("rf_regressor", RFNodeTransformer(n_estimators=7, random_state=0), np.c_[y_num]),
        ("rf_mixed", RFNodeTransformer(n_estimators=5, random_state=1), np.c_[y_num, y_str].astype(object)),
        ("gb_regressor", GBNodeTransformer(n_estimators=9, random_state=0), y_num),
        ("gb_binary", GBNodeTransformer(n_estimators=6, random_state=0), y_str),
        ("gb_3class", GBNodeTransformer(n_estimators=5, random_state=0), y3),
        ("gb_early_stop", GBNodeTransformer(n_estimators=400, n_iter_no_change=2, validation_fraction=0.3,
                                            random_state=0), y_num),
    ]


@pytest.mark.parametrize("case", range(6))
def test_forest_image_walk_equals_apply(case):
    X, forests = _forests()
    name, transformer, y = forests[case]
    transformer.fit(X, y)
    image = transformer.forest_image()
    Xq = np.random.default_rng(5).normal(size=(200, X.shape[1]))
    np.testing.assert_array_equal(walk(image, Xq), transformer.transform(Xq))
    assert image["d_in"] == X.shape[1]
    assert image["tree_offset"].size - 1 == transformer.transform(Xq[:1]).shape[1]
    depths = check_forest_image(image)
    trees = [t for f in transformer.estimators_ for t in np.asarray(f.estimators_).T.reshape(-1)] \
        if name.startswith("gb") else [t for f in transformer.estimators_ for t in f.estimators_]
    np.testing.assert_array_equal(depths, [t.tree_.max_depth for t in trees])
    if name == "gb_early_stop":
        forest = transformer.estimators_[0]
        assert forest.n_estimators_ < forest.n_estimators
        assert image["tree_offset"].size - 1 == forest.n_estimators_


def test_forest_image_is_class_major_for_multiclass_boosting():
    X, y_num, rng = _data(seed=3)
    y3 = np.array(["a", "b", "c"])[rng.integers(0, 3, len(X))]
    t = GBNodeTransformer(n_estimators=4, random_state=0).fit(X, y3)
    forest = t.estimators_[0]
    image = t.forest_image()
    # column j * stages + s is the tree of class j at stage s
    for j in range(3):
        for s in range(4):
            col = j * 4 + s
            a, b = image["tree_offset"][col], image["tree_offset"][col + 1]
            np.testing.assert_array_equal(image["threshold"][a:b], forest.estimators_[s, j].tree_.threshold)


def test_forest_image_of_plain_scikit_learn_ensembles():
    """Every ensemble kind the transformers grow, including classifiers on string targets."""
    X, y_num, _ = _data(seed=7)
    for est, y in ((RandomForestRegressor(n_estimators=3, random_state=0), y_num),
                   (RandomForestClassifier(n_estimators=3, random_state=0), np.where(y_num > 0, "p", "n")),
                   (GradientBoostingRegressor(n_estimators=3, random_state=0), y_num),
                   (GradientBoostingClassifier(n_estimators=3, random_state=0), np.where(y_num > 0, "p", "n"))):
        t = RFNodeTransformer(n_estimators=3)
        t.estimators_ = [est.fit(X, y)]
        t.n_features_in_ = X.shape[1]
        ids = est.apply(X)
        if ids.ndim == 3:
            ids = ids.transpose(0, 2, 1).reshape(len(X), -1)
        np.testing.assert_array_equal(walk(t.forest_image(), X), ids)


def _small_image():
    X, y_num, _ = _data(n=80, d=3, seed=11)
    t = RFNodeTransformer(n_estimators=2, random_state=0).fit(X, y_num)
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in t.forest_image().items()}


def test_structure_check_rejects_malformed_images():
    image = _small_image()
    check_forest_image(image)
    inner = np.flatnonzero(image["left"] != -1)
    assert inner.size > 2

    cyc = _small_image()  # a child that points back at the root: a cycle
    cyc["right"][inner[1]] = 0
    with pytest.raises(ValueError, match="child"):
        check_forest_image(cyc)

    out = _small_image()  # a child beyond the tree's last node
    a, b = out["tree_offset"][0], out["tree_offset"][1]
    out["left"][inner[0]] = b - a
    with pytest.raises(ValueError, match="child"):
        check_forest_image(out)

    feat = _small_image()
    feat["feature"][inner[0]] = feat["d_in"]
    with pytest.raises(ValueError, match="feature"):
        check_forest_image(feat)

    nan = _small_image()
    nan["threshold"][inner[0]] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        check_forest_image(nan)

    empty = _small_image()
    empty["tree_offset"] = np.array([0, 0, empty["tree_offset"][-1]])
    with pytest.raises(ValueError, match="tree_offset"):
        check_forest_image(empty)

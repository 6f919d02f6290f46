#!/usr/bin/env python3
"""Records scikit-learn's answers for two scenes of tests/geo_oracle.py into tests/golden/geo_sklearn.npz, so that the restatement
stays pinned where scikit-learn is not installed: DBSCAN(eps, 100).labels_ at every eps the scene runs (int16), PCA(2)'s yaw, and
the head of sklearn.utils.shuffle(arange(n), random_state=42).

    python tests/golden/make_geo_golden.py        (needs scikit-learn)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import geo_oracle as G  # noqa: E402

SCENES = ("trial2", "small")


def main():
    import sklearn
    from sklearn.cluster import DBSCAN
    from sklearn.decomposition import PCA
    from sklearn.utils import shuffle
    out = {"sklearn_version": np.array(sklearn.__version__)}
    for name in SCENES:
        depth, mask, K = G.make_scene(**G.SCENES[name])
        r = G.lift_points(depth, mask, K)
        P = G.unproject(depth, mask, K)
        v = PCA(2).fit((P - P.mean(0))[:, [0, 2]]).components_[0]
        out[f"{name}_yaw"] = np.array(np.arctan2(v[1], v[0]))
        eps = 0.01
        for t in range(1, (r["trial"] or 4) + 1):
            lab = DBSCAN(eps=eps, min_samples=100).fit(r["T"]).labels_
            assert lab.max() < 2 ** 15
            out[f"{name}_labels{t}"] = lab.astype(np.int16)
            eps = 2 * eps
        n = r["n_points"]
        out[f"{name}_perm_head"] = shuffle(np.arange(n), random_state=42)[:256].astype(np.int32)
    path = os.path.join(HERE, "geo_sklearn.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

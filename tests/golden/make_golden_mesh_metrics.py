"""Generate g27_mesh_metrics.npz from the REAL reference (build container only).

    python tests/golden/make_golden_mesh_metrics.py

The point-cloud metrics of neural_graph_mapping.evaluation (evaluation.py:65-130: scipy.spatial.KDTree build + query,
np.median / np.mean, ratios below 5 cm and 1 cm, F1), called one by one exactly as _evaluate_postprocessed_meshes calls them
(evaluation.py:197-208), on two pairs of small clouds.  The mocked trimesh cannot sample, so the clouds are made here: points
on the walls of a box (a room), the estimate a subset of the ground truth plus noise of a few centimetres, so that all four
ratios land strictly between 0 and 1.  Pair 0: 4001 ground-truth / 3000 estimated points, pair 1: 800 / 1001 -- odd and
even counts on either side, so both branches of the median run.  Stored: the clouds (float32; the reference is given exactly
these values), its ten numbers per pair and the per-point KDTree distances.  Data only.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from _ref_import import import_reference  # noqa: E402
import _mesh_metrics_host as MH  # noqa: E402

import_reference()
from neural_graph_mapping import evaluation as ev  # noqa: E402
from scipy import spatial  # noqa: E402

SEED = 27
PAIRS = ((4001, 3000, 0.02), (800, 1001, 0.015))        # ground-truth points, estimated points, noise sigma [m]
BAR = 2.0 ** -21                                          # the GPU test's relative bar on a distance


def box_surface(rng, n, size):
    """n points on the six walls of a box of the given size, uniform by area"""
    sx, sy, sz = size
    areas = np.array([sy * sz, sy * sz, sx * sz, sx * sz, sx * sy, sx * sy])
    wall = rng.choice(6, n, p=areas / areas.sum())
    p = rng.uniform(0, 1, (n, 3)) * size
    axis, side = wall // 2, wall % 2
    p[np.arange(n), axis] = side * np.asarray(size)[axis]
    return p


def pair(rng, n_gt, n_est, sigma):
    size = (1.6, 1.2, 0.9)
    gt = box_surface(rng, n_gt, size)
    src = gt[rng.choice(n_gt, n_est, replace=n_est > n_gt)]
    est = src + rng.normal(0, sigma, (n_est, 3))
    return gt.astype(np.float32), est.astype(np.float32)


def main():
    rng = np.random.default_rng(SEED)
    out = {}
    for i, (n_gt, n_est, sigma) in enumerate(PAIRS):
        gt32, est32 = pair(rng, n_gt, n_est, sigma)
        gt, est = gt32.astype(np.float64), est32.astype(np.float64)
        ref = {"median_acc": ev.median_accuracy(gt, est), "median_comp": ev.median_completion(gt, est),
               "acc": ev.mean_accuracy(gt, est), "comp": ev.mean_completion(gt, est),
               "acc_ratio": ev.accuracy_ratio(gt, est, 0.05, rerun_vis=False), "acc_ratio_1cm": ev.accuracy_ratio(gt, est, 0.01),
               "comp_ratio": ev.completion_ratio(gt, est, 0.05, rerun_vis=False),
               "comp_ratio_1cm": ev.completion_ratio(gt, est, 0.01),
               "f1_5cm": ev.reconstruction_f1(gt, est, 0.05), "f1_1cm": ev.reconstruction_f1(gt, est, 0.01)}
        assert tuple(ref) == MH.METRIC_KEYS
        acc_d = spatial.KDTree(gt).query(est)[0]                     # what every accuracy function queries (evaluation.py:96-97)
        comp_d = spatial.KDTree(est).query(gt)[0]                    # what every completion function queries (evaluation.py:81-82)
        for k in ("acc_ratio", "acc_ratio_1cm", "comp_ratio", "comp_ratio_1cm"):
            assert 0.0 < ref[k] < 1.0, (i, k, ref[k])
        # no distance within the GPU test's bar of a threshold: the ratios of an fp32 kernel are then exactly these
        for d in (acc_d, comp_d):
            for th in (0.05, 0.01):
                assert np.abs(d - th).min() > 4 * BAR * th, (i, th)
        # the restatement must agree before anything is stored
        mine = MH.metrics(acc_d, comp_d)
        assert max(abs(mine[k] - ref[k]) for k in ref) < 1e-12, (mine, ref)
        d_acc, _ = MH.nearest(est32, gt32)
        d_comp, _ = MH.nearest(gt32, est32)
        assert np.abs(d_acc - acc_d).max() < 1e-12 and np.abs(d_comp - comp_d).max() < 1e-12
        out.update({f"p{i}_gt": gt32, f"p{i}_est": est32, f"p{i}_acc_dist": acc_d, f"p{i}_comp_dist": comp_d,
                    f"p{i}_metrics": np.array([ref[k] for k in MH.METRIC_KEYS], np.float64)})
        print(f"pair {i}: " + ", ".join(f"{k}={ref[k]:.6f}" for k in MH.METRIC_KEYS))
    out["num_pairs"] = np.int64(len(PAIRS))
    path = os.path.join(HERE, "g27_mesh_metrics.npz")
    np.savez_compressed(path, **out)
    print(f"g27_mesh_metrics: {os.path.getsize(path) / 1024:.1f} KiB")
    assert os.path.getsize(path) < 200 * 1000


if __name__ == "__main__":
    main()

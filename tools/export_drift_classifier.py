#!/usr/bin/env python3
"""Export the reference's pickled accent-drift classifier to the plain tables this provider reads (rho_tts_amd/forest.py):

    python tools/export_drift_classifier.py IN.pkl OUT.npz

IN.pkl is what validation/classifier/trainer.py saves with joblib: the metadata dict {'model': CalibratedClassifierCV(...),
'optimal_threshold': ...}, or the bare model.  It is unpickled HERE, on a file you name, with the scikit-learn that wrote it - loading
a pickle runs code from the file, so only export files you trust.  This is the one place that does so: the package itself never
unpickles, and OUT.npz holds arrays only (np.load(allow_pickle=False) reads it).  Point `MI355XQwenTTS(drift_model_path=OUT.npz)` at
the result; scikit-learn is then not needed on the serving host.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv) -> int:
    if len(argv) != 3:
        print(__doc__, file=sys.stderr)
        return 2
    import joblib
    from rho_tts_amd import forest as F
    tables = F.export_sklearn(joblib.load(argv[1]))
    F.save(argv[2], tables)
    back = F.load(argv[2])
    n_forests, n_trees = back["forest_first"].shape[0] - 1, back["tree_first"].shape[0] - 1
    print(f"{argv[2]}: {int(back['n_features'])} features, {n_forests} forest(s), {n_trees} trees, {back['node_feature'].shape[0]} nodes, "
          f"depth {F.tree_depth(back)}, {back['iso_first'].shape[0] - 1} calibrator(s) with {back['iso_x'].shape[0]} knots, "
          f"optimal_threshold {float(back['optimal_threshold']):g}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

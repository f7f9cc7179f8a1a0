#!/usr/bin/env python3
"""Train the accent-drift classifier on this build's own feature vectors, on the GPU (rho_tts_amd/forest_train.py):

    python tools/train_drift_classifier.py DATASET_DIR [OUT.npz] [--voice-id ID] [--speaker-encoder encoder.npz]

DATASET_DIR holds good/*.wav and bad/*.wav (16-bit PCM at any rate - what the provider's auto-sort writes).  The model family is the
reference's (validation/classifier/trainer.py: five cross-validated forests of 200 trees with one isotonic calibrator each, the
cost-sensitive threshold sweep); the rows are the ones inference computes - [256 GE2E | 30 hand-crafted] with --speaker-encoder (the
.npz of tools/export_speaker_encoder.py), the 30 alone without.  OUT.npz holds the version-1 tables (arrays only), OUT.json the
reference's metadata.  Without OUT.npz the file goes to ~/.rho_tts/models/{ID}_classifier.npz.  Point
`MI355XQwenTTS(drift_model_path=OUT.npz)` at the result; neither scikit-learn nor a pickle is involved anywhere.
"""
import argparse
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("dataset_dir")
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--voice-id", default=None)
    ap.add_argument("--speaker-encoder", default=None)
    args = ap.parse_args(argv[1:])
    logging.basicConfig(level=logging.INFO, format="%(levelname)s: %(message)s")
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    from rho_tts_amd import forest as F
    from rho_tts_amd import forest_train as T
    path = T.train(args.dataset_dir, voice_id=args.voice_id, output_path=args.out, speaker_encoder_path=args.speaker_encoder)
    back = F.load(path)
    print(f"{path}: {int(back['n_features'])} features, {back['forest_first'].shape[0] - 1} forests, {back['tree_first'].shape[0] - 1} trees, "
          f"{back['node_feature'].shape[0]} nodes, depth {F.tree_depth(back)}, {back['iso_x'].shape[0]} knots, "
          f"optimal_threshold {float(back['optimal_threshold']):g}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

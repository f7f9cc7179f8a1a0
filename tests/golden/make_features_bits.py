#!/usr/bin/env python3
"""Write tests/golden/features_bits.npz on an MI355X: what rt_features_extract (HandcraftedFeatures.raw) and
rt_features_extract_batch (HandcraftedFeatures.batch / f0_states) give for the clips of tests/test_features_bits_gpu.py.  The
committed arrays were recorded from the last build in which the two entry points launched their front-half kernels separately;
the build that gave both one path reproduces them bit for bit (profiles/r13_features_one_path.txt).  A refresh after a compiler
upgrade - which may move the float64 sums - is a run of this script; the bounds against the oracle in tests/test_features_gpu.py
and tests/test_features_batch_gpu.py keep anchoring the values.

    python tests/golden/make_features_bits.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import torch
    from rho_tts_amd import _native
    from rho_tts_amd import features as PF
    from tests.test_features_bits_gpu import BATCH_KINDS, FULL_CMND, inputs
    ctx = _native.Context(0)
    ex = PF.HandcraftedFeatures(ctx)
    ex.set_pitch_model()
    out = {}
    clips = inputs()
    for kind, (x, sr) in clips.items():
        out[f"sha256_{kind}"] = np.array(hashlib.sha256(x.tobytes()).hexdigest())
        stats, cmnd, lpc = ex.raw(torch.from_numpy(x).cuda(), sr)
        out[f"stats_{kind}"], out[f"lpc_{kind}"], out[f"cmnd_shape_{kind}"] = stats, lpc, np.array(cmnd.shape, dtype=np.int64)
        if kind in FULL_CMND:
            out[f"cmnd_{kind}"] = cmnd
    xs = [torch.from_numpy(clips[k][0]).cuda() for k in BATCH_KINDS]
    out["batch"] = ex.batch(xs, 24000)
    for kind, st in zip(BATCH_KINDS, ex.f0_states(xs, 24000)):
        out[f"states_{kind}"] = st
    np.savez_compressed(os.path.join(HERE, "features_bits.npz"), **out)
    ex.close()
    ctx.close()
    print("wrote features_bits.npz")


if __name__ == "__main__":
    main()

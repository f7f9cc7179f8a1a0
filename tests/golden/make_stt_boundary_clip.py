#!/usr/bin/env python3
"""Write tests/golden/stt_boundary_clip.npz on an MI355X: rt_stt_log_mel / rt_stt_encode of the 3-s boundary clip at 24 kHz
(tests/test_oracle_whisper.py::boundary_clip) on the seeded test model.  The committed arrays were recorded from the last build
that had the single-clip front-end kernels; the build that folded them into the batched path gave the same bits
(profiles/r12_stt_one_path.txt), so a refresh after a compiler upgrade - which may move the float64 contractions of both - is a
run of this script, and the bound against the oracle in tests/test_stt_batch_gpu.py keeps anchoring the values.

    python tests/golden/make_stt_boundary_clip.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from rho_tts_amd import _native
    from rho_tts_amd import stt as S
    from tests.test_oracle_whisper import boundary_clip
    cfg = S.tiny_test_config()
    ctx = _native.Context(0)
    nat = S.NativeSTT(ctx, cfg, {k: v.cuda() for k, v in S.synthetic_state(cfg, 789).items()})
    x = boundary_clip(cfg, 24000)
    np.savez(os.path.join(HERE, "stt_boundary_clip.npz"), log_mel=nat.log_mel(x, 24000).cpu().numpy(), states=nat.encode(x, 24000).cpu().numpy())
    nat.close()
    ctx.close()
    print("wrote stt_boundary_clip.npz")


if __name__ == "__main__":
    main()

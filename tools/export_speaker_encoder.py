#!/usr/bin/env python3
"""Export resemblyzer's speaker-encoder checkpoint to the plain arrays this provider reads (rho_tts_amd/speaker.py):

    python tools/export_speaker_encoder.py IN.pt OUT.npz

IN.pt is resemblyzer's ``pretrained.pt``: ``{"model_state": state_dict, ...}`` as its training script saves it, or a bare state dict
of ``torch.nn.LSTM(40, 256, num_layers=3)`` as ``lstm`` and ``torch.nn.Linear(256, 256)`` as ``linear``.  It is read with
``torch.load(..., weights_only=True)``: tensors and plain containers only, so a file that needs full unpickling is refused and no
code from the file runs.  This is the one place that reads the checkpoint: the package itself never unpickles, and OUT.npz holds
float32 arrays under torch's tensor names (np.load(allow_pickle=False) reads it).  ``similarity_weight`` / ``similarity_bias`` (the
GE2E loss's scale, not part of the embedding) are dropped; any other unknown tensor, a missing one or a wrong shape is an error.
Point ``MI355XQwenTTS(speaker_encoder_path=OUT.npz)`` or ``SpeakerEmbedder(ctx, OUT.npz)`` at the result.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DROPPED = ("similarity_weight", "similarity_bias")


def export(src: str, dst: str) -> dict:
    import torch
    from rho_tts_amd import speaker as S
    blob = torch.load(src, map_location="cpu", weights_only=True)
    if isinstance(blob, dict) and isinstance(blob.get("model_state"), dict):
        blob = blob["model_state"]
    if not isinstance(blob, dict) or not all(isinstance(v, torch.Tensor) for v in blob.values()):
        raise ValueError(f"{src}: neither a state dict nor {{'model_state': state dict}}")
    state = {k: v.detach().to(torch.float32).numpy() for k, v in blob.items() if k not in DROPPED}
    unknown = sorted(set(state) - {name for name, _ in S.tensor_specs()})
    if unknown:
        raise ValueError(f"{src}: tensors the encoder does not have: {unknown}")
    S.save(dst, state)                                     # (check_state: every tensor present, shapes, finite values)
    return S.load(dst)


def main(argv) -> int:
    if len(argv) != 3:
        print(__doc__, file=sys.stderr)
        return 2
    back = export(argv[1], argv[2])
    print(f"{argv[2]}: {len(back)} tensors, {sum(int(a.size) for a in back.values())} parameters, float32")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

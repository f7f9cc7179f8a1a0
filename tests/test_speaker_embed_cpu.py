"""CPU checks of the GE2E speaker encoder's host definitions (rho_tts_amd/speaker.py), of the oracle the GPU tests compare with
(tests/speaker_embed_ref.py) and of the export tool.  Parity with resemblyzer is unpinned: these hold the restated definition."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from rho_tts_amd import speaker as S
from tests import speaker_embed_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("export_speaker_encoder", os.path.join(ROOT, "tools", "export_speaker_encoder.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# (length at 16 kHz, partials, whether the last one is dropped, the length the clip is zero-padded to or None); worked from the definition
SLICES = [(8000, 1, False, 25600), (37000, 2, False, 37920), (38000, 2, True, None), (208000, 16, False, None), (217600, 17, False, None),
          (224000, 17, True, None), (1, 1, None, None)]


@pytest.mark.parametrize("n,parts,dropped,padded", SLICES)
def test_partial_slices(n, parts, dropped, padded):
    slices, n_pad = S.partial_slices(n)
    assert S.FRAME_STEP == 77
    assert len(slices) == parts and slices == [(77 * i, 77 * i + 160) for i in range(parts)]
    if padded is not None:
        assert n_pad == padded == 160 * slices[-1][1]
    assert n_pad >= n and n_pad >= 160 * slices[-1][1] and (n_pad == n or n_pad == 160 * slices[-1][1])
    if dropped is not None:
        n_frames = -(-(n + 1) // 160)
        undropped = len(range(0, max(1, n_frames - 160 + 77 + 1), 77))
        assert undropped == parts + (1 if dropped else 0)
        if dropped:                                                            # the partial that went covered less than 0.75 of its 25600 samples
            assert (n - 160 * 77 * parts) / 25600 < 0.75


def _smooth(bits: str):
    return "".join("1" if v else "0" for v in S.smooth_voice_flags([int(c) for c in bits]))


def test_smooth_voice_flags_hand_worked():
    # the window of 8 about flag w is flags[w - 3 .. w + 4]; the mask is 1 where MORE than four of them are set (4 / 8 = 0.5 rounds to 0)
    assert _smooth("0" * 12) == "0" * 12 and _smooth("") == ""
    assert _smooth("1" * 12) == "1" * 12                                       # averages 5/8 .. 1 at the ends, dilation covers the rest
    # four voiced flags: every window holds at most 4 -> average exactly 0.5 at best -> rounds to even 0 -> nothing kept
    assert _smooth("0000111100000") == "0" * 13
    # five voiced flags at 4..8: the windows about w = 4 .. 7 hold all five (w = 3 and w = 8 hold four) -> mask 4..7 -> dilated by +-3 -> 1..10
    assert _smooth("00001111100000") == "01111111111000"
    # two runs of nine ones (0..8 and 17..25) with 8 silent flags between.  First run: w = 7 sees flags 4..11, five ones -> 1; w = 8 sees
    # 5..12, four -> 0: mask 0..7.  Second run: w = 16 sees 13..20, four -> 0; w = 17 sees 14..21, five -> 1; w = 24 sees 21..28, five -> 1;
    # w = 25 sees 22..29, four -> 0: mask 17..24.  The gap between the mask runs is 8..16, nine flags -> the dilation (3 from either side)
    # leaves 11..13 out, and covers the last flag
    got = _smooth("1" * 9 + "0" * 8 + "1" * 9)
    assert got == "1" * 11 + "0" * 3 + "1" * 12, got
    # ... and with 5 silent flags between the runs the mask gap is six flags (8..13) -> bridged from both sides -> everything kept
    got = _smooth("1" * 9 + "0" * 5 + "1" * 9)
    assert got == "1" * 23, got
    # one silent flag more: a mask gap of seven -> the middle flag stays out
    got = _smooth("1" * 9 + "0" * 6 + "1" * 9)
    assert got == "1" * 11 + "0" + "1" * 12, got


def test_smooth_voice_flags_equals_the_convolution_form():
    """The cumulative-sum form against the same thing written as correlations, on random flags."""
    rng = np.random.default_rng(5)
    for n in (1, 2, 7, 8, 9, 133):
        f = rng.integers(0, 2, n)
        avg = np.array([f[max(0, w - 3): w + 5].sum() / 8.0 for w in range(n)])
        mask = np.round(avg).astype(bool)
        want = np.array([mask[max(0, w - 3): w + 4].any() for w in range(n)])
        assert np.array_equal(S.smooth_voice_flags(f), want)


def test_the_oracles_step_equations_are_torchs_lstm():
    """Gate order i, f, g, o and both biases: the hand-written steps equal torch.nn.LSTM in float64."""
    st = R.state()
    x = np.random.default_rng(3).standard_normal((3, 160, 40))
    with torch.no_grad():
        _, (h, _) = R.torch_lstm(st, torch.float64)(torch.from_numpy(x))
    want = h[-1].numpy()
    got = R.lstm_by_hand(st, x)
    assert np.abs(got - want).max() < 1e-12, float(np.abs(got - want).max())
    # and the biases matter: a state with bias_hh zeroed gives something else
    st2 = dict(st)
    st2["lstm.bias_hh_l0"] = np.zeros_like(st["lstm.bias_hh_l0"])
    assert np.abs(R.lstm_by_hand(st2, x) - want).max() > 1e-6


def test_specs_and_seeded_state():
    specs = S.tensor_specs()
    assert sum(int(np.prod(s)) for _, s in specs) == 1_423_616 and len(specs) == 14
    a, b = S.synthetic_state(1), S.synthetic_state(1)
    assert all(np.array_equal(a[k], b[k]) and a[k].dtype == np.float32 and np.abs(a[k]).max() <= 1 / 16 for k in a)
    assert not np.array_equal(a["linear.weight"], S.synthetic_state(2)["linear.weight"])


def test_oracle_volume_and_trim():
    x = (0.01 * np.sin(np.arange(8000) * 0.05)).astype(np.float32)
    y = R.normalize_volume(x)
    assert abs(20 * np.log10(np.sqrt(np.mean(y ** 2))) + 30.0) < 1e-9          # brought up to -30 dBFS
    loud = (0.5 * np.sin(np.arange(8000) * 0.05)).astype(np.float32)
    assert np.array_equal(R.normalize_volume(loud), loud.astype(np.float64))   # increase only
    assert np.array_equal(R.normalize_volume(np.zeros(10)), np.zeros(10))      # the stated deviation: no NaN
    z = np.arange(480 * 5 + 17, dtype=np.float32)
    assert np.array_equal(R.trim_long_silences(z, np.ones(5)), z[: 480 * 5])   # all voiced: only cut to a multiple of 480
    assert R.trim_long_silences(z, np.zeros(5)).size == 0


def test_export_tool_round_trip(tmp_path):
    tool = _tool()
    st = S.synthetic_state(11)
    full = {k: torch.from_numpy(v.copy()) for k, v in st.items()}
    full["similarity_weight"], full["similarity_bias"] = torch.tensor([10.0]), torch.tensor([-5.0])
    for name, blob in (("wrapped", {"model_state": full, "step": 7}), ("bare", full)):
        src, dst = str(tmp_path / f"{name}.pt"), str(tmp_path / f"{name}.npz")
        torch.save(blob, src)
        back = tool.export(src, dst)
        assert sorted(back) == sorted(st)
        assert all(back[k].dtype == np.float32 and back[k].shape == st[k].shape and np.array_equal(back[k], st[k]) for k in st)
        with np.load(dst, allow_pickle=False) as z:
            assert sorted(z.files) == sorted(st)
    assert tool.main(["x", str(tmp_path / "bare.pt"), str(tmp_path / "again.npz")]) == 0


def test_export_tool_refuses_wrong_shapes_and_pickles(tmp_path):
    tool = _tool()
    st = {k: torch.from_numpy(v.copy()) for k, v in S.synthetic_state(11).items()}
    bad = dict(st)
    bad["lstm.weight_ih_l0"] = torch.zeros(1024, 41)
    torch.save(bad, str(tmp_path / "bad.pt"))
    with pytest.raises(ValueError, match="lstm.weight_ih_l0"):
        tool.export(str(tmp_path / "bad.pt"), str(tmp_path / "bad.npz"))
    missing = {k: v for k, v in st.items() if k != "linear.bias"}
    torch.save(missing, str(tmp_path / "missing.pt"))
    with pytest.raises(ValueError, match="linear.bias"):
        tool.export(str(tmp_path / "missing.pt"), str(tmp_path / "missing.npz"))
    extra = dict(st)
    extra["lstm.weight_ih_l3"] = torch.zeros(2)
    torch.save(extra, str(tmp_path / "extra.pt"))
    with pytest.raises(ValueError, match="does not have"):
        tool.export(str(tmp_path / "extra.pt"), str(tmp_path / "extra.npz"))
    # a checkpoint that needs full unpickling (a reference to a function inside) is refused by weights_only=True
    import pickle
    torch.save({"model_state": st, "oops": os.getcwd}, str(tmp_path / "pickled.pt"))
    with pytest.raises((pickle.UnpicklingError, RuntimeError)):
        tool.export(str(tmp_path / "pickled.pt"), str(tmp_path / "pickled.npz"))
    assert not os.path.exists(str(tmp_path / "pickled.npz"))


def test_the_package_never_unpickles(tmp_path):
    with pytest.raises(ValueError, match="export_speaker_encoder"):
        S.load(str(tmp_path / "pretrained.pt"))
    with pytest.raises(ValueError, match="synthetic=True"):
        S.SpeakerEmbedder(None)


def test_provider_configuration():
    from rho_tts_amd.provider import MI355XQwenTTS
    kw = dict(device="cuda", speaker="Vivian", model_path="x/CustomVoice-small")
    t = MI355XQwenTTS(**kw)
    assert t.speaker_encoder_path is None and t.speaker_similarity == "model"
    with pytest.raises(ValueError, match="speaker_encoder_path"):
        MI355XQwenTTS(speaker_similarity="ge2e", **kw)
    with pytest.raises(ValueError, match="speaker_similarity"):
        MI355XQwenTTS(speaker_similarity="cosine", **kw)

"""Fixtures of the language tests (a helper, not a test): the smallest model with a language slot, the weight sets and clips of the
beam tests (tests/stt_beam_cases.py, tests/test_stt_batch_gpu.py::ragged_clips), and the recorded figures.

The configuration is ``tiny_test_config()`` with Whisper's special-token layout in small: end-of-sequence 290, start-of-transcript
291, languages 292 .. 295, transcribe 296, no-speech 297, no-timestamps 298; prefix (291, 292, 296, 298); 2-s windows.

Cases are the first windows of the seven ragged clips under every weight set of STATES.  The conditions on them - every case's
language margin (top-1 minus top-2 language logit on the CPU oracle) is at least MARGIN, and at least two different languages are
detected over all of them - are asserted on the CPU (tests/test_stt_lang_cpu.py), so that a change of the oracle's arithmetic that
erodes a margin fails there and does not flake on the GPU.  Weight sets A and B of the beam tests meet both: ids 292 and 294 are
detected, and the smallest margin is 0.18 (set A, clip(1.3, 3)), 1500 times MARGIN.
"""
import dataclasses

from rho_tts_amd import stt as S
from tests import stt_beam_cases as K

SR = K.SR
E = K.E                        # the project's recorded device-to-oracle log-probability error (tests/stt_beam_cases.py)
MARGIN = K.MARGIN

LANGUAGES = {"en": 292, "zh": 293, "ja": 294, "ko": 295}
NO_SPEECH = 297


def lang_test_config() -> S.SttConfig:
    return dataclasses.replace(S.tiny_test_config(), prefix=(291, 292, 296, 298), languages=dict(LANGUAGES), no_speech_id=NO_SPEECH, language="en")


STATES = K.STATES

# Measured on an MI355X (tests/test_stt_lang_gpu.py prints them): the largest |device - oracle| of the language log-probability and of
# the no-speech log-probability over the 14 cases, and over the three clips at Whisper-tiny dimensions.  The bound is 4 E = 1.2e-4.
MEASURED = {"tiny language": 4.16e-6, "tiny no-speech": 9.88e-6, "whisper-tiny language": 8.23e-6, "whisper-tiny no-speech": 4.37e-6}

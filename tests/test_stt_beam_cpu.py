"""The beam-search rule's float64 reference (tests/stt_beam_ref.py) against hand-built examples, the Python argument checks, the
transcriber's dispatch by beam width, and the decisive margins of the GPU fixtures (tests/stt_beam_cases.py) - asserted here so that a
change of the oracle's arithmetic that erodes one fails on the CPU and does not flake on the GPU."""
import math

import numpy as np
import pytest

from oracle import whisper as OW
from rho_tts_amd import stt as S
from tests import stt_beam_cases as K
from tests import stt_beam_ref as R

EOS = 3
NONE = np.zeros(4, dtype=bool)
# a four-id model whose next-token probabilities depend on the last token only (ids 0, 1, 2 and end-of-sequence)
START = [.6, .3, .08, .02]
AFTER = {0: [.5, .3, .1, .1], 1: [.1, .1, .1, .7], 2: [.25, .25, .25, .25]}


def table_logits(beams):
    return np.log(np.array([AFTER[b[-1]] if b else START for b in beams], dtype=np.float64))


def test_end_of_sequence_in_the_middle_of_the_walk_and_a_full_list_completes():
    """Width 2, three steps.  Step 0 takes 0 (.6) and 1 (.3).  Step 1 sorts 00 (.30), 1-end (.21), 01 (.18), 02 (.06: id 2 before the
    equally likely end-of-sequence), 10, 11: the walk takes 00, finishes [1], takes 01.  Step 2 sorts 000 (.15), 01-end (.126),
    001 (.09): [0, 1] finishes second and fills the list.  log(.126) / 3 beats log(.21) / 2."""
    r = R.search(table_logits, 2, 3, EOS, NONE)
    assert r.ids == [0, 1] and r.ended
    assert r.score == pytest.approx(math.log(.6 * .3 * .7)) and r.norm == pytest.approx(math.log(.126) / 3)
    assert [(i, e) for i, _, e in r.entries] == [([1], True), ([0, 1], True)]
    assert r.entries[0][1] == pytest.approx(math.log(.21))
    assert r.final_margin == pytest.approx(math.log(.126) / 3 - math.log(.21) / 2)
    # the margin: step 0 leaves id 2 (.08) behind 1 (.3); step 1 leaves 02 (.06) behind 01 (.18); step 2 leaves 002 (.03) behind 001
    # (.09); the final ranks are closer than all of them
    assert r.margin == pytest.approx(r.final_margin) and r.final_margin < math.log(.09 / .03)


def test_the_budget_runs_out_before_the_list_is_full():
    """The same model with two steps: after step 1 the list holds [1] alone, and the first live beam, [0, 0] (.30), fills it up - and
    wins on log(.30) / 3 against log(.21) / 2, though it never ended."""
    r = R.search(table_logits, 2, 2, EOS, NONE)
    assert r.ids == [0, 0] and not r.ended and r.score == pytest.approx(math.log(.30)) and r.norm == pytest.approx(math.log(.30) / 3)
    assert [(i, e) for i, _, e in r.entries] == [([1], True), ([0, 0], False)]
    # one step: nothing finished, both live beams fill the list in order, [0] first
    r = R.search(table_logits, 2, 1, EOS, NONE)
    assert [(i, e) for i, _, e in r.entries] == [([0], False), ([1], False)] and r.ids == [0]
    assert r.norm == pytest.approx(math.log(.6) / 2)


def test_the_list_fills_up_in_the_middle_of_a_step():
    """One slot left, two end-of-sequence candidates in the walk: 1-end (.4 x .8) is admitted, 0-end (.5 x .6) is not; the walk goes on
    to two next beams all the same."""
    lg = np.log(np.array([[.12, .06, .22, .6], [.05, .05, .1, .8]]))
    st = R.beam_step(lg, [math.log(.5), math.log(.4)], 2, EOS, NONE, n_fin=1)
    assert st.finished == [(1, pytest.approx(math.log(.32)))] and st.n_fin == 2 and st.done
    assert [(t, j) for t, j, _ in st.next] == [(2, 0), (0, 0)]
    assert st.next[0][2] == pytest.approx(math.log(.11)) and st.walk_gap == pytest.approx(math.log(.06 / .04))     # (1-2, .04, is left out)
    st = R.beam_step(lg, [math.log(.5), math.log(.4)], 2, EOS, NONE, n_fin=0)
    assert [j for j, _ in st.finished] == [1, 0] and st.done


def test_ties_go_to_the_lower_beam_then_the_lower_id():
    lg = np.log(np.array([[.5, .3, .1, .1]] * 2))
    st = R.beam_step(lg, [math.log(.5)] * 2, 2, EOS, NONE)
    assert [(t, j) for t, j, _ in st.next] == [(0, 0), (0, 1)] and st.order_gaps[0] == 0.0
    st = R.beam_step(lg, [math.log(.5)] * 2, 3, EOS, NONE)
    assert [(t, j) for t, j, _ in st.next] == [(0, 0), (0, 1), (1, 0)]
    lg = np.log(np.array([[.3, .3, .3, .1]]))
    assert [t for t, _, _ in R.beam_step(lg, [0.0], 2, EOS, NONE).next] == [0, 1]


def test_masks_and_nans():
    """Masked ids and NaNs are never candidates and do not count in the log-sum-exp; the begin mask holds at the first step only."""
    never, begin = np.array([False, False, True, False]), np.array([True, False, False, True])
    lg = np.array([[1.0, 0.5, 9.0, 0.0]])
    st = R.beam_step(lg, [0.0], 1, EOS, never, begin, first_step=True)
    assert [t for t, _, _ in st.next] == [1] and st.next[0][2] == pytest.approx(0.0) and not st.finished
    st = R.beam_step(lg, [0.0], 1, EOS, never, begin, first_step=False)
    assert st.next[0][0] == 0 and st.next[0][2] == pytest.approx(1.0 - math.log(math.e + math.exp(.5) + 1.0))
    st = R.beam_step(np.array([[float("nan"), 0.5, 9.0, 0.0]]), [0.0], 1, EOS, never)
    assert st.next[0][0] == 1 and np.isfinite(st.next[0][2])


@pytest.fixture(scope="module")
def oracle_models():
    cfg = S.tiny_test_config()
    return cfg, {name: OW.build(cfg, make(cfg)) for name, make in K.STATES.items()}


def test_width_one_is_the_greedy_rule(oracle_models):
    cfg, models = oracle_models
    lens = []
    for name in ("clip(1.7, 11)", "clip(1.3, 3)"):
        mel = R.window_mels(cfg, K.CLIPS[name](), K.SR)[0]
        want, _ = OW.greedy(models["A"], cfg, mel)
        got = R.beam_search(models["A"], cfg, mel, 1)
        assert got.ids == want and got.ended == (len(want) < cfg.max_new_tokens)
        assert got.score == pytest.approx(R.rescore(models["A"], cfg, mel, got.ids, got.ended), abs=1e-9)
        lens.append(len(want))
    assert lens == [1, 7]


def test_the_fixtures_keep_their_margins(oracle_models):
    """Every GPU fixture: its decisive margin is at least the margin constant (4 E, E measured on the GPU), and it is the case the
    list describes - so many ids, ended or not, different from greedy or not."""
    cfg, models = oracle_models
    assert K.MARGIN >= 4 * K.E
    seen = []
    for name, clip_name, B, margin, n_ids, ended, differs in K.CASES:
        mel = R.window_mels(cfg, K.CLIPS[clip_name](), K.SR)[0]
        r = R.beam_search(models[name], cfg, mel, B)
        greedy, _ = OW.greedy(models[name], cfg, mel)
        assert r.margin >= K.MARGIN, (name, clip_name, B, r.margin)
        assert r.margin == pytest.approx(margin, rel=0.05), (name, clip_name, B, r.margin)
        assert (len(r.ids), r.ended, r.ids != greedy) == (n_ids, ended, differs), (name, clip_name, B)
        assert r.score == pytest.approx(R.rescore(models[name], cfg, mel, r.ids, r.ended), abs=1e-4)
        seen.append((B, r.ids != greedy, r.ended and len(r.ids) < R.budget_of(cfg)))
    assert len(seen) >= 6 and {2, 3, 5} <= {s[0] for s in seen}
    assert sum(s[1] for s in seen) >= 4 and sum(s[2] for s in seen) >= 2


def test_python_argument_checks():
    for bad in (0, 9, -1, 2.0, True, None, "5"):
        with pytest.raises(ValueError):
            S.check_beam_size(bad)
    assert [S.check_beam_size(b) for b in (1, 5, np.int64(8))] == [1, 5, 8] and S.MAX_BEAM == 8
    with pytest.raises(ValueError):                        # before anything touches a device
        S.WhisperTranscriber(None, synthetic=True, beam_size=9)
    nat = object.__new__(S.NativeSTT)
    nat.handle = None
    for args in (([], 24000, 0), ([], 24000, 9), ([], 24000, 2, -1), ([], 24000, 2)):      # the last: a closed handle
        with pytest.raises(ValueError):
            nat.transcribe_ids_beam(*args)


class StubSTT:
    def __init__(self):
        self.calls = []

    def transcribe_ids(self, audio, sr):
        self.calls.append(("single", 1))
        return [1]

    def transcribe_ids_batch(self, audios, sr):
        self.calls.append(("batch", len(audios)))
        return [[1]] * len(audios)

    def transcribe_ids_beam(self, audios, sr, beam_size, max_tokens=None):
        self.calls.append(("beam", len(audios), beam_size))
        return [[2, 3]] * len(audios), [-0.25] * len(audios)


def transcriber(beam_size):
    tr = object.__new__(S.WhisperTranscriber)
    tr.model, tr.tokenizer, tr.beam_size = StubSTT(), None, beam_size
    return tr


def test_the_transcriber_dispatches_by_beam_width():
    tr = transcriber(1)
    assert tr("a", 24000) == "<1>" and tr.ids("a", 24000) == [1] and tr.ids_batch(["a", "b"], 24000) == [[1], [1]] and tr.batch(["a", "b"], 24000) == ["<1>"] * 2
    assert tr.model.calls == [("single", 1), ("single", 1), ("batch", 2), ("batch", 2)]          # exactly the calls of before
    assert tr.batch_scored(["a"], 24000) == [("<2> <3>", -0.25)] and tr.model.calls[-1] == ("beam", 1, 1)     # width 1, scored
    tr = transcriber(5)
    assert tr("a", 24000) == "<2> <3>" and tr.ids("a", 24000) == [2, 3] and tr.ids_batch(["a", "b"], 24000) == [[2, 3]] * 2
    assert tr.batch(["a", "b", "c"], 24000) == ["<2> <3>"] * 3 and tr.batch_scored(["a", "b"], 24000) == [("<2> <3>", -0.25)] * 2
    assert tr.model.calls == [("beam", 1, 5), ("beam", 1, 5), ("beam", 2, 5), ("beam", 3, 5), ("beam", 2, 5)]

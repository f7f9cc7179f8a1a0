"""Host side of decoding on up to 128 rows: the width chooser (engine.pick_rows) and the provider's batch_size clamp."""
import random
from typing import Sequence

import pytest

from rho_tts_amd import engine as engine_mod
from rho_tts_amd.engine import FRAME_COST, frame_cost, pick_rows


def pick_rows_64(plan: Sequence[int], max_batch: int) -> int:
    """pick_rows as it stood while engines had at most 64 rows (a copy: the new function must agree with it there)."""
    n = len(plan)
    full = min(n, max_batch)
    if full <= 32 or not plan:
        return full

    def cost(rows: int) -> float:
        frames = max(float(max(plan)), float(sum(plan)) / rows)
        return frames * (1.0 + 0.4 * max(0, rows - 32) / 32.0)
    return 32 if cost(32) < 0.9 * cost(full) else full


def plans():
    rnd = random.Random(1234)
    out = [[], [7], [44] * 20, [44] * 32, [44] * 33, [44] * 64, [44] * 65, [44] * 200, [26 + (37 * i) % 80 for i in range(64)]]
    for _ in range(120):
        n = rnd.choice((1, 5, 31, 32, 33, 40, 48, 63, 64, 65, 100, 128, 300))
        lo = rnd.randint(1, 60)
        hi = lo + rnd.choice((0, 1, 10, 80, 400))
        out.append([rnd.randint(lo, hi) for _ in range(n)])
    return out


def test_engines_of_up_to_64_rows_choose_what_they_always_chose():
    for plan in plans():
        for max_batch in range(1, 65):
            assert pick_rows(plan, max_batch) == pick_rows_64(plan, max_batch), (len(plan), max_batch)


def test_a_128_row_engine_chooses_among_32_64_and_the_full_width():
    """The frame costs at 96 and 128 rows are the ones measured in profiles/r18_rows128.txt (engine.FRAME_COST)."""
    assert [r for r, _ in FRAME_COST] == [32, 64, 96, 128] and FRAME_COST[0][1] == 1.0 and FRAME_COST[1][1] == 1.4
    wide_pays = frame_cost(128) / 128 <= frame_cost(64) / 64            # a 128-row frame is cheaper per row than a 64-row frame
    # 128 equal lengths: one 128-row batch - unless the measurement (profiles/r18_rows128.txt) says 128 rows lose to 64
    assert pick_rows([44] * 128, 128) == (128 if wide_pays else 64)
    ragged = [26 + (37 * i) % 80 for i in range(64)]
    assert pick_rows(ragged * 8, 128) > 64 if wide_pays else pick_rows(ragged * 8, 128) == 64     # a long ragged queue
    assert pick_rows([], 128) == 0
    for plan in plans():
        for max_batch in (65, 96, 127, 128):
            got = pick_rows(plan, max_batch)
            full = min(len(plan), max_batch)
            assert 0 <= got <= full and (got == full or got in (32, 64)), (len(plan), max_batch, got)
            if got > 64:                                                 # never a width whose row-frame costs more than a 64-row frame's
                assert frame_cost(got) / got <= frame_cost(64) / 64, (got, len(plan))
            if full <= 64:
                assert got == pick_rows_64(plan, max_batch)
    assert frame_cost(32) == 1.0 and frame_cost(64) == 1.4 and frame_cost(96) == FRAME_COST[2][1] and frame_cost(128) == FRAME_COST[3][1]


@pytest.mark.parametrize("asked,got", [(128, 128), (500, 128), (64, 64), (0, 1)])
def test_provider_hands_batch_size_to_the_engine_clamped_to_128(monkeypatch, asked, got):
    from rho_tts_amd.provider import MI355XQwenTTS
    seen = {}

    class _Cfg:
        hf_max_position_embeddings = 0

    class _Engine:
        def __init__(self, model_path, device_ordinal=0, max_batch=32, **kw):
            seen["max_batch"] = max_batch
            self.cfg = _Cfg()
            self.max_batch = max_batch

        def close(self):
            pass

    monkeypatch.setenv("RHO_TTS_AMD_SYNTHETIC", "1")
    monkeypatch.setattr(engine_mod, "Engine", _Engine)
    t = MI355XQwenTTS(device="cuda", reference_audio="ref.wav", reference_text="the reference words", batch_size=asked)
    eng = t._load_engine()
    assert seen["max_batch"] == got and eng.max_batch == got
    # more segments than rows go down in ONE call (continuous batching) on engines of up to 128 rows
    todo = list(range(got + 5))
    assert t._cut_batches(todo, None, got) == [todo]

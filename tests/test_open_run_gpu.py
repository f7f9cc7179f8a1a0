"""An open run on the GPU (rt_generate_open / _submit / _cancel_item): items join a decode batch in flight, and every one of them is
bit for bit what it gets alone with its voice on the path that existed before - a SECOND model created without max_voices, one item
per rt_generate.

1. items submitted before the first step, mid-run onto free rows, while the rows are busy (hand-over, a re-voiced block) and after
   the run went idle - preset `small` under rt_debug_tune 1500 and 1501, preset `tiny`; hand-over cadence 4 and 1;
2. rows parked for more frames than max_positions minus the shortest prefix;
3. refusals leave the run intact, a spent horizon included;
4. rt_generate_cancel_item for a waiting and a decoding item."""
import contextlib
import ctypes

import pytest
import torch

from oracle.model import Voice
from rho_tts_amd import config, weights

pytestmark = pytest.mark.gpu

SAMPLING = (1, 0.9, 50, 1.0, 1.05)
A, B, C, D = 0, 1, 2, 3
RT_OK, RT_ERR_INVALID, RT_ERR_LENGTH, RT_ERR_STATE, RT_ERR_UNSUPPORTED = 0, 1, 3, 6, 7


@pytest.fixture(scope="module")
def ctx():
    from rho_tts_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


def clone(cfg, n_ref, seed):
    g = torch.Generator().manual_seed(seed)
    return Voice("english", speaker_embed=torch.randn(cfg.talker.hidden, generator=g) * 0.05,
                 ref_text_ids=[int(v) for v in torch.randint(0, cfg.text_vocab - 64, (5,), generator=g)],
                 ref_codes=torch.randint(0, cfg.codec.codebook_size, (n_ref, cfg.n_groups), generator=g))


def set_voice(nm, v):
    return nm.set_voice(v.language, v.speaker, v.speaker_embed, v.ref_text_ids, v.ref_codes)


class Models:
    """A bank model with `voices` resident (the open runs) and a plain one without max_voices (every item alone)."""

    def __init__(self, ctx, preset, voices, max_batch=16, max_positions=None):
        from rho_tts_amd._native_model import NativeModel, RtSampling
        self.cfg = config.PRESETS[preset]()
        state = {k: v.cuda() for k, v in weights.synthetic_state(self.cfg, 789).items()}
        self.bank = NativeModel(ctx, self.cfg, max_batch=max_batch, max_voices=4, max_positions=max_positions)
        self.bank.load_state(state)
        self.plain = NativeModel(ctx, self.cfg, max_batch=max_batch, max_positions=max_positions)
        self.plain.load_state(state)
        self.voices, self.sp = voices, RtSampling(*SAMPLING)
        self.lens = []
        for i, v in enumerate(voices):
            self.bank.select_voice(i)
            self.lens.append(set_voice(self.bank, v))
        self.bank.select_voice(0)
        self._alone, self._plain_voice, self.form = {}, None, 0

    def close(self):
        self.bank.close()
        self.plain.close()

    @contextlib.contextmanager
    def decode_form(self, mfma):
        assert self.bank.lib.rt_debug_tune(1500 + mfma, 0) == 0
        self.form = mfma
        try:
            yield
        finally:
            assert self.bank.lib.rt_debug_tune(1500, 0) == 0
            self.form = 0

    @contextlib.contextmanager
    def cadence(self, every):
        assert self.bank.lib.rt_debug_tune(1700 + every, 0) == 0
        try:
            yield
        finally:
            assert self.bank.lib.rt_debug_tune(1704, 0) == 0

    def items(self, n, seed):
        g = torch.Generator().manual_seed(seed)
        texts = [[int(t) for t in torch.randint(0, self.cfg.text_vocab - 64, (int(k),), generator=g)] for k in torch.randint(3, 10, (n,), generator=g)]
        frames = [int(f) for f in torch.randint(3, 9, (n,), generator=g)]
        return texts, frames, [500 + 13 * i for i in range(n)]

    def alone(self, v, text, frames, item_id):
        key = (self.form, v, tuple(text), frames, item_id)
        if key not in self._alone:
            if self._plain_voice != v:
                assert set_voice(self.plain, self.voices[v]) == self.lens[v]
                self._plain_voice = v
            self._alone[key] = self.plain.generate([text], [frames], self.sp, seed=5, item_ids=[item_id])[0]
        return self._alone[key]

    def open(self, rows=8, max_text=9, max_frames=8, horizon=256, voices=(A, B, C, D), **kw):
        self.bank.generate_open(rows, max_text, max_frames, horizon, list(voices), self.sp, seed=5, **kw)

    def drain(self, every, limit=400):
        for _ in range(limit):
            run, done = self.bank.generate_step(every)
            if done:
                return run
        raise AssertionError("the run did not drain")

    def same_as_alone(self, idx, texts, frames, ids, voices):
        """every item of `idx` (item number in the run -> position in the lists), read by rt_generate_peek, against itself alone"""
        got = {}
        for item, i in idx.items():
            got[i], fin = self.bank.generate_peek(item, 0, frames[i])
            assert fin and got[i].shape[0] == frames[i] and int(got[i].abs().sum()) > 0, (item, i)
        for v in sorted(set(voices[i] for i in got)):                  # (grouped: the plain model changes voice once per voice)
            for i in [i for i in got if voices[i] == v]:
                assert torch.equal(got[i], self.alone(v, texts[i], frames[i], ids[i])), (i, v)
        return got


@pytest.fixture(scope="module")
def small(ctx):
    cfg = config.small()
    m = Models(ctx, "small", [clone(cfg, 56, 5), clone(cfg, 90, 6), clone(cfg, 56, 7), Voice("chinese", speaker="ryan")])
    a, b, c, d = m.lens
    assert a >= 64 and a % 32 and b > a and c == a and d < 64, m.lens
    yield m
    m.close()


# ------------------------------------------------------------------------------------------------ 1. item by item
VOICES_14 = [A, B, A, B, A, B, A, B, C, A, B, C, D, C]


def arrivals(m, every, voices, n_decl):
    """14 items over 8 rows (two 4-row blocks): 0, 1 with the open call, 2, 3 before the first step; after one step 4 and 5 find free
    rows of their voices; 6 .. 11 come at once - more than the free rows, and voice C has no block until one has drained (re-voiced);
    12, 13 come after the run has gone idle."""
    texts, frames, ids = m.items(14, 61)
    nm = m.bank
    sub = lambda i: nm.generate_submit(texts[i], frames[i], ids[i], voices[i])          # noqa: E731
    m.open(voices=list(range(n_decl)), first=[(texts[i], frames[i], ids[i], voices[i]) for i in (0, 1)])
    idx = {0: 0, 1: 1}
    for i in (2, 3):
        idx[sub(i)] = i
    run, done = nm.generate_step(1)
    assert run == 1 and not done
    for i in (4, 5):
        idx[sub(i)] = i
    run, done = nm.generate_step(1)
    assert run == 2 and not done
    for i in range(6, 12):
        idx[sub(i)] = i
    assert sorted(idx) == list(range(12))
    run = m.drain(every)
    assert nm.generate_step(every) == (run, True) and nm.generate_step(every) == (run, True)      # idle: no frame is launched
    for i in (12, 13):
        idx[sub(i)] = i
    run2, done = nm.generate_step(1)
    assert run2 == run + 1 and not done
    m.drain(every)
    got = m.same_as_alone(idx, texts, frames, ids, voices)
    nm.generate_end()
    st = nm.generate_stats()
    assert st["rows"] == 8 and st["frames_kept"] == sum(frames) and st["hand_overs"] >= 2, st
    # the same items as a closed list: the same codes
    closed = nm.generate(texts, frames, m.sp, seed=5, item_ids=ids, voices=voices, max_rows=8)
    assert all(torch.equal(closed[i], got[i]) for i in range(14))
    return st


@pytest.mark.parametrize("every", [4, 1])
@pytest.mark.parametrize("mfma", [0, 1])
def test_small_items_join_a_run_in_flight(small, mfma, every):
    with small.decode_form(mfma), small.cadence(every):
        arrivals(small, every, VOICES_14, 4)
        assert small.bank.revoiced_blocks() >= 1


def test_small_one_declared_voice_takes_the_block_table_form(small):
    """a session with one voice: still the block-table form, every item what the single-voice path gives it"""
    with small.cadence(4):
        arrivals(small, 4, [A] * 14, 1)


@pytest.mark.parametrize("every", [4, 1])
def test_tiny_items_join_a_run_in_flight(ctx, every):
    cfg = config.tiny()
    m = Models(ctx, "tiny", [Voice("english", speaker="vivian"), Voice("chinese", speaker="ryan"), clone(cfg, 9, 8), clone(cfg, 70, 9)], max_batch=8)
    try:
        assert m.lens[0] == m.lens[1] and m.lens[2] > m.lens[0] and m.lens[3] >= 64
        with m.cadence(every):
            arrivals(m, every, VOICES_14, 4)
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ 2. parked rows in a long run
def test_small_rows_stay_parked_past_max_positions(ctx):
    """One row of block 0 decodes one long item of voice A after another; block 1 had a short item of voice D (the shortest prefix) and
    its rows then idle for more frames than max_positions - len(D): a parked row that just stepped on would leave the cache.  What keeps
    them inside is the rule a closed multi-voice list already had: every look that places an item puts EVERY free row back behind its
    prefix, and between two such looks a run decodes at most max_frames + cadence frames, which rt_generate_open bounds below
    max_positions for every declared voice.  (The extra re-park of a row that comes within 2 x cadence of max_positions is a safety
    net behind that rule; no schedule that the open call admits reaches it, and this test does not.)  Preset small with 256
    positions instead of its 1024: the same code at a quarter of the frames."""
    cfg = config.small()
    small = Models(ctx, "small", [clone(cfg, 56, 5), Voice("chinese", speaker="ryan")], max_batch=8, max_positions=256)
    try:
        _parked_rows(small, 0, 1)
    finally:
        small.close()


def _parked_rows(small, A, D):
    nm, every = small.bank, 4
    max_pos, la, ld = nm.max_positions, small.lens[A], small.lens[D]
    texts, _, ids = small.items(5, 62)
    texts = [t[:3] for t in texts]
    big = max_pos - la - (3 + 2) - every - 1                        # the largest item that fits behind voice A
    frames, voices = [3, big, big, big, big], [D, A, A, A, A]
    # long items: each joins 2 x every frames before the one decoding ends; block 1 idles from frame 3 + every at the latest
    n_long = 1
    while big + (n_long - 1) * (big - 2 * every) - 3 - every <= max_pos - ld:
        n_long += 1
    assert 2 <= n_long <= 4, n_long
    with small.cadence(every):
        small.open(max_frames=big, horizon=(n_long + 2) * (big + 2 * every) + 64, voices=[A, D])
        idx = {nm.generate_submit(texts[0], 3, ids[0], D): 0, nm.generate_submit(texts[1], big, ids[1], A): 1}
        for i in range(2, n_long + 1):
            # the next long item joins shortly before the one decoding ends: a row of block 0 is always busy, the run never idle
            prev = next(k for k, v in idx.items() if v == i - 1)
            for _ in range(400):
                run, done = nm.generate_step(every)
                assert not done
                if nm.generate_peek(prev, 0, big)[0].shape[0] >= big - 2 * every:
                    break
            idx[nm.generate_submit(texts[i], big, ids[i], A)] = i
        run = small.drain(every)
        assert run - 3 - every > max_pos - ld, (run, max_pos, ld)
        small.same_as_alone(idx, texts, frames, ids, voices)
        nm.generate_end()
        assert nm.generate_stats()["frames_kept"] == sum(frames[: len(idx)])


# ------------------------------------------------------------------------------------------------ 3. refusals
def rc_submit(nm, text, frames, item_id, voice):
    ids = (ctypes.c_int32 * max(1, len(text)))(*text)
    item = ctypes.c_int32(-1)
    return nm.lib.rt_generate_submit(nm.handle, ids, len(text), frames, item_id, voice, ctypes.byref(item))


def test_small_refusals_leave_the_run_intact(small):
    nm, every = small.bank, 4
    texts, frames, ids = small.items(12, 63)
    voices = [A, B, D, A, B, D, A, B, D, A, B, D]
    assert rc_submit(nm, texts[0], frames[0], ids[0], A) == RT_ERR_STATE                       # no run at all
    nm.generate_begin(texts[:2], frames[:2], small.sp, seed=5, item_ids=ids[:2])
    assert rc_submit(nm, texts[0], frames[0], ids[0], A) == RT_ERR_STATE                       # a closed-list run
    assert nm.lib.rt_generate_cancel_item(nm.handle, 0) == RT_ERR_STATE
    nm.generate_end()
    one = (ctypes.c_int32 * 16)()
    with pytest.raises(RuntimeError, match="unsupported|teacher|trace"):
        small.open(_forced=one)
    dummy = torch.zeros(16, device="cuda")
    with pytest.raises(RuntimeError, match="unsupported|teacher|trace"):
        small.open(_trace=dummy.data_ptr())
    nm.clear_voice(C)
    try:
        with pytest.raises(ValueError):
            small.open(voices=[A, C])                                                          # a declared voice that is not set
        with small.cadence(every):
            # horizon 60: at frame 0 an 8-frame item fits while (8 + 4) * unfinished / 2 blocks + 8 + 10 <= 60, i.e. seven of them
            small.open(horizon=60, voices=[A, B, D])
            idx = {}
            for i in range(3):
                idx[nm.generate_submit(texts[i], frames[i], ids[i], voices[i])] = i
            nm.generate_step(1)
            assert rc_submit(nm, texts[3] + [1] * 7, 4, 1, A) == RT_ERR_INVALID                # text longer than declared (9)
            assert rc_submit(nm, texts[3], 9, 1, A) == RT_ERR_INVALID                          # frames above declared (8)
            assert rc_submit(nm, texts[3], 0, 1, A) == RT_ERR_INVALID
            assert rc_submit(nm, texts[3], 4, 1, C) == RT_ERR_INVALID                          # not declared, and not set either
            assert rc_submit(nm, texts[3], 4, 1, 7) == RT_ERR_INVALID                          # outside the bank
            assert rc_submit(nm, [small.cfg.text_vocab], 4, 1, A) == RT_ERR_INVALID
            refused = None
            for i in range(3, 12):
                rc = rc_submit(nm, texts[i], 8, ids[i], voices[i])
                if rc != RT_OK:
                    refused = i
                    assert rc == RT_ERR_LENGTH and "horizon is spent" in nm.lib.rt_last_error(nm.ctx.handle).decode()
                    break
                idx[len(idx)] = i
            assert refused is not None and refused >= 5, refused
            fr = frames[:3] + [8] * 9
            small.drain(every)
            small.same_as_alone(idx, texts, fr, ids, voices)                                   # the live items finished, each as alone
            nm.generate_end()
            assert nm.generate_stats()["frames_kept"] == sum(fr[i] for i in idx.values())
            small.open(horizon=60, voices=[A, B, D])                                           # a reopened run serves the refused item
            idx = {nm.generate_submit(texts[refused], 8, ids[refused], voices[refused]): refused}
            small.drain(every)
            small.same_as_alone(idx, texts, fr, ids, voices)
            nm.generate_end()
    finally:
        nm.select_voice(C)
        set_voice(nm, small.voices[C])
        nm.select_voice(A)
    # positions: prefix + suffix + frames beyond max_positions
    with small.cadence(every):
        most = nm.max_positions - small.lens[D] - 2 * every - 1        # the most frames a run behind voice D can be opened for
        with pytest.raises(RuntimeError, match="length"):
            small.open(max_frames=most + 1, horizon=4 * nm.max_positions, voices=[D])
        small.open(max_frames=most, horizon=4 * nm.max_positions, voices=[D])
        assert rc_submit(nm, texts[0], most, 1, D) == RT_ERR_LENGTH     # ... and a text of three tokens or more does not fit beside them
        assert "max_positions" in nm.lib.rt_last_error(nm.ctx.handle).decode()
        idx = {nm.generate_submit(texts[0], frames[0], ids[0], D): 0}
        small.drain(every)
        small.same_as_alone(idx, texts, frames, ids, [D])
        nm.generate_end()


# ------------------------------------------------------------------------------------------------ 4. cancel
def test_small_cancel_a_waiting_and_a_decoding_item(small):
    nm, every = small.bank, 4
    texts, _, ids = small.items(8, 64)
    frames = [8, 8, 8, 8, 8, 6, 5, 7]
    voices = [A, A, A, A, A, B, A, A]                                  # 4 rows = one block: items 0 .. 3 decode, 4 .. 7 wait
    with small.cadence(every):
        small.open(rows=4, voices=[A, B])
        idx = {nm.generate_submit(texts[i], frames[i], ids[i], voices[i]): i for i in range(8)}
        assert nm.generate_step(3) == (3, False)
        nm.generate_cancel_item(1)                                     # decoding: three frames so far
        nm.generate_cancel_item(4)                                     # waiting
        part, fin = nm.generate_peek(1, 0, 8)
        assert fin and part.shape[0] == 3
        none, fin = nm.generate_peek(4, 0, 8)
        assert fin and none.shape[0] == 0
        small.drain(every)
        nm.generate_cancel_item(2)                                     # after it has finished: nothing changes
        again, fin = nm.generate_peek(1, 0, 8)
        assert fin and torch.equal(again, part) and torch.equal(part, small.alone(A, texts[1], 8, ids[1])[:3])
        assert nm.generate_peek(4, 0, 8)[0].shape[0] == 0
        rest = {k: v for k, v in idx.items() if v not in (1, 4)}
        small.same_as_alone(rest, texts, frames, ids, voices)
        nm.generate_end()
        st = nm.generate_stats()
        assert st["frames_kept"] == sum(frames) - 8 - 8 + 3 and st["hand_overs"] >= 2, st       # (item 1's row was handed on)
        with pytest.raises(ValueError):
            small.open(rows=4, voices=[A, B])
            try:
                nm.generate_cancel_item(0)                             # no such item
            finally:
                nm.generate_end()

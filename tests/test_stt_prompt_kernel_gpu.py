"""The kernels of a prompt policy on their own (rt_debug_stt_prompt_prefix, rt_debug_stt_beam_reorder_range): the ragged prefix pass
against transformers' forward behind the same tokens, a window in a joint pass against the window alone, the ranged gather on a
patterned cache, and the longest prefix of Whisper-tiny dimensions (227 tokens) with three greedy steps behind it.

The bound on the prefix pass is 4 E on the last row's logits as they stand, and on their log-softmax - the quantity E
(tests/stt_beam_cases.py) was measured on.  Measured on an MI355X (this file prints the figures): see MEASURED in tests/stt_prompt_cases.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import whisper as OW
from rho_tts_amd import _native
from rho_tts_amd import stt as S
from tests import stt_beam_ref as R
from tests import stt_prompt_cases as PC
from tests import stt_prompt_ref as P
from tests import stt_seek_ref as SR
from tests.test_oracle_whisper import clip

pytestmark = pytest.mark.gpu

SR_IN = PC.SR
CFG = PC.prompt_test_config()


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def declare(lib):
    i32, vp = C.c_int32, C.c_void_p
    lib.rt_debug_stt_beam_reorder_range.argtypes = [vp, i32, i32, i32, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_uint16)]
    lib.rt_debug_stt_prompt_prefix.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int64), i32, i32, C.POINTER(i32), C.POINTER(i32), vp]


def prefix_logits(nat, clips, rows):
    """rt_debug_stt_prompt_prefix: the logits [len(clips)][vocab] behind the token rows, one per clip's first window."""
    declare(nat.lib)
    xs, n, ptrs, lens = nat._clips(clips)
    flat = [t for r in rows for t in r]
    out = torch.empty(n, nat.cfg.vocab, dtype=torch.float32, device=xs[0].device)
    nat.ctx.check(nat.lib.rt_debug_stt_prompt_prefix(nat.handle, ptrs, lens, n, SR_IN, (C.c_int32 * len(flat))(*flat), (C.c_int32 * n)(*[len(r) for r in rows]),
                                                     C.c_void_p(out.data_ptr())), "rt_debug_stt_prompt_prefix")
    return out.cpu().double().numpy()


def oracle_logits(model, cfg, x, row):
    enc = R.encode(model, SR.own_features(cfg, x, SR_IN)(0, min(len(x), cfg.chunk_seconds * SR_IN)))
    return SR._logits(model, enc, row, [[]])[0]


def log_softmax(z):
    m = z.max(axis=-1, keepdims=True)
    return z - (m + np.log(np.exp(z - m).sum(axis=-1, keepdims=True)))


@pytest.mark.parametrize("st", ["A", "B"])
def test_ragged_prefix_pass(ctx, st):
    """Prefix lengths 3, 4, 11 and 19 (the longest the small model takes) in one pass: every window's last-row logits against the
    oracle, and bit-equal to the window in a pass of its own."""
    state = PC.STATES[st](CFG)
    nat = S.NativeSTT(ctx, CFG, {k: v.cuda() for k, v in state.items()})
    try:
        model = OW.build(CFG, state)
        forced = SR.ts_prefix(CFG)
        text = [7, 19, 33, 48, 64, 81, 99, 118, 138, 159, 181, 204, 228, 253, 279]
        rows = [forced, forced + [CFG.timestamp_begin + 3], [CFG.sot_prev_id] + text[:7] + forced, [CFG.sot_prev_id] + text + forced]
        assert [len(r) for r in rows] == [3, 4, 11, 19]
        clips = [PC.CLIPS[k]()[:2 * SR_IN] for k in ("clip(5.0, 2)", "clip(6.3, 11)", "clip(4.1, 5)", "clip(7.0, 3)")]
        joint = prefix_logits(nat, clips, rows)
        worst = raw = 0.0
        for w, (x, r) in enumerate(zip(clips, rows)):
            want = oracle_logits(model, CFG, x, r)
            worst = max(worst, float(np.abs(log_softmax(joint[w]) - log_softmax(want)).max()))
            raw = max(raw, float(np.abs(joint[w] - want).max()))
            alone = prefix_logits(nat, [x], [r])
            assert np.array_equal(alone[0], joint[w]), w
        print(f"set {st}: ragged prefix pass max |log-softmax - oracle| {worst:.3g} (raw logits {raw:.3g}), bound {4 * PC.E:.3g}")
        assert worst <= 4 * PC.E and raw <= 4 * PC.E
        # a row too long, an id outside the vocabulary: refused, nothing launched, and the handle answers afterwards
        declare(nat.lib)
        xs, n, ptrs, lens = nat._clips(clips[:1])
        out = torch.empty(1, CFG.vocab, dtype=torch.float32, device=xs[0].device)
        for bad in ([0] * 20, [CFG.vocab], []):
            rc = nat.lib.rt_debug_stt_prompt_prefix(nat.handle, ptrs, lens, 1, SR_IN, (C.c_int32 * max(len(bad), 1))(*bad), (C.c_int32 * 1)(len(bad)), C.c_void_p(out.data_ptr()))
            assert rc == _native.RT_ERR_INVALID, bad
        assert np.array_equal(prefix_logits(nat, clips[:1], rows[:1])[0], joint[0])
    finally:
        nat.close()


def test_ranged_gather(ctx):
    """2 layers, 6 rows, ranges that are empty, of one position and up to the last position of the cache: inside its range a row
    holds its parent's pattern, everything else keeps the destination's sentinel, and the source cache is as it was."""
    lib = ctx.lib
    declare(lib)
    L, rows, H, Pmax, d = 2, 6, 2, 9, 32
    src = [1, 0, 2, 2, 5, 3]
    lo = [0, 3, 4, 8, 9, 2]
    hi = [0, 4, 9, 9, 9, 2]                                   # empty at 0, one position, to the end, the last position alone, empty at the end, empty inside
    n = L * rows * H * Pmax * d
    out = (C.c_uint16 * (8 * n))()
    i32 = lambda v: (C.c_int32 * rows)(*v)                   # noqa: E731
    ctx.check(lib.rt_debug_stt_beam_reorder_range(ctx.handle, L, rows, H, Pmax, d, i32(src), i32(lo), i32(hi), out), "rt_debug_stt_beam_reorder_range")
    got = np.frombuffer(out, dtype=np.uint16).reshape(2, 4, L, rows, H, Pmax, d)
    i = np.arange(n, dtype=np.int64)
    pattern = np.stack([((i * 40503 + q * 12289) & 0x7fff).astype(np.uint16) for q in range(4)]).reshape(4, L, rows, H, Pmax, d)
    assert np.array_equal(got[0], pattern)
    want = np.full_like(pattern, 0xbeef)
    for r, parent in enumerate(src):
        want[:, :, r, :, lo[r]:hi[r]] = pattern[:, :, parent, :, lo[r]:hi[r]]
    assert np.array_equal(got[1], want)
    for bad_lo, bad_hi in (([-1] + lo[1:], hi), (lo, [10] + hi[1:]), ([5] + lo[1:], [4] + hi[1:])):
        assert lib.rt_debug_stt_beam_reorder_range(ctx.handle, L, rows, H, Pmax, d, i32(src), i32(bad_lo), i32(bad_hi), out) == _native.RT_ERR_INVALID


def test_whisper_tiny_dimensions(ctx):
    """An initial prompt of the full 223 ids: a prefix of 227 tokens.  The prefix-pass logits against the oracle, then the seek call -
    three greedy steps behind that prefix - against the restated loop."""
    cfg = S.SttConfig(max_new_tokens=3, timestamp_begin=50364)
    state = S.synthetic_state(cfg, 789)
    nat = S.NativeSTT(ctx, cfg, {k: v.cuda() for k, v in state.items()})
    try:
        model = OW.build(cfg, state)
        initial = [int(t) for t in np.random.default_rng(20).integers(0, cfg.eos_id, P.prompt_cap(cfg))]
        row = P.window_prefix(cfg, cfg.sot_prev_id, initial)
        assert len(initial) == 223 and len(row) == 227
        x = clip(4.0, SR_IN, 3)
        got = prefix_logits(nat, [x], [row])[0]
        want = oracle_logits(model, cfg, x, row)
        err, raw = float(np.abs(log_softmax(got) - log_softmax(want)).max()), float(np.abs(got - want).max())
        print(f"Whisper-tiny dimensions, 227 prefix rows: max |log-softmax - oracle| {err:.3g} (raw logits {raw:.3g}), bound {4 * PC.E:.3g}")
        assert err <= 4 * PC.E and raw <= 4 * PC.E
        nat.set_prompt(initial, condition_on_previous=False)
        clip_, = nat.transcribe_ids_seek([x], SR_IN, 1, no_speech=False)
        ref = P.clip_transcribe(model, cfg, x, SR_IN, 1, cfg.sot_prev_id, cfg.max_initial_timestamp_index, False, initial)
        w, r = clip_.windows[0], ref.windows[0]
        print(f"three greedy steps behind it: margin {ref.margin:.3g} ids {r.ids} |logprob - reference| {abs(w.logprob - r.logprob):.3g}")
        assert len(clip_.windows) == 1 and w.prompt_len == 223 and w.n_ids == len(r.ids) == 3
        assert ref.margin >= PC.MARGIN                       # (1.79e-3 on the CPU reference: PC.TINY_CASE)
        assert clip_.ids == ref.ids and abs(w.logprob - r.logprob) <= 4 * PC.E
    finally:
        nat.close()

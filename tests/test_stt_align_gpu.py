"""Token and word times on the GPU (rt_stt_align; DESIGN.md section 5, "word times") against tests/stt_align_ref.py: the path kernel
exactly, the matrix kernel within one float32 ulp, the probabilities kernel within 4 x torch's own float32 error, the model path
against the oracle's cross-attention, batch invariance bit for bit, the argument rules, and the Python layer end to end.

Measured on an MI355X (this file prints the figures): see MEASURED below and DESIGN.md section 5."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from oracle import whisper as OW
from rho_tts_amd import _native
from rho_tts_amd import stt as S
from tests import stt_align_ref as R
from tests import stt_seek_cases as SC
from tests.test_oracle_whisper import clip

pytestmark = pytest.mark.gpu

SR_IN = 24000
CFG = S.tiny_test_config()
HEADS = CFG.aligned_heads
# Largest |device - oracle| on the three clips of the model path, measured on an MI355X: the probabilities W (values of order 1e-2) and
# the token log-probabilities.  The bars are 4 x these.
MEASURED = {"W": 3.91e-8, "logprob": 5.25e-6}
vp, i32, i64, f32p, i32p = C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_float), C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    lib = c.lib
    lib.rt_debug_stt_align_probs.argtypes = [vp, vp, i32, i32, i32, vp, vp, i32, i32, i32p, i32p, i32p, i32, i32p, i32, i32, vp]
    lib.rt_debug_stt_align_matrix.argtypes = [vp, vp, i32, i32, i32, i32, vp]
    lib.rt_debug_stt_dtw.argtypes = [vp, vp, i32, i32, i32, i32p]
    lib.rt_debug_stt_align_stages.argtypes = [vp, C.POINTER(vp), C.POINTER(i64), i32, i32, i32p, i32p, i32p, f32p, i64, f32p, i64, i32p, i32p, f32p]
    yield c
    c.close()


@pytest.fixture(scope="module")
def model(ctx):
    state = S.synthetic_state(CFG, 789)
    nat = S.NativeSTT(ctx, CFG, {k: v.cuda() for k, v in state.items()})
    yield nat, OW.build(CFG, state)
    nat.close()


@pytest.fixture(scope="module")
def clips(model):
    """The three clips of the model path, once: samples, the oracle's log-mel, 12 (or fewer) greedy ids, frames, and the oracle's W and
    log-probabilities."""
    _, oracle = model
    out = []
    for seconds, seed in ((0.6, 1), (1.3, 2), (2.0, 3)):
        x = clip(seconds, SR_IN, seed)
        x16 = OW.resample(x, SR_IN, CFG.sample_rate)
        mel = OW.log_mel(CFG, x16)
        ids, _ = OW.greedy(oracle, CFG, mel, 12)
        F = R.n_frames(CFG, len(x16))
        W, lp = R.model_pass(oracle, CFG, mel, ids, HEADS, F)
        out.append(dict(x=x, ids=ids, F=F, W=W, lp=lp))
    return out


def ints(v):
    return (C.c_int32 * max(len(v), 1))(*[int(t) for t in v])


def dtw(ctx, M, mode=-1):
    M = np.ascontiguousarray(M, dtype=np.float32)
    n, F = M.shape
    d = torch.from_numpy(M).cuda()
    out = (C.c_int32 * n)()
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rt_debug_stt_dtw(ctx.handle, d.data_ptr(), n, F, mode, out), "rt_debug_stt_dtw")
    return np.array(list(out), dtype=np.int64)


@pytest.mark.parametrize("n,F", [(1, 1), (1, 9), (9, 1), (13, 65), (40, 13), (300, 40), (3, 750), (449, 750)])
def test_dtw_equals_the_reference_on_planted_matrices(ctx, n, F):
    M, _ = R.planted_matrix(n, F, seed=7 * n + F)
    want = R.dtw_frames(M)
    got = dtw(ctx, M)
    assert np.array_equal(got, want), (n, F, np.flatnonzero(got != want)[:8])


def test_dtw_ties_and_both_homes_of_the_trace(ctx):
    flat = np.full((9, 17), 0.25, dtype=np.float32)            # all equal: every tie takes the "left" branch
    assert np.array_equal(dtw(ctx, flat), R.dtw_frames(flat))
    M, _ = R.planted_matrix(13, 65, seed=3)
    want = R.dtw_frames(M)
    assert np.array_equal(dtw(ctx, M, 0), want) and np.array_equal(dtw(ctx, M, 1), want)       # the trace in global memory / in LDS
    noisy = np.random.default_rng(5).standard_normal((31, 77)).astype(np.float32)              # no structure at all
    assert np.array_equal(dtw(ctx, noisy), R.dtw_frames(noisy))


def ulps(a, b):
    """Distance in float32 steps (both finite)."""
    def key(t):
        i = t.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i >= 0, i, -(i & 0x7fffffff))
    return (key(a) - key(b)).abs()


@pytest.mark.parametrize("heads,n,F,width", [(1, 2, 3, 7), (1, 2, 4, 7), (3, 13, 7, 7), (6, 40, 65, 7), (2, 5, 750, 7),
                                             (1, 5, 9, 1), (3, 13, 7, 1), (2, 9, 20, 3), (2, 9, 20, 31), (1, 4, 16, 31)])
def test_matrix_kernel_within_one_ulp(ctx, heads, n, F, width):
    g = torch.Generator().manual_seed(100 * heads + n + F + width)
    W = torch.rand((heads, n, F), generator=g) * 2.0 + torch.randn((heads, 1, F), generator=g)       # per-column std of order 1
    W[0, :, F // 2] = 0.375                                     # a constant column: z = 0 there
    d_W, d_M = W.cuda().contiguous(), torch.empty((n, F), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rt_debug_stt_align_matrix(ctx.handle, d_W.data_ptr(), heads, n, F, width, d_M.data_ptr()), "rt_debug_stt_align_matrix")
    got, want = d_M.cpu(), R.matrix(W, width)
    worst = int(ulps(got, want).max())
    print(f"matrix heads {heads} n {n} F {F} width {width}: max ulp {worst}, max |diff| {float((got - want).abs().max()):.3g}")
    assert torch.isfinite(got).all() and worst <= 1
    if heads == 1 and (F <= width // 2 or width == 1):          # (one head, nothing filtered: the column comes through as it is)
        assert torch.equal(got[:, F // 2], torch.zeros(n))


def split_planes(k):
    hi = k.to(torch.bfloat16)
    lo = (k - hi.float()).to(torch.bfloat16)
    return hi, lo


@pytest.mark.parametrize("d,n_ctx,F,rows", [(32, 100, 1, 1), (32, 100, 37, 13), (64, 100, 100, 13), (64, 1500, 37, 1), (32, 1500, 1500, 13), (64, 1500, 1, 13)])
def test_probabilities_kernel(ctx, d, n_ctx, F, rows):
    heads, slots, q_rows = 2, 2, rows + 3
    g = torch.Generator().manual_seed(d + n_ctx + F + rows)
    q = torch.randn((q_rows, heads, d), generator=g)
    hi, lo = split_planes(torch.randn((slots, heads, n_ctx, d), generator=g))
    k = hi.float() + lo.float()                                  # what the kernel reads: quantisation is not in the comparison
    src = [(3 * a + 1) % q_rows for a in range(rows)]
    ldw = F + 3                                                  # the cells behind a row's F frames are not the kernel's to write
    W = torch.full((heads, rows, ldw), -1.0, device="cuda")
    dq, dhi, dlo = q.cuda().contiguous(), hi.cuda().contiguous(), lo.cuda().contiguous()
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rt_debug_stt_align_probs(ctx.handle, dq.data_ptr(), q_rows, heads, d, dhi.data_ptr(), dlo.data_ptr(), slots, n_ctx, ints(src), ints([1] * rows),
                                               ints([F] * rows), rows, ints([1, 0]), 2, ldw, W.data_ptr()), "rt_debug_stt_align_probs")
    assert torch.equal(W[:, :, F:].cpu(), torch.full((heads, rows, 3), -1.0))
    got = W[:, :, :F].cpu()
    qs = q[src]                                                  # [rows][heads][d]; every row points at slot 1 of 2
    exact = torch.softmax(torch.einsum("rhd,htd->hrt", qs.double(), k[1].double()) / d ** 0.5, dim=-1)
    own = torch.softmax(torch.einsum("rhd,htd->hrt", qs, k[1]) / d ** 0.5, dim=-1)
    e_torch = float((own.double() - exact).abs().max())
    e_kernel = float((got.double() - exact[[1, 0]][:, :, :F]).abs().max())       # heads in the order given: 1, 0
    print(f"probs d {d} n_ctx {n_ctx} F {F} rows {rows}: kernel {e_kernel:.3g} torch float32 {e_torch:.3g}")
    assert e_kernel <= 4 * e_torch


def stages(ctx, nat, xs, ids):
    """rt_debug_stt_align_stages on windows xs with text ids: (W [n][heads][r_max][f_max], [M [n + 1][F] per window], frames, log-probabilities)"""
    pcm, n, ptrs, lens = nat._clips(xs)
    offs = [0]
    for t in ids:
        offs.append(offs[-1] + len(t))
    NH, w_cap, m_cap = len(HEADS), n * len(HEADS) * 32 * CFG.n_ctx, n * 32 * CFG.n_ctx
    h_W, h_M, shape = (C.c_float * w_cap)(), (C.c_float * m_cap)(), (C.c_int32 * 2)()
    fr, lp = (C.c_int32 * (offs[-1] + n))(), (C.c_float * max(offs[-1], 1))()
    ctx.check(ctx.lib.rt_debug_stt_align_stages(nat.handle, ptrs, lens, n, SR_IN, ints([t for w in ids for t in w]), ints(offs), None, h_W, w_cap, h_M, m_cap, shape, fr, lp),
              "rt_debug_stt_align_stages")
    r_max, f_max = shape[0], shape[1]
    W = torch.from_numpy(np.ctypeslib.as_array(h_W)[:n * NH * r_max * f_max].copy()).reshape(n, NH, r_max, f_max)
    flat, Ms, at = np.ctypeslib.as_array(h_M), [], 0
    for x, t in zip(pcm, ids):
        F = R.n_frames(CFG, -(-x.numel() * 2 // 3))                  # (24 kHz -> 16 kHz)
        Ms.append(flat[at:at + (len(t) + 1) * F].copy().reshape(len(t) + 1, F))
        at += (len(t) + 1) * F
    return W, Ms, list(fr), [float(v) for v in lp[:offs[-1]]]


def test_model_path_against_the_oracle(ctx, model, clips):
    nat, _ = model
    W, Ms, fr, lp = stages(ctx, nat, [c["x"] for c in clips], [c["ids"] for c in clips])
    e_w = e_lp = 0.0
    at = lat = 0
    for b, c in enumerate(clips):
        n, F = len(c["ids"]), c["F"]
        own = W[b, :, :n + 1, :F]
        e_w = max(e_w, float((own - c["W"]).abs().max()))
        e_lp = max(e_lp, float((torch.tensor(lp[lat:lat + n]) - c["lp"]).abs().max()))
        # the call's frames are the reference pipeline's on the call's OWN W (M is not compared on this path: with seeded weights the
        # per-column deviation is 1e-5 and smaller, which turns a 1e-5 relative difference of W into 1e-3 and more of M)
        assert fr[at:at + n + 1] == R.frames_from_weights(own, CFG.median_filter_width).tolist(), b
        assert Ms[b].shape == (n + 1, F) and np.isfinite(Ms[b]).all() and fr[at:at + n + 1] == R.dtw_frames(Ms[b]).tolist(), b    # ... and the path of its own M
        at += n + 1
        lat += n
    print(f"model path: max |W - oracle| {e_w:.3g} (recorded {MEASURED['W']:.3g}), max |logprob - oracle| {e_lp:.3g} (recorded {MEASURED['logprob']:.3g})")
    assert e_w <= 4 * MEASURED["W"] and e_lp <= 4 * MEASURED["logprob"]


def align(nat, xs, ids):
    t = nat.align_ids(xs, SR_IN, ids)
    return [(w.start, w.end, w.logprob, w.n_frames) for w in t]


def test_batch_invariance(model, clips):
    nat, _ = model
    xs, ids = [c["x"] for c in clips], [c["ids"] for c in clips]
    alone = [align(nat, [x], [t])[0] for x, t in zip(xs, ids)]
    assert align(nat, xs, ids) == alone
    assert align(nat, xs[::-1], ids[::-1]) == alone[::-1]
    assert [a[3] for a in alone] == [c["F"] for c in clips]
    many = align(nat, [xs[i % 3] for i in range(33)], [ids[i % 3] for i in range(33)])            # 33 windows: two groups
    assert many == [alone[i % 3] for i in range(33)]
    gap = align(nat, [xs[0], xs[1], xs[2]], [ids[0], [], ids[2]])                                     # a window with no ids between two with ids
    assert gap[0] == alone[0] and gap[2] == alone[2] and gap[1] == ([], [], [], clips[1]["F"])


def test_errors_leave_the_handle_usable(ctx, clips):
    state = S.synthetic_state(CFG, 789)
    nat = S.NativeSTT(ctx, dataclasses.replace(CFG, alignment_heads=()), {k: v.cuda() for k, v in state.items()})      # no rt_stt_set_alignment
    lib, c = ctx.lib, clips[0]
    try:
        def call(x, ids):
            pcm, n, ptrs, lens = nat._clips([x])
            out = S.RtSttAlignOut()
            fr = (C.c_int32 * (len(ids) + 1))()
            out.h_token_frame = fr
            return lib.rt_stt_align(nat.handle, ptrs, lens, 1, SR_IN, ints(ids), ints([0, len(ids)]), None, C.byref(out)), list(fr)

        def heads(pairs, width):
            return lib.rt_stt_set_alignment(nat.handle, ints([v for p in pairs for v in p]), len(pairs), width)

        assert call(c["x"], c["ids"])[0] == _native.RT_ERR_INVALID                                    # no alignment heads
        assert heads(HEADS, 6) == _native.RT_ERR_INVALID                                              # an even width
        assert heads([(1, 0), (1, 0)], 7) == _native.RT_ERR_INVALID                                  # a pair twice
        assert heads([(2, 0)], 7) == _native.RT_ERR_INVALID and heads([(1, 2)], 7) == _native.RT_ERR_INVALID
        assert call(c["x"], c["ids"])[0] == _native.RT_ERR_INVALID                                    # ... and none of them set anything
        assert heads(HEADS, 7) == _native.RT_OK
        want = call(c["x"], c["ids"])
        assert want[0] == _native.RT_OK and want[1] == R.frames_from_weights(stages(ctx, nat, [c["x"]], [c["ids"]])[0][0, :, :len(c["ids"]) + 1, :c["F"]], 7).tolist()
        for x, ids, rc in ((c["x"], [CFG.vocab], _native.RT_ERR_INVALID), (c["x"], [1, CFG.eos_id], _native.RT_ERR_INVALID), (c["x"], [1] * 29, _native.RT_ERR_LENGTH),
                           (np.zeros(2 * SR_IN + 1, dtype=np.float32), [1, 2], _native.RT_ERR_LENGTH)):
            assert call(x, ids)[0] == rc
            assert call(c["x"], c["ids"]) == want                                                     # after each error the handle aligns as before
    finally:
        nat.close()


def test_python_layer(ctx):
    cfg = SC.seek_test_config()
    x = clip(5.0, SR_IN, 2)                                      # 2-s windows: more than two of them
    tw = S.WhisperTranscriber(ctx, synthetic=True, cfg=cfg, timestamps=True, word_timestamps=True)
    tp = S.WhisperTranscriber(ctx, synthetic=True, cfg=cfg, timestamps=True)
    try:
        segs, plain = tw.batch_segments([x], SR_IN)[0], tp.batch_segments([x], SR_IN)[0]
        assert len(segs) >= 1 and all(g.words is None for g in plain)
        assert [dataclasses.replace(g, words=None) for g in segs] == plain
        clips_ = tw._seek([x], SR_IN)[0]
        tick, win = int(0.02 * SR_IN), cfg.chunk_seconds
        for g in segs:
            assert g.words is not None and [t for w in g.words for t in w.ids] == g.ids
            k = max(i for i, w in enumerate(clips_.windows) if w.offset // tick <= g.start_tick)
            lo = clips_.windows[k].offset / SR_IN
            times = [t for w in g.words for t in (w.start, w.end)]
            assert times == sorted(times) and all(lo <= t <= lo + win for t in times)
            assert all(0.0 < w.probability <= 1.0 and w.word == f"<{w.ids[0]}>" for w in g.words)
        ids = [[5, 9, 17], [3, 4]]
        xs = [x[:2 * SR_IN], x[SR_IN:3 * SR_IN]]
        words, times = tw.align(xs, SR_IN, ids), tw.model.align_ids(xs, SR_IN, ids)
        for ws, tt, t in zip(words, times, ids):
            assert [(w.start, w.end, w.ids) for w in ws] == [(s, e, [i]) for s, e, i in zip(tt.start, tt.end, t)]
    finally:
        tw.close()
        tp.close()


def test_words_under_a_detected_language(ctx):
    """language="auto": the windows of a clip are aligned under the language id the seek call detected for it, not the configured one."""
    cfg = SC.seek_test_config()
    x = clip(5.0, SR_IN, 2)
    ta = S.WhisperTranscriber(ctx, synthetic=True, cfg=cfg, language="auto", timestamps=True, word_timestamps=True)
    try:
        seen, inner = [], ta.model.align_ids

        def spy(windows, sample_rate, ids, languages=None):
            seen.append(languages)
            return inner(windows, sample_rate, ids, languages=languages)
        ta.model.align_ids = spy
        segs = ta.batch_segments([x], SR_IN)[0]
        assert all(g.words is not None and [t for w in g.words for t in w.ids] == g.ids for g in segs)
        detected = ta._seek([x], SR_IN)[0].language
        assert all(set(langs) == {detected} for langs in seen)
        # a clip as the seek call would report it, under a language that is not the configured one: one window, one segment
        lang = max(v for v in cfg.languages.values() if v != cfg.prefix[1])
        seg = S.SttSegment(0.0, 1.0, [5, 9, 17], 0, 50)
        made = S.SttSeekClip([5, 9, 17], 0.0, lang, 1.0, [seg], [S.SttSeekWindow(0, 5, 0.0, float("nan"), 100)])
        del seen[:]
        ta._fill_words([x], SR_IN, [made], [[seg]])
        assert seen == [[lang]]
        want = inner([x[:cfg.chunk_seconds * SR_IN]], SR_IN, [[5, 9, 17]], languages=[lang])[0]
        assert [(w.start, w.end, w.ids) for w in seg.words] == [(a, b, [t]) for a, b, t in zip(want.start, want.end, [5, 9, 17])]
        assert [w.probability for w in seg.words] == [float(np.exp(v)) for v in want.logprob] or \
            np.allclose([w.probability for w in seg.words], np.exp(want.logprob), rtol=1e-12)
    finally:
        ta.close()

"""k_stt_beam_select under the timestamp rule on its own (rt_debug_stt_beam_step_ts) against one step of the float64 restatement
(tests/stt_seek_ref.py step_row + tests/stt_beam_ref.py beam_step): tokens, parents and the rows' new history state exact, scores
within 4 E.  Inputs are built so that every ordering the step depends on, and every logsumexp decision, is at least 1e-3 apart in
float64 (the bound 4 E = 1.2e-4 is eight times below that).  The vocabulary of 400 is no multiple of the workgroup's 1024 threads."""
import ctypes as C

import numpy as np
import pytest
import torch

from rho_tts_amd import _native
from rho_tts_amd import stt as S
from tests import stt_beam_ref as R
from tests import stt_seek_cases as SC
from tests import stt_seek_ref as SR

pytestmark = pytest.mark.gpu

GAP = 1e-3
CFG = SC.seek_test_config()
T0, EOS, V = CFG.timestamp_begin, CFG.eos_id, CFG.vocab
# every shape of history behind the first step: one timestamp; timestamp + text; a closed pair; a pair followed by text; text and
# a timestamp that is closing a pair; a second pair
SHAPES = [[T0 + 7], [T0 + 7, 31], [T0 + 3, 31, T0 + 20, T0 + 20], [T0 + 3, 31, T0 + 20, T0 + 20, 44, 45], [T0, 12, 13, T0 + 50],
          [T0 + 1, 9, T0 + 5, T0 + 5, 8, T0 + 30, T0 + 30], [T0 + 2, 31, 32, 33]]


@pytest.fixture(scope="module")
def nat():
    ctx = _native.Context(0)
    m = S.NativeSTT(ctx, CFG, {k: v.cuda() for k, v in S.synthetic_state(CFG, 789).items()})
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    m.lib.rt_debug_stt_beam_step_ts.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, f32p, C.c_int32, C.c_int32, i32p, i32p, i32p, C.c_int32, C.c_int32,
                                                C.c_int32, i32p, i32p, i32p, i32p, f32p, i32p, i32p, f32p, i32p, i32p, i32p, i32p, i32p]
    yield m
    m.close()
    ctx.close()


def device_step(nat, logits, row_stride, scores, W, B, n_live, n_fin, first_step, max_initial, hists):
    d = torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)).cuda()
    torch.cuda.synchronize()
    n = W * B
    i32 = lambda a: (C.c_int32 * len(a))(*[int(v) for v in a])
    state = [SR.state_of(h, T0) for h in hists] + [(0, 0)] * (n - len(hists))
    sc = (C.c_float * n)(*[float(v) for v in np.asarray(scores, dtype=np.float32).reshape(-1)])
    tok, par, fb, fl, lt = (C.c_int32 * n)(), (C.c_int32 * n)(), (C.c_int32 * n)(), (C.c_int32 * n)(), (C.c_int32 * n)()
    so, fs = (C.c_float * n)(), (C.c_float * n)()
    nl, nf, dn, live = (C.c_int32 * W)(), (C.c_int32 * W)(), (C.c_int32 * W)(), C.c_int32()
    nat.ctx.check(nat.lib.rt_debug_stt_beam_step_ts(nat.handle, C.c_void_p(d.data_ptr()), row_stride, sc, W, B, i32(n_live), i32(n_fin), i32([0] * W),
                                                    int(first_step), 0 if first_step else 3, max_initial, i32([s[0] for s in state]), i32([s[1] for s in state]),
                                                    tok, par, so, nl, fb, fs, nf, dn, C.byref(live), fl, lt), "rt_debug_stt_beam_step_ts")
    return dict(tok=list(tok), par=list(par), score=list(so), n_live=list(nl), fin_beam=list(fb), fin_score=list(fs), n_fin=list(nf), done=list(dn),
                flags=list(fl), last=list(lt))


def reference(logits, scores, hists, B, n_fin, first_step, max_initial):
    """One window: (step, lse margins) with the rows masked by the restated rule."""
    never, begin = SR.suppress_mask(CFG)
    rows, lse = [], []
    for x, h in zip(logits, hists):
        y, m = SR.step_row(x, h, T0, EOS, never, begin, max_initial)
        rows.append(y)
        lse.append(m)
    return R.beam_step(np.stack(rows), np.asarray(scores, dtype=np.float64), B, EOS, np.zeros(V, dtype=bool), None, False, n_fin), lse


def check(nat, logits, scores, hists, B, n_live, n_fin=None, first_step=False, max_initial=-1):
    """logits [W][row_stride][V], scores [W][B], hists [W][n_live] -> the reference steps and margins, after holding the device to them."""
    logits = np.asarray(logits, dtype=np.float32)
    W, stride = logits.shape[:2]
    n_fin = n_fin or [0] * W
    scores = np.asarray(scores, dtype=np.float32).reshape(W, B)
    flat = [(hists[w][j] if j < n_live[w] else []) for w in range(W) for j in range(B)]
    got = device_step(nat, logits, stride, scores, W, B, n_live, n_fin, first_step, max_initial, flat)
    out = []
    for w in range(W):
        st, lse = reference(logits[w, :n_live[w]].astype(np.float64), scores[w, :n_live[w]], hists[w], B, n_fin[w], first_step, max_initial)
        assert all(g >= GAP for g in st.order_gaps) and all(abs(m) >= GAP for m in lse), (w, st.order_gaps, lse)
        nb = len(st.next)
        rows = slice(w * B, w * B + nb)
        assert got["n_live"][w] == nb and got["tok"][rows] == [t for t, _, _ in st.next], (w, got["tok"][rows], st.next)
        assert got["par"][rows] == [w * B + j for _, j, _ in st.next]
        err = np.abs(np.asarray(got["score"][rows]) - np.asarray([s for _, _, s in st.next]))
        assert err.max(initial=0.0) <= 4 * SC.E, err
        assert got["n_fin"][w] == st.n_fin and got["done"][w] == int(st.done)
        new = slice(w * B + n_fin[w], w * B + st.n_fin)
        assert got["fin_beam"][new] == [j for j, _ in st.finished]
        assert np.abs(np.asarray(got["fin_score"][new]) - np.asarray([s for _, s in st.finished])).max(initial=0.0) <= 4 * SC.E
        # the history state of every next beam is that of its parent's history with the token behind it
        want = [SR.state_of(hists[w][j] + [t], T0) for t, j, _ in st.next]
        assert list(zip(got["flags"][rows], got["last"][rows])) == want, (w, want)
        out.append((st, lse))
    return out


def planted(B, W, hists, seed, first_step=False, max_initial=-1, n_live=None):
    """Logits [W][B][V] within +-8 with planted leaders among text and timestamp ids and a per-row offset on the timestamp ids (so
    the logsumexp rule decides both ways), and descending incoming scores: the first seed from `seed` on whose step is decided by GAP."""
    for s in range(seed, seed + 300):
        rng = np.random.default_rng(s)
        n = 1 if first_step else B
        lg = rng.uniform(-8.0, 2.0, size=(W, n, V)).astype(np.float32)
        sc = np.sort(rng.uniform(-1.5, 0.0, size=(W, B)).astype(np.float32), axis=1)[:, ::-1].copy()
        for w in range(W):
            for j in range(n):
                lg[w, j, T0:] += (-5.0, 0.0, 8.0)[(w + j + s) % 3]
                ids = rng.choice(np.r_[np.arange(0, EOS + 1), np.arange(T0, V)], size=B + 5, replace=False)
                lg[w, j, ids] += (11.0 - 0.7 * np.arange(B + 5) + rng.uniform(-0.2, 0.2, size=B + 5)).astype(np.float32)
        try:
            for w in range(W):
                k = n_live[w] if n_live else n
                st, lse = reference(lg[w, :k].astype(np.float64), sc[w, :k], hists[w][:k], B, 0, first_step, max_initial)
                assert all(g >= GAP for g in st.order_gaps) and all(abs(m) >= GAP for m in lse) and len(st.next) == B
        except AssertionError:
            continue
        return lg, sc
    raise AssertionError("no seed gives a step decided by 1e-3")


@pytest.mark.parametrize("B", [1, 2, 5, 8])
def test_step_against_the_rule_over_every_history_shape(nat, B):
    W = max(2, -(-len(SHAPES) // B))
    W = min(W, 32 // B)
    hists = [[SHAPES[(w * B + j) % len(SHAPES)] for j in range(B)] for w in range(W)]
    lg, sc = planted(B, W, hists, 100 * B)
    res = check(nat, lg, sc, hists, B, [B] * W)
    lse = [m for _, ms in res for m in ms if np.isfinite(m)]
    if B * W >= len(SHAPES):
        assert any(m > 0 for m in lse) and any(m < 0 for m in lse)         # the logsumexp rule decides both ways
    if B > 1:                                                                # a step that permutes the beams, state and all
        assert any([j for _, j, _ in st.next] != sorted(j for _, j, _ in st.next) for st, _ in res)


def test_fewer_live_beams_and_a_partly_filled_list(nat):
    B, W = 5, 2
    hists = [[SHAPES[1], SHAPES[3], SHAPES[4]], [SHAPES[6], SHAPES[5]]]
    n_live = [3, 2]
    lg, sc = planted(B, W, hists, 7, n_live=n_live)
    check(nat, lg, sc, hists, B, n_live, n_fin=[2, 0])


def test_the_first_step_with_and_without_a_limit(nat):
    """Behind the prefix: one row per window, every text id barred - end-of-sequence and the largest text logits included - and with
    max_initial_timestamp_index 25 every timestamp above T0 + 25."""
    B, W = 3, 2
    lg, sc = planted(B, W, [[[]], [[]]], 40, first_step=True)
    lg[:, 0, 5] = 30.0
    lg[:, 0, EOS] = 29.0
    lg[:, 0, T0 - 1] = 31.0                                   # <|notimestamps|>
    lg[0, 0, T0 + 60], lg[0, 0, T0 + 25], lg[0, 0, T0 + 26] = 14.0, 12.5, 13.0
    sc[:] = 0.0
    free = check(nat, lg, sc, [[[]], [[]]], B, [1, 1], first_step=True, max_initial=-1)
    assert free[0][0].next[0][0] == T0 + 60 and all(t >= T0 for st, _ in free for t, _, _ in st.next)
    bound = check(nat, lg, sc, [[[]], [[]]], B, [1, 1], first_step=True, max_initial=25)
    assert bound[0][0].next[0][0] == T0 + 25 and all(T0 <= t <= T0 + 25 for st, _ in bound for t, _, _ in st.next)
    assert all(not st.finished for st, _ in free + bound)


def test_a_nan_logit_is_never_chosen_and_poisons_nothing(nat):
    B = 2
    hists = [[SHAPES[1], SHAPES[4]]]                           # text may follow | closing a pair: a timestamp or the end
    lg = np.full((1, B, V), -9.0, dtype=np.float32)
    lg[0, 0, [40, 41, 42, T0 + 30]] = [8.0, float("nan"), 6.0, 5.0]
    lg[0, 1, [T0 + 50, T0 + 60, T0 + 61, EOS, 17]] = [float("nan"), 7.0, 6.0, 6.5, 20.0]
    (st, lse), = check(nat, lg, [[-0.1, -0.2]], hists, B, [B])
    toks = [t for t, _, _ in st.next]
    assert 41 not in toks and T0 + 50 not in toks and 17 not in toks and np.isfinite([s for _, _, s in st.next]).all()
    assert lse[0] < 0 < lse[1]

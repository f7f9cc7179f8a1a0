"""The two kernels of the speech-to-text beam search on their own: k_stt_beam_select on supplied logits (rt_debug_stt_beam_step)
against one step of the float64 rule (tests/stt_beam_ref.py beam_step) - ids and parents exact, scores within 1e-5 - and the KV
reorder (rt_debug_stt_beam_reorder) on a cache filled with a recognisable pattern.

Inputs are built so that every ordering the step depends on - consecutive candidates the walk consumes, and the last of them against
the first left out - is at least 1e-3 apart in float64 (float32 log-softmax of logits within +-16 over <= 51865 terms with a tree
reduction is good to a few 1e-6: two orders of magnitude), except for the exact ties placed on purpose."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from rho_tts_amd import _native
from rho_tts_amd import stt as S
from tests import stt_beam_ref as R

pytestmark = pytest.mark.gpu

GAP = 1e-3
TOL = 1e-5


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def config(V):
    base = S.tiny_test_config()
    if V == base.vocab:
        return base
    if V == 51865:
        eos = 50257
        return dataclasses.replace(base, vocab=V, eos_id=eos, prefix=(eos + 1, eos + 2, eos + 3), suppress_from=eos, begin_suppress=(220, eos))
    # any other size: end-of-sequence in the middle and a few suppressed ids, so that the last id of the vocabulary can be chosen
    eos = V // 2
    return dataclasses.replace(base, vocab=V, eos_id=eos, prefix=(eos + 1, eos + 2, eos + 3), suppress_from=0, begin_suppress=(7, eos),
                               suppress_tokens=(eos + 1, eos + 2, eos + 3))


@pytest.fixture(scope="module")
def models(ctx):
    made = {}

    def get(V):
        if V not in made:
            cfg = config(V)
            made[V] = (cfg, S.NativeSTT(ctx, cfg, {k: v.cuda() for k, v in S.synthetic_state(cfg, 789).items()}))
        return made[V]
    yield get
    for _, nat in made.values():
        nat.close()


def declare(lib):
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    lib.rt_debug_stt_beam_step.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, f32p, C.c_int32, C.c_int32, i32p, i32p, i32p, C.c_int32, C.c_int32,
                                           i32p, i32p, f32p, i32p, i32p, f32p, i32p, i32p, i32p]
    lib.rt_debug_stt_beam_reorder.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, i32p, C.c_int32, C.POINTER(C.c_uint16)]


def device_step(nat, logits, row_stride, scores, W, B, n_live, n_fin, done, first_step, step=3):
    """logits [W][row_stride][V] float32, scores [W][B]."""
    declare(nat.lib)
    d = torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)).cuda()
    torch.cuda.synchronize()
    R_ = W * B
    i32 = lambda a: (C.c_int32 * len(a))(*[int(v) for v in a])
    sc = (C.c_float * R_)(*[float(v) for v in np.asarray(scores, dtype=np.float32).reshape(-1)])
    tok, par, fb = (C.c_int32 * R_)(), (C.c_int32 * R_)(), (C.c_int32 * R_)()
    so, fs = (C.c_float * R_)(), (C.c_float * R_)()
    nl, nf, dn, live = (C.c_int32 * W)(), (C.c_int32 * W)(), (C.c_int32 * W)(), C.c_int32()
    nat.ctx.check(nat.lib.rt_debug_stt_beam_step(nat.handle, C.c_void_p(d.data_ptr()), row_stride, sc, W, B, i32(n_live), i32(n_fin), i32(done),
                                                 int(first_step), step, tok, par, so, nl, fb, fs, nf, dn, C.byref(live)), "rt_debug_stt_beam_step")
    return dict(tok=list(tok), par=list(par), score=list(so), n_live=list(nl), fin_beam=list(fb), fin_score=list(fs), n_fin=list(nf), done=list(dn),
                live=live.value)


def check(nat, cfg, logits, scores, B, n_live, n_fin=None, done=None, first_step=False, row_stride=None, ties=0):
    """Every window of `logits` [W][row_stride][V] through the device step and through beam_step.  Returns the reference steps."""
    logits = np.asarray(logits, dtype=np.float32)
    W = logits.shape[0]
    row_stride = row_stride or B
    n_fin = n_fin or [0] * W
    done = done or [0] * W
    scores = np.asarray(scores, dtype=np.float32).reshape(W, B)
    got = device_step(nat, logits, row_stride, scores, W, B, n_live, n_fin, done, first_step)
    never, begin = R.masks(cfg)
    steps, seen_ties = [], 0
    for w in range(W):
        rows = slice(w * B, (w + 1) * B)
        if done[w]:                                            # a completed window rides along untouched
            assert got["tok"][rows] == [-1] * B and got["par"][rows] == [-1] * B and got["done"][w] == 1 and got["n_fin"][w] == n_fin[w]
            assert got["score"][rows] == [float(v) for v in scores[w]]
            steps.append(None)
            continue
        st = R.beam_step(logits[w, :n_live[w]].astype(np.float64), scores[w, :n_live[w]].astype(np.float64), B, cfg.eos_id, never, begin, first_step, n_fin[w])
        steps.append(st)
        seen_ties += sum(1 for g in st.order_gaps if g == 0.0)
        assert all(g == 0.0 or g >= GAP for g in st.order_gaps), (w, st.order_gaps)     # the inputs decide everything by >= 1e-3
        nb = len(st.next)
        assert got["n_live"][w] == nb
        assert got["tok"][w * B:w * B + nb] == [t for t, _, _ in st.next], w
        assert got["par"][w * B:w * B + nb] == [w * B + j for _, j, _ in st.next], w
        assert got["par"][w * B + nb:(w + 1) * B] == list(range(w * B + nb, (w + 1) * B))
        np.testing.assert_allclose(got["score"][w * B:w * B + nb], [s for _, _, s in st.next], rtol=0, atol=TOL)
        assert got["n_fin"][w] == st.n_fin and got["done"][w] == int(st.done)
        new = slice(w * B + n_fin[w], w * B + st.n_fin)
        assert got["fin_beam"][new] == [j for j, _ in st.finished], w
        np.testing.assert_allclose(got["fin_score"][new], [s for _, s in st.finished], rtol=0, atol=TOL)
    assert seen_ties == ties
    assert got["live"] == sum(1 for w in range(W) if not done[w]) - sum(1 for w in range(W) if not done[w] and steps[w].done)
    return steps


def planted(cfg, B, W, seed, n_live=None, eos_rank=None):
    """Logits [W][B][V] within +-16 with a dozen planted leaders per row, and incoming scores, every decision >= 1e-3 apart: the
    first seed from `seed` on that gives such a step (checked again by `check`)."""
    V = cfg.vocab
    never, begin = R.masks(cfg)
    allowed = np.flatnonzero(~never & (np.arange(V) != cfg.eos_id))
    for s in range(seed, seed + 200):
        rng = np.random.default_rng(s)
        lg = rng.uniform(-8.0, 2.0, size=(W, B, V)).astype(np.float32)
        sc = np.sort(rng.uniform(-3.0, 0.0, size=(W, B)).astype(np.float32), axis=1)[:, ::-1].copy()
        for w in range(W):
            for j in range(B):
                ids = rng.choice(allowed, size=B + 4, replace=False)
                if eos_rank is not None and (w + j) % 2 == 0:
                    ids[min(eos_rank, B + 3)] = cfg.eos_id
                lg[w, j, ids] = (13.0 - 0.61 * np.arange(B + 4) + rng.uniform(-0.2, 0.2, size=B + 4)).astype(np.float32)
        live = n_live or [B] * W
        ok = True
        for w in range(W):
            st = R.beam_step(lg[w, :live[w]].astype(np.float64), sc[w, :live[w]].astype(np.float64), B, cfg.eos_id, never, begin, False, 0)
            ok = ok and all(g >= GAP for g in st.order_gaps)
        if ok:
            return lg, sc
    raise AssertionError("no seed gives a step decided by 1e-3")


@pytest.mark.parametrize("V,B,W", [(300, 3, 2), (300, 1, 1), (51865, 5, 3), (51865, 8, 4), (1025, 4, 2)])
def test_step_against_the_rule(models, V, B, W):
    """V = 1025 is one element past the workgroup's stride of 1024; 51865 x 8 x 4 fills the group's 32 rows."""
    cfg, nat = models(V)
    lg, sc = planted(cfg, B, W, 10 * B + W, eos_rank=1)
    if V == 1025:
        lg[0, 0, 1024] = 15.5                                  # the lone element of the last stride leads its row
    steps = check(nat, cfg, lg, sc, B, [B] * W)
    assert any(st.finished for st in steps) or B == 1
    if V == 1025:
        assert 1024 in [t for t, _, _ in steps[0].next]
    # a window with fewer live beams than B, a finished list that is partly filled, and a later step
    if B > 1:
        n_live = [max(1, B - 1 - (w % 2)) for w in range(W)]
        lg2, sc2 = planted(cfg, B, W, 1000 + 10 * B + W, n_live=n_live, eos_rank=0)
        check(nat, cfg, lg2, sc2, B, n_live, n_fin=[(B - 1) if w == 0 else 0 for w in range(W)])


def test_first_step_has_one_row_per_window_and_its_own_mask(models):
    """The step behind the prefix: logits [W][1][V] (row_stride 1), one live beam of score 0; the begin-suppressed ids (7 and
    end-of-sequence) hold the two largest logits and are not chosen - the same logits at a later step choose them."""
    cfg, nat = models(300)
    B, W = 3, 2
    lg, _ = planted(cfg, 1, W, 77)
    lg = lg.reshape(W, 1, cfg.vocab)
    lg[:, 0, 7] = 15.0
    lg[:, 0, cfg.eos_id] = 14.0
    sc = np.zeros((W, B), dtype=np.float32)
    first = check(nat, cfg, lg, sc, B, [1] * W, first_step=True, row_stride=1)
    assert all(7 not in [t for t, _, _ in st.next] and not st.finished and len(st.next) == B for st in first)
    later = check(nat, cfg, lg, sc, B, [1] * W, first_step=False, row_stride=1)
    assert all(st.next[0][0] == 7 and len(st.finished) == 1 for st in later)


def hand_rows(cfg, B, rows):
    """Logits [1][B][V]: a floor of -9 and the given {id: value} per row."""
    lg = np.full((1, B, cfg.vocab), -9.0, dtype=np.float32)
    for j, row in enumerate(rows):
        for t, v in row.items():
            lg[0, j, t] = v
    return lg


def test_walk_cases(models):
    cfg, nat = models(300)
    eos, B = cfg.eos_id, 3
    # (a) a row whose best candidate is end-of-sequence; (b) all B + 1 candidates of row 0 land in the consumed part of the walk
    # (its lead is larger than its spread, and end-of-sequence is among them, so the walk needs B + 1 candidates for B beams)
    lg = hand_rows(cfg, B, [{eos: 9.0, 11: 8.0, 12: 7.5, 13: 7.0, 14: 1.0}, {21: 9.0, 22: 8.0, 23: 7.0, 24: 6.0}, {31: 9.0, 32: 8.0, 33: 7.0, 34: 6.0}])
    st = check(nat, cfg, lg, [[0.0, -6.0, -7.0]], B, [B])[0]
    assert st.finished and st.finished[0][0] == 0 and [j for _, j, _ in st.next] == [0, 0, 0] and [t for t, _, _ in st.next] == [11, 12, 13]
    # (c) masked ids hold the largest raw logits (never-ids sit behind end-of-sequence); (d) a NaN logit is never chosen and does not
    # poison the row's log-sum-exp
    lg = hand_rows(cfg, B, [{295: 15.0, 296: 14.0, 41: 6.0, 42: 5.0, 43: 4.0, 44: 3.0}, {51: 6.5, 52: 5.5, 53: float("nan"), 54: 3.5, 55: 2.5},
                            {61: 6.2, 62: 5.2, 63: 4.2, 64: 3.2}])
    st = check(nat, cfg, lg, [[-1.0, -1.1, -1.25]], B, [B])[0]
    assert not {295, 296, 53} & {t for t, _, _ in st.next}
    # (e) the finished list fills up in the middle of a step: two slots left, three end-of-sequence candidates in the walk
    lg = hand_rows(cfg, B, [{eos: 9.0, 11: 2.0, 12: 1.0, 13: 0.5}, {eos: 9.0, 21: 2.0, 22: 1.0, 23: 0.5}, {eos: 9.0, 31: 8.7, 32: 8.3, 33: 8.0}])
    st = check(nat, cfg, lg, [[-0.5, -0.7, -0.9]], B, [B], n_fin=[1])[0]
    assert [j for j, _ in st.finished] == [0, 1] and st.done


def test_exact_ties_go_to_the_lower_beam_then_the_lower_id(models):
    cfg, nat = models(300)
    B = 2
    # two equal logits in one row: the lower id first
    lg = hand_rows(cfg, B, [{40: 8.0, 17: 8.0, 60: 3.0}, {70: 7.0, 71: 6.0, 72: 2.0}])
    st = check(nat, cfg, lg, [[-0.25, -4.0]], B, [B], ties=1)[0]
    assert [t for t, _, _ in st.next] == [17, 40]
    # two bit-identical rows with equal incoming scores: the lower beam first, and the walk stops before the higher beam's twin
    row = {90: 8.0, 91: 6.0, 92: 2.0}
    lg = hand_rows(cfg, B, [row, row])
    st = check(nat, cfg, lg, [[-0.5, -0.5]], B, [B], ties=1)[0]
    assert [(t, j) for t, j, _ in st.next] == [(90, 0), (90, 1)]
    B = 3
    lg = hand_rows(cfg, B, [row, row, {95: 8.0, 96: 7.0, 97: 6.0, 98: 5.0}])
    st = check(nat, cfg, lg, [[-0.5, -0.5, -9.0]], B, [B], ties=2)[0]        # (90: beams 0 and 1; 91: the walk's last and the first left out)
    assert [(t, j) for t, j, _ in st.next] == [(90, 0), (90, 1), (91, 0)]


def test_a_completed_window_rides_beside_a_live_one(models):
    cfg, nat = models(300)
    B, W = 3, 3
    lg, sc = planted(cfg, B, W, 5, eos_rank=2)
    steps = check(nat, cfg, lg, sc, B, [B] * W, n_fin=[0, B, 1], done=[0, 1, 0])
    assert steps[1] is None and steps[0] is not None and steps[2] is not None


@pytest.mark.parametrize("src,length", [([1, 0, 2], 5), ([0, 0, 0], 7), ([0, 1, 2], 3), ([2, 2, 0], 0)])
def test_reorder(ctx, src, length):
    """A swap, a fan-out, the identity (and nothing to copy): over 2 layers x 2 heads every plane of row r holds its parent's
    pattern at positions [0, len) and the destination's sentinel behind them."""
    lib = ctx.lib
    declare(lib)
    L, rows, H, P, d = 2, 3, 2, 9, 32
    n = L * rows * H * P * d
    out = (C.c_uint16 * (8 * n))()
    ctx.check(lib.rt_debug_stt_beam_reorder(ctx.handle, L, rows, H, P, d, (C.c_int32 * rows)(*src), length, out), "rt_debug_stt_beam_reorder")
    got = np.frombuffer(out, dtype=np.uint16).reshape(2, 4, L, rows, H, P, d)
    i = np.arange(n, dtype=np.int64)
    pattern = np.stack([((i * 40503 + q * 12289) & 0x7fff).astype(np.uint16) for q in range(4)]).reshape(4, L, rows, H, P, d)
    assert np.array_equal(got[0], pattern)                     # the source cache is left as it was
    want = np.full_like(pattern, 0xbeef)
    for r, parent in enumerate(src):
        want[:, :, r, :, :length] = pattern[:, :, parent, :, :length]
    assert np.array_equal(got[1], want)

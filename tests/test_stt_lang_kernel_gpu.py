"""k_stt_probe on its own (rt_debug_stt_probe): the same float32 logits to the kernel and to the float64 rule (tests/stt_lang_ref.py
probe).  The language id must be exact; the two log-probabilities agree within 1e-5 absolute - a fixed-order float32 sum of at most
51865 exponentials is good to about log2(V) 2^-24 = 1e-6, which leaves a factor of ten.

Random rows keep the two largest language logits at least 1e-3 apart (float32 compares the very numbers the rule sees, so any gap
would do; the gap keeps the case honest should the kernel ever compare something derived).  Three rows are special: two equal
language maxima (the lowest id wins), a NaN on a language id (it never wins, and takes no part in the sums), and -inf everywhere but
on one language (probability 1, no-speech probability 0)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from rho_tts_amd import _native
from rho_tts_amd import stt as S
from tests import stt_lang_ref as LR

pytestmark = pytest.mark.gpu

TOL = 1e-5


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def config(V, n_lang):
    """The smallest model over a vocabulary of V with n_lang language ids behind start-of-transcript, Whisper's order of specials."""
    eos = 50257 if V == 51865 else 150
    sot, first = eos + 1, eos + 2
    langs = {f"l{i}": first + i for i in range(n_lang)}
    tr = first + n_lang
    return dataclasses.replace(S.tiny_test_config(), vocab=V, eos_id=eos, prefix=(sot, first, tr, tr + 2), suppress_from=eos, begin_suppress=(7, eos),
                               languages=langs, no_speech_id=tr + 1, language="l0")


@pytest.fixture(scope="module")
def models(ctx):
    made = {}

    def get(V, n_lang):
        if (V, n_lang) not in made:
            cfg = config(V, n_lang)
            made[V, n_lang] = (cfg, S.NativeSTT(ctx, cfg, {k: v.cuda() for k, v in S.synthetic_state(cfg, 789).items()}))
        return made[V, n_lang]
    yield get
    for _, nat in made.values():
        nat.close()


def device_probe(nat, logits):
    lib = nat.lib
    lib.rt_debug_stt_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    d = torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)).cuda()
    torch.cuda.synchronize()
    n = logits.shape[0]
    lang, prob, ns = (C.c_int32 * n)(), (C.c_float * n)(), (C.c_float * n)()
    nat.ctx.check(lib.rt_debug_stt_probe(nat.handle, C.c_void_p(d.data_ptr()), logits.shape[1], n, lang, prob, ns), "rt_debug_stt_probe")
    return list(lang), np.array(prob, dtype=np.float64), np.array(ns, dtype=np.float64)


def random_rows(rng, rows, V, ids):
    z = rng.uniform(-20.0, 20.0, size=(rows, V)).astype(np.float32)
    for r in range(rows):                        # the two largest language logits at least 1e-3 apart
        order = np.argsort(z[r, ids])
        if z[r, ids[order[-1]]] - z[r, ids[order[-2]]] < 1e-3:
            z[r, ids[order[-1]]] += np.float32(1e-2)
    return z


def log_err(got_p, want_log):
    """|log got - want| with -inf == log 0."""
    with np.errstate(divide="ignore"):
        got = np.log(got_p)
    if np.isinf(want_log) or np.isinf(got):
        return 0.0 if got == want_log else np.inf
    return abs(got - want_log)


@pytest.mark.parametrize("V", [300, 51865])
@pytest.mark.parametrize("n_lang", [4, 99])
@pytest.mark.parametrize("rows", [1, 5])
def test_probe_against_the_float64_rule(models, V, n_lang, rows):
    cfg, nat = models(V, n_lang)
    ids = sorted(cfg.languages.values())
    rng = np.random.default_rng(1000 * rows + n_lang + V)
    z = random_rows(rng, rows, V, ids)
    lang, prob, ns = device_probe(nat, z)
    worst = 0.0
    for r in range(rows):
        want = LR.probe(z[r], ids, cfg.no_speech_id)
        assert lang[r] == want.language, (r, lang[r], want.language)
        worst = max(worst, log_err(prob[r], want.log_language_prob), log_err(ns[r], want.log_no_speech_prob))
    print(f"V={V} languages={n_lang} rows={rows}: max |log p - float64| {worst:.3g} (bound {TOL})")
    assert worst <= TOL
    if rows > 1:                                 # a row's three results do not depend on what it is batched with, nor on the stride
        wide = np.zeros((rows, V + 37), dtype=np.float32)
        wide[:, :V] = z
        assert all(np.array_equal(a, b) for a, b in zip(device_probe(nat, wide), (lang, prob, ns)))
        for r in (0, rows - 1):
            l1, p1, n1 = device_probe(nat, z[r:r + 1])
            assert (l1[0], p1[0], n1[0]) == (lang[r], prob[r], ns[r])


@pytest.mark.parametrize("V", [300, 51865])
@pytest.mark.parametrize("n_lang", [4, 99])
def test_special_rows(models, V, n_lang):
    cfg, nat = models(V, n_lang)
    ids = sorted(cfg.languages.values())
    rng = np.random.default_rng(7 + V + n_lang)
    z = random_rows(rng, 3, V, ids)
    z[0, ids] = np.minimum(z[0, ids], np.float32(10.0))
    z[0, [ids[1], ids[-1]]] = np.float32(12.5)                   # two equal maxima: the lowest id wins
    top = ids[int(np.argmax(z[1, ids]))]
    z[1, top] = np.nan                                           # a NaN on what was the winner: it never wins
    z[2, :] = -np.inf
    z[2, ids[2]] = np.float32(-3.25)                             # -inf everywhere but on one language
    lang, prob, ns = device_probe(nat, z)
    want = [LR.probe(z[r], ids, cfg.no_speech_id) for r in range(3)]
    assert lang == [w.language for w in want]
    assert lang[0] == ids[1] and lang[1] != top and lang[2] == ids[2]
    assert prob[2] == 1.0 and ns[2] == 0.0 and want[2].log_language_prob == 0.0 and want[2].log_no_speech_prob == -np.inf
    worst = max(max(log_err(prob[r], want[r].log_language_prob), log_err(ns[r], want[r].log_no_speech_prob)) for r in range(3))
    print(f"V={V} languages={n_lang} special rows: max |log p - float64| {worst:.3g} (bound {TOL})")
    assert np.isfinite(prob).all() and np.isfinite(ns).all() and worst <= TOL


def test_arguments(models):
    cfg, nat = models(300, 4)
    lib = nat.lib
    z = np.zeros((2, 300), dtype=np.float32)
    device_probe(nat, z)
    d = torch.zeros(2, 300, device="cuda")
    lang, prob, ns = (C.c_int32 * 40)(), (C.c_float * 40)(), (C.c_float * 40)()
    for stride, n in ((299, 1), (300, 0), (300, 33)):
        assert lib.rt_debug_stt_probe(nat.handle, C.c_void_p(d.data_ptr()), stride, n, lang, prob, ns) == _native.RT_ERR_INVALID
    assert lib.rt_debug_stt_probe(nat.handle, None, 300, 1, lang, prob, ns) == _native.RT_ERR_INVALID
    assert device_probe(nat, z)[0] == [min(cfg.languages.values())] * 2          # equal logits: the lowest id; the handle is usable

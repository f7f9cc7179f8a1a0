"""CPU checks of tests/sampling_ref.py and of the inputs of tests/test_sampler_frame_gpu.py: draw_decided draws what
oracle/sampling.py draws, the random stream reads the low half of an item id, the inputs leave fewer draws undecided than the cap
allows, and the reference alone tells the sampler's keys and its history apart on them."""
import numpy as np
import pytest

from tests import sampler_frame_cases as K
from tests.sampling_ref import CAP, DECIDED, SamplingParams, draw, draw_decided, uniform


@pytest.mark.parametrize("V,sup_from", [(3072, 2048), (1000, 640), (700, 690), (6000, 5000)])
def test_draw_decided_draws_what_the_oracle_draws(V, sup_from):
    logits, seen = K.corner_logits(V, sup_from)
    allow = min(V - 1, sup_from + 102)
    sup = np.zeros(V, bool)
    sup[sup_from:] = True
    sup[allow] = False
    cases = [K.GREEDY, K.SP_A, K.SP_B, K.TOP1, SamplingParams(True, 1.0, 5, 0.3, 1.2)]
    for sp in cases:
        for r in range(logits.shape[0]):
            u = uniform(K.SEED, r, 7, 3)
            tok, margin = draw_decided(logits[r].numpy(), sp, u, sup, seen[r].numpy())
            assert tok == draw(logits[r].numpy(), sp, u, sup, seen[r].numpy()), (sp, r)
            assert margin >= 0
            if not sp.do_sample or sp.top_k == 1 or r == 8:            # greedy, one candidate, one finite value
                assert margin == np.inf, (sp, r)


def test_margin_is_the_distance_to_the_nearest_boundary():
    """Two candidates with p = (1, 1): cum = (1, 2), target = 2 u: the margin is min(|1 - 2 u|, |2 - 2 u|) / 2; a top-p limit of
    exactly 1 = cum[0] has margin 0."""
    lg = np.array([0.0, 0.0, -np.inf], np.float32)
    sp = SamplingParams(True, 1.0, 2, 1.0, 1.0)
    for u in (np.float32(0.25), np.float32(0.5), np.float32(0.75), np.float32(0.5 + 2.0 ** -22)):
        tok, margin = draw_decided(lg, sp, u)
        assert tok == draw(lg, sp, u) == (0 if u < 0.5 else 1)
        assert margin == min(abs(1 - 2 * float(u)), abs(2 - 2 * float(u))) / 2
    assert draw_decided(lg, sp, np.float32(0.5 + 2.0 ** -22))[1] < DECIDED <= draw_decided(lg, sp, np.float32(0.5 + 2.0 ** -19))[1]
    assert draw_decided(lg, SamplingParams(True, 1.0, 2, 0.5, 1.0), np.float32(0.3))[1] == 0.0


def test_the_random_stream_reads_the_low_half_of_the_item_id():
    for item in (0, 7, 2 ** 31 + 3, 5):
        for frame, group in ((0, 0), (5, 3)):
            assert uniform(K.SEED, item + 2 ** 32, frame, group) == uniform(K.SEED, item, frame, group)
    assert uniform(K.SEED, 2 ** 31 + 3, 1, 0) != uniform(K.SEED, 3, 1, 0)
    assert uniform(K.SEED, 7, 1, 0) != uniform(K.SEED & 0xFFFFFFFF, 7, 1, 0)          # the seed's high half counts


def _share(margins):
    return sum(1 for m in margins if m < DECIDED) / len(margins)


@pytest.mark.parametrize("V,n_slabs", K.SLAB_CASES)
def test_undecided_share_of_the_slab_inputs(V, n_slabs):
    sup, eos = K.layout(V)
    _, logits = K.slab_case(V, n_slabs)
    margins = []
    for sp in (K.SP_A, K.SP_B):
        for frame in (0, 1, 5):
            margins += K.reference(logits, sp, frame, K.frame_offsets(frame), 0, sup, eos, 1, 2)[1]
    assert _share(margins) <= CAP, _share(margins)


@pytest.mark.parametrize("V", [700, 3072])
def test_frame_item_and_group_keys_show_on_the_slab_inputs(V):
    """A sampler keyed by the global frame, by the row instead of the item id, by the whole 64-bit id's other half or by another
    group draws other tokens on these inputs: decided draws differ."""
    sup, eos = K.layout(V)
    _, logits = K.slab_case(V, 1)
    frame, off = 5, K.frame_offsets(5)
    base = K.reference(logits, K.SP_A, frame, off, 2, sup, eos, 0, 2)

    def differs(other):
        return any(m >= DECIDED and a != b for a, b, m in zip(base[0], other[0], base[1]))
    assert differs(K.reference(logits, K.SP_A, frame, 0 * off, 2, sup, eos, 0, 2))                        # global frame
    assert differs(K.reference(logits, K.SP_A, frame, off, 3, sup, eos, 0, 2))                            # group + 1
    assert differs(K.reference(logits, K.SP_A, frame, off, 2, sup, eos, 0, 2, items=list(range(K.M))))    # row, not item id
    assert differs(K.reference(logits, K.SP_A, frame, off, 2, sup, eos, 0, 2, seed=K.SEED & 0xFFFFFFFF))  # seed's low half alone


def test_penalty_history_shows_on_the_integer_inputs():
    """Three frames on the same integer logits: tokens repeat, and a sampler that forgets the history draws other tokens."""
    V = 700
    sup, eos = K.layout(V)
    logits = K.integer_case(V)
    for sp in (K.SP_B, SamplingParams(True, 0.9, 50, 1.0, 1.3)):
        seen = np.zeros((K.M, V), bool)
        import torch
        seen = torch.from_numpy(seen)
        changed, margins = 0, []
        for frame in range(3):
            toks, mar, _, _, after = K.reference(logits, sp, frame, [0] * K.M, 0, sup, eos, 0, 2, seen=seen)
            blank = K.reference(logits, sp, frame, [0] * K.M, 0, sup, eos, 0, 2, seen=torch.zeros_like(seen))[0]
            changed += sum(1 for a, b, m in zip(toks, blank, mar) if m >= DECIDED and a != b)
            margins += mar
            seen = after
        assert changed >= 1, sp
        assert _share(margins) <= CAP


@pytest.mark.parametrize("V,H", K.EMBED_CASES)
def test_undecided_share_of_the_embedding_inputs(V, H):
    _, logits = K.slab_case(V, 1, seed=H)
    margins = K.reference(logits, K.SP_A, 1, K.frame_offsets(1), 1, V, -1, 0, 0)[1]
    assert _share(margins) <= CAP

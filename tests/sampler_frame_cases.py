"""Inputs and the CPU reference of tests/test_sampler_frame_gpu.py (the sampler launch in the decode loop's form), shared with
tests/test_sampling_ref_cpu.py, which shows on the CPU that these inputs leave fewer draws undecided than the cap allows."""
import numpy as np
import torch

from tests.sampling_ref import SamplingParams, draw_decided, uniform

M, NF = 24, 6                                  # rows of a launch, frames every frame-strided buffer holds
SEED = 789 + (5 << 32)                         # (a non-zero high half)
ITEMS = [0, 7, 2 ** 31 + 3, 2 ** 32 + 5] + [11 * r + 1 for r in range(4, M)]
SP_A = SamplingParams(True, 0.9, 50, 1.0, 1.05)
SP_B = SamplingParams(True, 1.3, 64, 0.8, 1.3)
GREEDY = SamplingParams(False)
TOP1 = SamplingParams(True, 0.7, 1, 1.0, 1.0)
SLAB_CASES = [(V, n) for V in (700, 2048, 3072, 6000) for n in (1, 3)]
EMBED_CASES = [(64, 64), (256, 256), (2048, 1024), (700, 2080)]
TABLE_CASES = [(64, 64, 128), (2048, 1024, 4096), (700, 2080, 2060)]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def corner_logits(V, sup_from, rows=M):
    """The rows of test_sampler_matches_oracle_draw_for_draw (tests/test_kernels_gpu.py): ties at the top, all equal, ties across
    the top-k cut, integer logits, fewer finite values than k, one finite value, the top-k in the last waves / in one wave."""
    g = gen(31 + V)
    logits = torch.randn(rows, V, generator=g) * 2.0
    logits[3, 100] = logits[3, 200] = float(logits[3].max()) + 1.0
    logits[4, :] = 0.5
    logits[5] = torch.round(logits[5] * 4) / 4
    logits[6] = torch.round(logits[6])
    logits[7, : sup_from - 7] = float("-inf")
    logits[8, :] = float("-inf"); logits[8, 17] = 0.25
    logits[9, sup_from - 40: sup_from] += 9.0
    logits[10, :64] += 9.0; logits[10, :64] = torch.round(logits[10, :64])
    seen = torch.rand(rows, V, generator=g) < 0.05
    return logits, seen


def layout(V):
    """(suppress_from, end-of-sequence id): the id lies above suppress_from, as the codec's control ids do."""
    sup = V - V // 8
    return sup, sup + 5


def slab_case(V, n_slabs, seed=0):
    """slabs [n_slabs][M][V] whose float32 sum in slab order (the reference's logits) is about 2 * randn; in every third row the
    end-of-sequence id carries the largest logit (40, exactly: slab 0 holds it, the others hold 0 there)."""
    sup, eos = layout(V)
    slabs = torch.randn(n_slabs, M, V, generator=gen(1000 + V + n_slabs + seed)) * (2.0 / n_slabs ** 0.5)
    slabs[:, ::3, eos] = 0.0
    slabs[0, ::3, eos] = 40.0
    return slabs, sum_slabs(slabs)


def sum_slabs(slabs):
    l = torch.zeros_like(slabs[0])
    for s in slabs:
        l = l + s                                  # float32, slab order, starting from 0
    return l


def integer_case(V, seed=0):
    """Row 6 of the kernel test on every row: logits rounded to integers, so a few tokens carry the mass and repeats occur."""
    return torch.round(torch.randn(M, V, generator=gen(2000 + V + seed)) * 2.0)


def frame_offsets(frame, seed=0):
    """Per-row starts in 0 .. frame; the first rows get both ends."""
    off = torch.randint(0, frame + 1, (M,), generator=gen(3000 + frame + seed), dtype=torch.int32)
    off[0], off[1] = 0, frame
    return off


def forced_rows(V):
    """-1 (free), a code, the end-of-sequence id: mixed in one launch."""
    sup, eos = layout(V)
    return torch.tensor([(-1, (r * 5 + 1) % sup, eos)[r % 3] for r in range(M)], dtype=torch.int32)


def reference(logits, sp, frame, frame_off, group, sup_from, eos, eos_live, min_frames, forced=None, seen=None, seed=SEED, items=ITEMS):
    """What one launch must leave behind: (raw tokens, margins, out, eos flags, seen afterwards); seen [M][V] bool or None.
    A forced row has margin inf."""
    lg = logits.numpy()
    V = lg.shape[1]
    toks, margins = [], []
    seen_after = None if seen is None else seen.clone()
    for r in range(lg.shape[0]):
        own = int(frame) - int(frame_off[r])
        if forced is not None and int(forced[r]) >= 0:
            tok, mar = int(forced[r]), np.inf
        else:
            sup = np.zeros(V, bool)
            sup[sup_from:] = True
            if eos >= 0 and eos_live and own >= min_frames:
                sup[eos] = False
            tok, mar = draw_decided(lg[r], sp, uniform(seed, items[r] & 0xFFFFFFFF, own, group), sup,
                                    None if seen is None else seen[r].numpy())
        toks.append(tok)
        margins.append(mar)
        if seen_after is not None:
            seen_after[r, tok] = True
    flags = [int(eos >= 0 and t == eos) for t in toks]
    out = [0 if f else t for t, f in zip(toks, flags)]
    return toks, margins, out, flags, seen_after

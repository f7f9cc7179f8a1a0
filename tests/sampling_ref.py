"""The sampler's definition (oracle/sampling.py) with a statement of when a draw is DECIDED, and the replay of a finished
sampled generation draw by draw (tests/test_sampler_frame_gpu.py, tests/test_sampled_loop_gpu.py).

The GPU sampler and oracle.sampling.draw define the same float32 order - penalty, suppression, l / T, the (value desc,
index asc) sort, the Kogge-Stone running sums.  The one place they may differ is expf against np.exp: each is at most 1 ulp
off, so a term differs by at most 2^-22 relative, and six rounded additions per side add 12 * 2^-24: 2^-20 relative in all.
A draw whose every comparison (cum against the top-p limit, cum against the target) is further than that from equality is
decided: both sides must give the same token.  A draw closer than that is left out, and the share left out is capped."""
from types import SimpleNamespace

import numpy as np

from oracle.model import OracleModel
from oracle.sampling import SamplingParams, draw, scan_f32, uniform  # noqa: F401  (draw, uniform: re-exported)

DECIDED = 2.0 ** -20          # smallest margin of a decided draw
CAP = 0.01                    # largest share of a test's draws that may be undecided


def draw_decided(logits, sp, u, suppress=None, seen=None):
    """(token, margin): oracle.sampling.draw's token, and the smallest distance - relative to the total the comparison uses -
    between a running sum and the top-p limit (top_p < 1) or the target.  inf for greedy draws and rows with one candidate."""
    l = np.array(logits, dtype=np.float32, copy=True)
    if seen is not None and sp.repetition_penalty != 1.0:
        pen = np.float32(sp.repetition_penalty)
        l = np.where(seen, np.where(l > 0, l / pen, l * pen), l).astype(np.float32)
    if suppress is not None:
        l[suppress] = -np.inf
    if not sp.do_sample:
        return int(np.argmax(l)), np.inf
    if not (1 <= sp.top_k <= 64):
        raise ValueError("sampling needs 1 <= top_k <= 64")
    l = (l / np.float32(sp.temperature)).astype(np.float32)
    order = np.lexsort((np.arange(l.shape[0]), -l))[: sp.top_k]
    order = order[np.isfinite(l[order])]
    if order.size == 0:
        return int(np.argmax(l)), np.inf
    if order.size == 1:
        return int(order[0]), np.inf
    p = np.exp((l[order] - l[order[0]]).astype(np.float32)).astype(np.float32)
    cum = scan_f32(p)
    total = cum[-1]
    keep = p.shape[0]
    margin = np.inf
    c64 = cum.astype(np.float64)
    if sp.top_p < 1.0:
        lim = np.float32(np.float32(sp.top_p) * total)
        margin = float(np.abs(c64 - float(lim)).min() / float(total))
        reach = np.nonzero(cum >= lim)[0]
        if reach.size:
            keep = int(reach[0]) + 1
            total = cum[keep - 1]
    target = np.float32(u * total)
    margin = min(margin, float(np.abs(c64[:keep] - float(target)).min() / float(total)))
    over = np.nonzero(cum[:keep] > target)[0]
    return (int(order[int(over[0])]) if over.size else int(order[keep - 1])), margin


def talker_suppress(cfg, allow_eos):
    """OracleModel.talker_suppress for a configuration alone (the method reads nothing but self.cfg)."""
    return OracleModel.talker_suppress(SimpleNamespace(cfg=cfg), allow_eos)


def replay(cfg, codes, n_frames, trace, sp_talker, sp_pred, seed, item_ids, ignore_eos, min_frames, frame_add=0, item_add=0,
           group_add=0, history=True, eos_from=None, forced_frames=None):
    """Every draw of a finished sampled generation, recomputed from the traced logits.

    codes: the per-item [T_i][G] codes the generation returned; n_frames: the per-item frame limits it was given; trace:
    {"talker": [T][B][V], "predictor": [T][G-1][B][Vp]} float32 on the CPU.  An item with fewer frames than its limit stopped
    at an end of sequence: its draw at (item, T_i, 0) is replayed too and is expected to be the end-of-sequence id.
    forced_frames: per item, the number of leading frames that were teacher-forced - no draws, but their group-0 codes enter the
    history (a forced end of sequence is no draw either).  Behind them group 0 is drawn freely while the other groups stay forced to
    the last forced frame's codes (oracle/model.py, OracleModel.generate): only the group-0 draws are replayed for such an item.
    Returns a list of (item index, frame, group, expected token, margin, token the generation holds).

    frame_add / item_add / group_add / history / eos_from replay a DIFFERENT sampler (the key shifted by one, no penalty
    history, end of sequence allowed from another frame on): what the tests use to show that a case tells these apart."""
    G = cfg.n_groups
    eos_from = min_frames if eos_from is None else eos_from
    masks = {a: talker_suppress(cfg, a) for a in (False, True)}
    tk, pr = trace["talker"].numpy(), trace["predictor"].numpy()
    out = []
    for b, item in enumerate(item_ids):
        T = int(codes[b].shape[0])
        stopped = T < int(n_frames[b])
        got = codes[b].numpy()
        seen = np.zeros(cfg.codec_vocab, dtype=bool)
        n_forced = 0 if forced_frames is None else int(forced_frames[b])
        for t in range(T + (1 if stopped else 0)):
            if t < n_forced:
                if t < T:
                    seen[int(got[t, 0])] = True
                continue
            allow = (not ignore_eos) and t >= eos_from
            tok, mar = draw_decided(tk[t, b], sp_talker, uniform(seed, item + item_add, t + frame_add, group_add), masks[allow],
                                    seen if history else None)
            have = cfg.codec_eos_id if t == T else int(got[t, 0])
            out.append((b, t, 0, tok, mar, have))
            seen[have] = True
            if t == T or n_forced:
                continue
            for g in range(1, G):
                tok, mar = draw_decided(pr[t, g - 1, b], sp_pred, uniform(seed, item + item_add, t + frame_add, g + group_add))
                out.append((b, t, g, tok, mar, int(got[t, g])))
    return out


def tally(draws):
    """(number of draws, undecided ones, mismatches among the decided ones, smallest margin among the decided ones)."""
    decided = [d for d in draws if d[4] >= DECIDED]
    bad = [d for d in decided if d[3] != d[5]]
    return len(draws), len(draws) - len(decided), bad, min((d[4] for d in decided), default=np.inf)

"""Reference of the token-time path (rt_stt_align; DESIGN.md section 5, "word times"): transformers' own ``_median_filter`` and
``_dynamic_time_warping`` (models/whisper/generation_whisper.py) around a float64 normalisation, and the teacher-forced pass of the
oracle (oracle/whisper.build) with ``output_attentions=True``.

Row convention (OpenAI's and faster-whisper's): the decoder reads [prefix + ids]; the n + 1 rows at positions P - 1 .. P - 1 + n are the
alignment rows, row k predicts token k of ids + [end-of-sequence].  The row whose input would be end-of-sequence is not fed."""
import numpy as np
import torch
from transformers.models.whisper.generation_whisper import _dynamic_time_warping, _median_filter


def planted_matrix(n, F, seed, noise=0.5):
    """A matrix [n][F] with a planted staircase - row i owns the frames [edges[i], edges[i + 1]) at +4 - over uniform noise in
    (-noise, 0], and the staircase's first frames.  For F >= n the staircase is the one best path: it collects every +4 cell, and a
    cell off it only costs.  (n > F: rows without a frame of their own share one; the best path is then whatever the reference finds.)"""
    g = np.random.default_rng(seed)
    edges = np.minimum(np.round(np.linspace(0, F, n + 1)).astype(np.int64), F)
    M = (-noise * g.random((n, F))).astype(np.float32)
    for i in range(n):
        M[i, edges[i]:max(edges[i + 1], min(edges[i] + 1, F))] += 4.0
    return M, np.minimum(edges[:n], F - 1)


def dtw_frames(M) -> np.ndarray:
    """Per row of M [n][F] the frame at which the least-cost path over -M enters it: ``_extract_token_timestamps``' jump rule."""
    text, time = _dynamic_time_warping(-np.asarray(M, dtype=np.float32).astype(np.float64))
    jumps = np.pad(np.diff(text), (1, 0), constant_values=1).astype(bool)
    return np.asarray(time)[jumps].astype(np.int64)


def matrix(W, width: int) -> torch.Tensor:
    """W [heads][n][F] (float32) -> M [n][F] (float32): population standard deviation and mean over the rows in float64, z = 0 where the
    deviation is 0 (the library's documented deviation: the reference has NaN there), ``_median_filter`` along time, the mean over
    the heads in float64, rounded once."""
    w = torch.as_tensor(W, dtype=torch.float32).double()
    std = torch.std(w, dim=-2, keepdim=True, unbiased=False)
    mean = torch.mean(w, dim=-2, keepdim=True)
    z = torch.where(std == 0, torch.zeros_like(w), (w - mean) / torch.where(std == 0, torch.ones_like(std), std))
    z = _median_filter(z[None], width)[0]
    return z.mean(dim=0).float()


def frames_from_weights(W, width: int) -> np.ndarray:
    return dtw_frames(matrix(W, width).numpy())


def n_frames(cfg, n16: int) -> int:
    return int(min(max(n16 // cfg.hop // 2, 1), cfg.n_ctx))


@torch.no_grad()
def model_pass(model, cfg, mel: torch.Tensor, ids, heads, F: int):
    """(W [heads][n + 1][F] float32, log-probabilities [n]) of the oracle's teacher-forced pass over prefix + ids."""
    P, n = len(cfg.prefix), len(ids)
    toks = torch.tensor([list(int(t) for t in cfg.prefix) + [int(t) for t in ids]])
    out = model(input_features=mel[None], decoder_input_ids=toks, output_attentions=True)
    rows = slice(P - 1, P + n)
    W = torch.stack([out.cross_attentions[l][0, h, rows, :F] for l, h in heads]).float()
    lp = torch.log_softmax(out.logits[0, P - 1:P - 1 + n, :cfg.eos_id].float(), dim=-1)
    return W, lp[torch.arange(n), torch.tensor([int(t) for t in ids])] if n else lp[:0, 0]

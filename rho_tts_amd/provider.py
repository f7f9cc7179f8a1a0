"""``MI355XQwenTTS`` — the drop-in generation provider.

Registers through ``TTSFactory.register_provider()`` (factory.py:110-123) and implements the two
abstract members of ``BaseTTS`` (``_generate_audio`` base_tts.py:587-599, ``sample_rate`` :1192-1196)
with the constructor surface of the reference's ``QwenTTS`` (providers/qwen.py:48-66).

What differs from the reference, on purpose:
  * ``batch_size`` is live.  The reference stores it and never reads it (qwen.py:59,83) and its
    ``_run_pipeline`` is strictly sequential (base_tts.py:726,753,770).  Here ``_run_pipeline`` is
    overridden to flatten texts -> segments, run them ``batch_size`` at a time through
    ``_generate_audio(list)``, and finish every item (join -> loudness -> decay check) in ONE fused
    HIP launch — with the reference's per-item semantics (listed at ``BatchedPipeline``).
  * the voice conditioning is computed once per voice, not on every call (qwen.py:253-258).
  * ``sample_rate`` is a constant; the reference generates a throw-away sample to learn it (qwen.py:408-413).
  * every numeric leaf runs on the GPU through the C ABI; there is no CPU path.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import logging
import threading
import time
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import torch

from . import _native
from .api import (BaseTTS, CancellationToken, CancelledException, ProviderInfo, TTSFactory, VoiceInfo)

logger = logging.getLogger("rho_tts_amd")

PROVIDER_NAME = "qwen_mi355x"
BUILTIN_VOICES = ["Chelsie", "Aidan", "Vivian", "Ryan", "Aria", "Ethan", "Luna", "Harper", "James"]
_NO_TRANSCRIPT = object()      # "no transcript was handed in" (None is a transcript: the transcription failed)


class BatchedPipeline:
    """Batched restatement of ``BaseTTS._run_pipeline`` (base_tts.py:708-956).  Kept from the reference:
      - phonetic mapping first (:721); segmentation per text with the memory-aware limit (:730-731)
      - ``CancelledException`` is raised, not returned, at text / segment / iteration granularity (:727,754,771)
      - ``ValueError`` propagates; ``RuntimeError`` mentioning "out of memory" or "length" and any other
        exception fail only the segment they hit and are retried up to ``max_iterations`` (:786-797);
        other ``RuntimeError`` propagate (:794)
      - ``max_iterations == 1`` means no validation calls at all (:800)
      - a text whose audio decays is regenerated whole, up to ``max_decay_retries`` times, with a seed taken
        from the wall clock (:741-748, 926-941)
      - per-item ``None`` on failure (:943-946); metadata: ``decay_ratio`` always, ``drift_prob`` = max and
        ``text_similarity`` = min only when validation ran (:948-953)
      - ``progress_callback("Generating segment i/n...")`` once per segment and attempt (:760-761)
    """

    def _run_pipeline(self, texts, cancellation_token, progress_callback=None):
        plans = self._plan_texts(texts, cancellation_token)
        self._begin_retry_seeds()
        return self._run_plans(plans, list(range(len(plans))), cancellation_token, progress_callback)

    def _plan_texts(self, texts, token, max_chars: Optional[int] = None) -> List[List[str]]:
        """Phonetic mapping, then segmentation per text with the memory-aware limit (base_tts.py:721,727-731).
        ``max_chars``: a limit agreed beforehand (data-parallel runs: every rank must cut the texts alike) instead of this
        process's own free-memory reading."""
        mapped = [self._apply_phonetic_mapping(t) for t in texts]
        plans: List[List[str]] = []
        for idx, text in enumerate(mapped):
            if token.is_cancelled():
                raise CancelledException(f"Cancelled during text item {idx}")
            plans.append(self._split_text_into_segments(text, self._compute_max_chars() if max_chars is None else max_chars))
        return plans

    # ---- retry seeds.  The reference reseeds from the wall clock at every decay retry and validation retry
    # (``self.seed = int(time.time() * 1000) % 100000``, base_tts.py:743,778) and leaves ``self.seed`` mutated.  Here the clock is
    # read ONCE per call and the seed of retry stage (decay attempt a, validation iteration k) is derived from that reading: still
    # a fresh clock-dependent seed per retry, still left in ``self.seed`` - but a function of (clock reading, a, k) alone, so the
    # ranks of a data-parallel call (which share rank 0's reading) give an item the audio one GPU would, retries included, and
    # can agree afterwards on the seed the call leaves behind.
    @staticmethod
    def _retry_clock() -> int:
        return int(time.time() * 1000) % 100000

    def _begin_retry_seeds(self, base: Optional[int] = None, entry_seed: Optional[int] = None) -> None:
        self._retry_base = int(self._retry_clock() if base is None else base)
        self._entry_seed = int(self.seed if entry_seed is None else entry_seed)
        self.seed = self._entry_seed
        self._last_stage = (0, 0)

    def _stage_seed(self, attempt: int, iteration: int) -> int:
        if (attempt, iteration) == (0, 0):
            return self._entry_seed
        return int((self._retry_base + 7919 * attempt + 104729 * iteration) % 100000)

    def _enter_stage(self, attempt: int, iteration: int) -> None:
        if not hasattr(self, "_retry_base"):
            self._begin_retry_seeds()
        self.seed = self._stage_seed(attempt, iteration)
        self._last_stage = max(getattr(self, "_last_stage", (0, 0)), (attempt, iteration))

    def _run_plans(self, plans, owned, token, progress_callback=None):
        """The pipeline for the text items ``owned`` (indices into ``plans``; all of them on one GPU, this rank's share in a
        data-parallel run).  Returns one entry per owned item, in that order.  The RNG stream of a segment is its position in
        the work list of ALL items, owned or not: a text's audio does not depend on how many ranks shared the list."""
        seg_base, tot = [], 0
        for pl in plans:
            seg_base.append(tot)
            tot += len(pl)
        n = len(plans)
        final: List[Optional[torch.Tensor]] = [None] * n
        seg_audio: List[List[torch.Tensor]] = [[] for _ in range(n)]
        decay: List[Tuple[float, bool]] = [(0.0, True)] * n
        scores: List[Tuple[List[float], List[float]]] = [([], []) for _ in range(n)]
        pending = list(owned)
        cv = self._call_voices                               # (once per call, not per retry)
        if cv is not None and self.max_iterations > 1 and any(cv[i] is not None for i in owned) and \
                (getattr(self, "drift_scorer", None) is not None or hasattr(self, "_validate_accent_drift")):
            logger.info(f"  {sum(cv[i] is not None for i in owned)} text(s) speak with a bank voice: accent drift is scored for the "
                        "provider's own voice only")
        for attempt in range(self.max_decay_retries):
            if not pending:
                break
            if attempt > 0:
                self._enter_stage(attempt, 0)
                logger.warning(f"  sound decay detected in {len(pending)} item(s), regenerating (attempt {attempt + 1}/{self.max_decay_retries})")
            work = [(i, s, seg) for i in pending for s, seg in enumerate(plans[i])]
            for i in pending:
                seg_audio[i], scores[i] = [], ([], [])
            got = self._generate_work(work, plans, token, progress_callback, scores, [seg_base[i] + s for i, s, _ in work], attempt)
            for (i, s, _), a in zip(work, got):
                if a is not None:
                    seg_audio[i].append(a)
            ready = [i for i in pending if seg_audio[i]]
            finished = self._finish_items([seg_audio[i] for i in ready]) if ready else []
            still = []
            for i, res in zip(ready, finished):
                if res is None:
                    continue
                final[i], ratio, ok = res
                decay[i] = (ratio, ok)
                logger.info(f"  Item {i + 1} sound decay ratio: {ratio:.3f} (threshold: {self.sound_decay_threshold})")
                if not ok:
                    still.append(i)
            pending = still
        out: List[Optional[Tuple[torch.Tensor, int, dict]]] = []
        for i in owned:
            if final[i] is None or not seg_audio[i]:
                logger.error(f"Item {i + 1} failed: no audio generated")
                out.append(None)
                continue
            meta: Dict[str, float] = {}
            if scores[i][0]:
                meta["drift_prob"] = max(scores[i][0])
            if scores[i][1]:
                meta["text_similarity"] = min(scores[i][1])
            meta["decay_ratio"] = decay[i][0]
            out.append((final[i], len(seg_audio[i]), meta))
        return out

    # Voices of the call in flight, one entry per TEXT (None: the provider's own voice), or None when the call names none
    # (MI355XQwenTTS.generate(voices=...)).  Every segment of a text inherits its text's voice.
    _call_voices: Optional[List[Optional[str]]] = None

    def _work_voices(self, work) -> Optional[List[Optional[str]]]:
        cv = self._call_voices
        return None if cv is None else [cv[i] for i, _, _ in work]

    # one entry of `work` per (item, segment index, text); returns the accepted audio (or None) per entry
    def _generate_work(self, work, plans, token, progress_callback, scores, stream_ids=None, attempt: int = 0):
        if stream_ids is None:
            stream_ids = list(range(len(work)))
        # the drift classifier is trained for the provider's own voice: segments of another voice are not scored (no drift_prob),
        # their text match and the decay check run as ever
        voices = self._work_voices(work)
        foreign = None if voices is None else [v is not None for v in voices]
        accepted: List[Optional[torch.Tensor]] = [None] * len(work)
        # per-segment validation state, exactly the reference's locals (base_tts.py:765-768): best audio by drift, the
        # MINIMUM drift seen, the LAST text similarity computed (whenever the voice check passed), the last audio
        state = [{"best": None, "best_drift": float("inf"), "text_sim": None, "last": None} for _ in work]
        todo = list(range(len(work)))
        bs = max(1, int(getattr(self, "batch_size", 1)))
        for iteration in range(self.max_iterations):
            if not todo:
                break
            if iteration > 0:
                self._enter_stage(attempt, iteration)
            retry: List[int] = []
            for chunk in self._cut_batches(todo, work, bs):
                for w in chunk:
                    i, s, _ = work[w]
                    if token.is_cancelled():
                        raise CancelledException(f"Cancelled during segment {s + 1} of item {i + 1}")
                    if progress_callback and iteration == 0:
                        progress_callback(f"Generating segment {s + 1}/{len(plans[i])}...")
                self._set_seeds()
                # RNG stream of a segment = its index in the work list of the whole call: independent of how the list is cut into
                # batches and of how many ranks share it
                skip = None if foreign is None else [foreign[w] for w in chunk]
                if voices is None:
                    audios = self._generate_chunk([work[w][2] for w in chunk], [stream_ids[w] for w in chunk], token)
                else:
                    audios = self._generate_chunk([work[w][2] for w in chunk], [stream_ids[w] for w in chunk], token, [voices[w] for w in chunk])
                scored = audios if skip is None else [None if f else a for a, f in zip(audios, skip)]
                drifts = self._chunk_drifts(scored) if self.max_iterations > 1 else None
                texts = self._chunk_texts(audios, drifts, skip) if self.max_iterations > 1 else None
                for k, (w, a) in enumerate(zip(chunk, audios)):
                    if a is None:
                        retry.append(w)
                        continue
                    state[w]["last"] = a
                    if self.max_iterations == 1:
                        state[w]["best"] = a
                        accepted[w] = a
                        if getattr(self, "auto_sort_good_dir", None) or getattr(self, "auto_sort_bad_dir", None):
                            self._auto_sort_only(a)          # drift detection for auto-sort even without validation retries (:801-818)
                        continue
                    if self._validate_segment(a, work[w][2], state[w], None if drifts is None else drifts[k],
                                              transcript=_NO_TRANSCRIPT if texts is None else texts[k],
                                              score_drift=not (skip is not None and skip[k])):
                        accepted[w] = a                      # valid: this attempt's audio is kept (:859)
                    else:
                        retry.append(w)
            todo = retry
        for w in todo:                                       # iterations exhausted: best by drift, else the last audio (:887-898)
            st = state[w]
            accepted[w] = st["best"] if st["best"] is not None else st["last"]
        if self.max_iterations > 1:
            for w, a in enumerate(accepted):                 # scores of every segment that produced audio (:901-906)
                if a is None:
                    continue
                i = work[w][0]
                if state[w]["best_drift"] != float("inf"):
                    scores[i][0].append(state[w]["best_drift"])
                if state[w]["text_sim"] is not None:
                    scores[i][1].append(state[w]["text_sim"])
        return accepted

    def _estimate_cost(self, segment: str) -> Optional[float]:
        """Expected decode length of a segment (any monotone unit), or None when the provider cannot tell.
        A batch decodes until its LONGEST member ends, so ragged batches idle their short rows."""
        return None

    def _cut_batches(self, todo: List[int], work, bs: int) -> List[List[int]]:
        """Cut the work list into batches of ``bs``.  More work than one batch is bucketed by estimated length (longest first,
        so every batch holds segments of similar length); fewer keeps arrival order.  The RNG stream of a segment is its index
        in the work list, so the audio of every segment is the same for any cut; inside a batch the indices stay ascending."""
        if len(todo) > bs:
            costs = {w: self._estimate_cost(work[w][2]) for w in todo}
            if all(c is not None for c in costs.values()):
                order = sorted(todo, key=lambda w: (-costs[w], w))
                return [sorted(order[b0:b0 + bs]) for b0 in range(0, len(order), bs)]
        return [todo[b0:b0 + bs] for b0 in range(0, len(todo), bs)]

    def _generate_chunk(self, segs: List[str], item_idx: List[int], token, voices=None) -> List[Optional[torch.Tensor]]:
        """One batched ``_generate_audio`` call; on failure fall back to one call per segment so that the
        reference's per-segment error policy decides who fails.  ``voices``: a bank name (or None) per segment, handed on only when
        the call names voices at all."""
        def kw(k=None):
            return {} if voices is None else {"voices": list(voices) if k is None else [voices[k]]}
        try:
            out = self._generate_audio(list(segs), item_ids=item_idx, cancellation_token=token, **kw())
            return list(out)
        except (ValueError, CancelledException):
            raise
        except Exception as first:  # noqa: BLE001
            if len(segs) == 1:
                return [self._classify(first)]
        res: List[Optional[torch.Tensor]] = []
        for k, (seg, it) in enumerate(zip(segs, item_idx)):
            try:
                res.append(self._generate_audio(seg, item_ids=[it], cancellation_token=token, **kw(k)))
            except (ValueError, CancelledException):
                raise
            except Exception as e:  # noqa: BLE001
                res.append(self._classify(e))
        return res

    @staticmethod
    def _classify(e: Exception):
        if isinstance(e, RuntimeError):
            msg = str(e).lower()
            if "out of memory" in msg or "length" in msg:
                logger.error(f"    segment OOM/length: {e}")
                if torch.cuda.is_available():
                    torch.cuda.empty_cache()
                return None
            raise e
        logger.warning(f"    generation error ({e})")
        return None

    # Optional tensor-level validators: callables on the waveform the provider still holds (GPU or CPU,
    # 1-D float32) - when both are set a segment is validated without the reference's temp-WAV round trip
    # (base_tts.py:821-830); either one alone replaces its file-based counterpart.
    drift_scorer = None        # Callable[[torch.Tensor, int], float]            -> accent-drift probability
    transcriber = None         # Callable[[torch.Tensor, int], Optional[str]]    -> transcription (None = failed)

    def _chunk_drifts(self, audios) -> Optional[List[Optional[float]]]:
        """The drift of every audio of a chunk from ONE call of ``drift_scorer.batch`` (features.make_drift_scorer: one native
        call and one host synchronisation for the chunk), aligned with ``audios`` (None where there is no audio) - or None when
        the scorer has no ``batch``, or when the call fails: the per-segment call then decides, segment by segment."""
        batch = getattr(getattr(self, "drift_scorer", None), "batch", None)
        have = [a for a in audios if a is not None]
        if not callable(batch) or not have:
            return None
        try:
            vals = [float(v) for v in batch(have, self.sample_rate)]
            if len(vals) != len(have):
                raise RuntimeError(f"drift_scorer.batch returned {len(vals)} scores for {len(have)} segments")
        except Exception as e:  # noqa: BLE001
            logger.warning(f"    batched drift scoring failed ({e}); scoring per segment")
            return None
        it = iter(vals)
        return [None if a is None else next(it) for a in audios]

    def _chunk_texts(self, audios, drifts, skip=None) -> Optional[list]:
        """The transcript of every segment of a chunk that the per-segment order would transcribe, from ONE call of
        ``transcriber.batch`` (stt.WhisperTranscriber.batch: one native call for the chunk), aligned with ``audios``
        (``_NO_TRANSCRIPT`` where the segment is not in the call).  A segment is in the call when it has audio and its voice check
        is known to pass before the text check: its drift from ``_chunk_drifts`` is below the threshold, or no drift scorer and no
        file-based drift validator is configured.  Any other segment is decided by the per-segment call, and so is the whole
        chunk - None - when the transcriber has no ``batch`` or the call fails."""
        batch = getattr(getattr(self, "transcriber", None), "batch", None)
        if not callable(batch):
            return None
        skip = list(skip) if skip is not None else [False] * len(audios)      # segments whose voice check is not run: they pass it
        if getattr(self, "drift_scorer", None) is not None:
            if drifts is None and not all(f or a is None for a, f in zip(audios, skip)):
                return None
            drifts = drifts if drifts is not None else [None] * len(audios)
            take = [a is not None and (f or (d is not None and float(d) < self.accent_drift_threshold)) for a, d, f in zip(audios, drifts, skip)]
        elif hasattr(self, "_validate_accent_drift"):
            return None
        else:
            take = [a is not None for a in audios]
        have = [a for a, t in zip(audios, take) if t]
        if not have:
            return None
        try:
            vals = list(batch(have, self.sample_rate))
            if len(vals) != len(have):
                raise RuntimeError(f"transcriber.batch returned {len(vals)} transcripts for {len(have)} segments")
        except Exception as e:  # noqa: BLE001
            logger.warning(f"    batched transcription failed ({e}); transcribing per segment")
            return None
        it = iter(vals)
        return [next(it) if t else _NO_TRANSCRIPT for t in take]

    def _validate_segment(self, audio: torch.Tensor, text: str, st: dict, drift: Optional[float] = None, transcript=_NO_TRANSCRIPT,
                          score_drift: bool = True) -> bool:
        """One validation attempt (base_tts.py:821-886), updating the segment's state in the reference's order: drift ->
        auto-sort -> best-by-drift -> text match only if the voice passed.  A validator that raises counts as a failed
        attempt but keeps what it had already recorded.  Returns True when the attempt is accepted.  ``drift``: the scorer's value
        for this audio when the chunk was scored in one call (``_chunk_drifts``); the scorer is then not called again.  ``transcript``:
        likewise the transcriber's text from ``_chunk_texts`` (None is a transcript: "transcription failed").  ``score_drift=False``
        (a segment of a bank voice, for which the classifier was not trained): the voice check is not run and passes, no drift is
        recorded; the text check is the same."""
        scorer, transcriber = getattr(self, "drift_scorer", None), getattr(self, "transcriber", None)
        file_based = hasattr(self, "_validate_accent_drift")          # the reference's file-based validators (absent in the host mirror)
        if not score_drift:
            try:
                if st["best"] is None:
                    st["best"] = audio
                text_ok = True
                if transcriber is not None:
                    from .validation import validate_text_match
                    heard = transcriber(audio, self.sample_rate) if transcript is _NO_TRANSCRIPT else transcript
                    text_ok, sim, _ = validate_text_match(heard, text, self.text_similarity_threshold)
                    st["text_sim"] = sim
                elif file_based:
                    with self._validation_input(audio) as path:
                        text_ok, sim, _ = self._validate_text_match(path, text)
                    st["text_sim"] = sim
                if text_ok:
                    st["best"] = audio
                return bool(text_ok)
            except Exception as e:  # noqa: BLE001
                logger.warning(f"    validation error ({e})")
                return False
        if scorer is None and transcriber is None and not file_based:
            st["best"] = audio
            return True
        need_file = file_based and (scorer is None or transcriber is None or bool(getattr(self, "auto_sort_good_dir", None) or getattr(self, "auto_sort_bad_dir", None)))
        try:
            with (self._validation_input(audio) if need_file else contextlib.nullcontext(None)) as path:
                if scorer is not None:
                    drift = float(scorer(audio, self.sample_rate)) if drift is None else float(drift)
                    voice_ok = drift < self.accent_drift_threshold
                elif file_based:
                    drift, voice_ok = self._validate_accent_drift(path)
                else:
                    drift, voice_ok = 0.0, True                        # no classifier: passes, as base_tts.py:218-220 does
                if path is not None and hasattr(self, "_auto_sort_audio"):
                    self._auto_sort_audio(path, drift)
                if drift < st["best_drift"]:
                    st["best_drift"], st["best"] = drift, audio.clone()
                text_ok = True
                if voice_ok:
                    if transcriber is not None:
                        from .validation import validate_text_match
                        heard = transcriber(audio, self.sample_rate) if transcript is _NO_TRANSCRIPT else transcript
                        text_ok, sim, _ = validate_text_match(heard, text, self.text_similarity_threshold)
                        st["text_sim"] = sim
                    elif file_based:
                        text_ok, sim, _ = self._validate_text_match(path, text)
                        st["text_sim"] = sim
                if voice_ok and text_ok:
                    st["best"] = audio
                    return True
                return False
        except Exception as e:  # noqa: BLE001
            logger.warning(f"    validation error ({e})")
            return False

    def _auto_sort_only(self, audio: torch.Tensor) -> None:
        """``max_iterations == 1`` with an auto-sort directory set (base_tts.py:801-818): score the accepted audio and copy it to
        the good / bad folder; nothing is retried and no score reaches the metadata.  As in the reference, only the copy itself
        is non-fatal (``_auto_sort_audio`` swallows ``OSError``)."""
        scorer = getattr(self, "drift_scorer", None)
        with self._validation_input(audio) as path:
            drift = float(scorer(audio, self.sample_rate)) if scorer is not None else self._validate_accent_drift(path)[0]
            self._auto_sort_audio(path, drift)

    def _validation_input(self, audio: torch.Tensor):
        """What the validators are handed: the reference's file-based validators get a temporary 16-bit WAV
        (base_tts.py:821-830), written from a device-side int16 conversion when the audio lives on the GPU."""
        import os
        import tempfile

        @contextlib.contextmanager
        def cm():
            fd, path = tempfile.mkstemp(suffix=".wav", prefix="rho_tts_validate_")
            os.close(fd)
            try:
                mono = audio.detach()
                self._save_wav(path, mono.unsqueeze(0) if mono.dim() == 1 else mono, self.sample_rate)
                yield path
            finally:
                try:
                    os.remove(path)
                except OSError:
                    pass
        return cm()


class DataParallelPipeline(BatchedPipeline):
    """``_run_pipeline`` across the GPUs of a node (BASELINE.json configs[3]): one process per GPU under
    ``torch.distributed`` (backend "nccl" = RCCL over xGMI), every rank calling ``generate()`` with the SAME texts.
    The reference's loop over texts is strictly sequential (base_tts.py:726-954) and keeps no state between items, so whole text
    items are the unit: they are dealt over the ranks by estimated decode length (dist.shard_items), every rank runs its share
    through the batched pipeline above (continuous batching on its decode rows, validation and decay retries included), and the
    finished waveforms + per-item records are gathered to rank 0 and put back in the caller's order.  Two collectives carry
    data - the broadcast of the voice conditioning rank 0 computed (once per voice) and the gather of the waveforms - plus
    one-word status exchanges so that a failure on one rank ends the call on all of them.
    Rank 0 returns the complete result list; the other ranks return their own items and ``None`` elsewhere (``generate()`` on
    them returns nothing and saves nothing: MI355XQwenTTS.generate).  A text's audio is a function of (text, voice, seed,
    position in the call), not of the number of ranks.
    ``data_parallel``: "auto" (on when a process group with more than one rank is initialised), True, False."""

    data_parallel = "auto"

    def _dp(self):
        mode = getattr(self, "data_parallel", "auto")
        if mode is False or mode in ("off", "0"):
            return None
        import os

        import torch.distributed as td
        if not (td.is_available() and td.is_initialized()):
            if mode is True:
                raise ValueError("data_parallel=True needs an initialised torch.distributed process group "
                                 "(launch one process per GPU with torch.distributed.run; rho_tts_amd.dist.init_from_env)")
            return None
        world = td.get_world_size()
        forced = mode is True or os.environ.get("RHO_TTS_AMD_FORCE_DIST", "") not in ("", "0")    # (one rank: exercises the RCCL call sites)
        if world < 2 and not forced:
            return None
        return td, td.get_rank(), world

    def _dp_device(self, td) -> torch.device:
        return torch.device(self.device) if str(td.get_backend()) == "nccl" else torch.device("cpu")

    @staticmethod
    def _dp_agree(td, dev, err: Optional[BaseException], what: str) -> None:
        from . import dist as D
        code = 0 if err is None else (2 if isinstance(err, CancelledException) else (3 if isinstance(err, ValueError) else 1))
        worst = D.agree(td, dev, code)
        if err is not None:
            raise err
        if worst == 2:
            raise CancelledException(f"cancelled on another rank during {what}")
        if worst == 3:
            raise ValueError(f"configuration error on another rank during {what}")
        if worst:
            raise RuntimeError(f"another rank failed during {what}")

    def _dp_share_voice(self, td, rank: int, dev) -> None:
        """Rank 0 computes the conditioning (audio encoder + prefix prefill), everyone else imports its KV blob."""
        raise NotImplementedError

    def _dp_costs(self, plans) -> List[float]:
        out = []
        for pl in plans:
            c = 0.0
            for seg in pl:
                e = self._estimate_cost(seg)
                c += float(e) if e is not None else float(max(1, len(seg.split())))
            out.append(c)
        return out

    def _run_pipeline(self, texts, cancellation_token, progress_callback=None):
        dp = self._dp()
        if dp is None:
            return super()._run_pipeline(texts, cancellation_token, progress_callback)
        from . import dist as D
        td, rank, world = dp
        dev = self._dp_device(td)
        plans, err, mc = [], None, 0
        # ---- what every rank must hold alike BEFORE anything is planned: the segment limit (it reads this process's free memory,
        # base_tts.py:158-185, and is refined by the loaded checkpoint, qwen.py:131-139 - so the engine is loaded first and the
        # ranks take the smallest limit any of them computed), the seed the call starts from and the clock reading its retry
        # seeds derive from (rank 0's)
        try:
            self._load_engine()
            mc = int(self._compute_max_chars())
        except BaseException as e:  # noqa: BLE001
            err = e
        self._dp_agree(td, dev, err, "loading")
        mc, _ = D.min_max(td, dev, mc)
        seed0, base0 = D.broadcast_ints(td, dev, [int(self.seed), self._retry_clock()], src=0)
        self._begin_retry_seeds(base0, seed0)
        try:
            plans = self._plan_texts(texts, cancellation_token, max_chars=mc)
        except BaseException as e:  # noqa: BLE001  (a token cancelled on ONE rank: re-raised by _dp_agree, on every rank)
            err = e
        self._dp_agree(td, dev, err, "planning")
        # the plans decide who owns what and where every waveform goes: a rank that cut its texts differently would drop or double
        # items without any error - so the plans' digest must agree before the deal
        import hashlib
        digest = int.from_bytes(hashlib.sha256(repr(plans).encode("utf-8")).digest()[:7], "big")
        lo, hi = D.min_max(td, dev, digest)
        if lo != hi:
            raise ValueError("data-parallel ranks planned different segmentations of the same texts (different texts, phonetic "
                             "mappings or segment limits per rank): every rank must call generate() with the same arguments")
        self._dp_share_voice(td, rank, dev)
        shards = D.shard_items(self._dp_costs(plans), world)
        local = []
        try:
            local = self._run_plans(plans, shards[rank], cancellation_token, progress_callback)
        except BaseException as e:  # noqa: BLE001  (re-raised by _dp_agree, on every rank)
            err = e
        # the seed the call leaves in self.seed is the last retry stage ANY rank reached - what one process running every item
        # would hold (its loops are attempt-major, iteration-minor) - so the next call starts alike on every rank
        a_k = getattr(self, "_last_stage", (0, 0))
        _, top = D.min_max(td, dev, a_k[0] * 100000 + a_k[1])
        self.seed = self._stage_seed(top // 100000, top % 100000)
        self._dp_agree(td, dev, err, "generation")
        nan = float("nan")
        wavs = [None if r is None else r[0].reshape(-1) for r in local]
        rows = torch.tensor([[0.0, nan, nan, nan, 0.0] if r is None else
                             [float(r[1]), float(r[2]["decay_ratio"]), float(r[2].get("drift_prob", nan)), float(r[2].get("text_similarity", nan)),
                              1.0 if r[0].dim() == 2 else 0.0] for r in local], dtype=torch.float64).reshape(len(local), 5)
        per_rank = D.gather_waveforms(wavs, td, dst=0, device=dev)
        recs = D.gather_rows(rows, td, dst=0, device=dev)
        if rank != 0:
            out: List[Optional[Tuple[torch.Tensor, int, dict]]] = [None] * len(plans)
            for i, r in zip(shards[rank], local):
                out[i] = r
            return out
        items = []
        for r in range(world):
            got = []
            for w, rec in zip(per_rank[r], recs[r].tolist()):
                if w is None:
                    got.append(None)
                    continue
                meta = {}
                if rec[2] == rec[2]:
                    meta["drift_prob"] = rec[2]
                if rec[3] == rec[3]:
                    meta["text_similarity"] = rec[3]
                meta["decay_ratio"] = rec[1]
                got.append((w.unsqueeze(0) if rec[4] else w, int(rec[0]), meta))
            items.append(got)
        return D.unshard(items, shards, len(plans))


class HipAudioLeaves:
    """The numeric leaves of the pipeline as calls into the fused HIP kernel (one stage mask each).
    Reference: base_tts.py:297-536, providers/qwen.py:268-378.  Inputs may be CPU or GPU tensors; the result lives
    where the input lived."""

    def _post_params(self, stages: int) -> _native.PostParams:
        return _native.make_post_params(
            sample_rate=self.sample_rate, silence_threshold_db=self.silence_threshold_db,
            fade_duration_sec=self.fade_duration_sec, crossfade_duration_sec=self.crossfade_duration_sec,
            inter_sentence_pause_sec=self.inter_sentence_pause_sec, trim_silence=self.trim_silence,
            sound_decay_threshold=getattr(self, "sound_decay_threshold", 0.3), stages=stages)

    def _post(self, items, stages, seg_trim=None):
        return self._native_ctx().post_process(self._post_params(stages), items, seg_trim)

    def _trim_silence(self, audio: torch.Tensor, from_start: bool = True, from_end: bool = True) -> torch.Tensor:
        if not self.trim_silence or audio.numel() == 0:
            return audio
        st = (_native.POST_TRIM_START if from_start else 0) | (_native.POST_TRIM_END if from_end else 0)
        if st == 0:
            return audio.reshape(-1) if audio.dim() == 2 else audio
        (out,), (s,) = self._post([[audio]], st)
        return out.unsqueeze(0) if s.all_silent else out       # the reference returns a (1, window) view for silence (:379-380)

    def _remove_dc_offset(self, audio: torch.Tensor) -> torch.Tensor:
        if audio.numel() == 0:
            return audio
        (out,), _ = self._post([[audio]], _native.POST_DC)
        return out.view(audio.shape)

    def _apply_fades(self, audio: torch.Tensor, fade_in: bool = True, fade_out: bool = True) -> torch.Tensor:
        if audio.numel() == 0:
            return audio
        st = (_native.POST_FADE_IN if fade_in else 0) | (_native.POST_FADE_OUT if fade_out else 0)
        (out,), _ = self._post([[audio]], st)
        return out.view(audio.shape)

    def _smooth_segment_join(self, audio_segments):
        if len(audio_segments) == 0:
            return None
        st = _native.POST_PIPELINE & ~(_native.POST_LOUDNESS | _native.POST_DECAY)
        (out,), (s,) = self._post([list(audio_segments)], st)
        return out.unsqueeze(0) if s.all_silent else out

    def _post_process_audio(self, audio: torch.Tensor) -> torch.Tensor:
        (out,), _ = self._post([[audio]], _native.POST_LOUDNESS)
        return out.view(audio.shape)

    def _validate_sound_decay(self, audio: torch.Tensor) -> tuple:
        if audio.numel() == 0:
            return 1.0, True
        _, (s,) = self._post([[audio]], _native.POST_DECAY)
        return s.decay_ratio, bool(s.decay_ok)

    def _save_wav(self, path: str, audio: torch.Tensor, sample_rate: int) -> None:
        """Output stage (base_tts.py:654-671).  A waveform that still lives in HBM is converted to the reference's 16-bit PCM
        (clip, x 32767, truncate - the stdlib fallback's definition) ON the device and crosses PCIe as int16: half the bytes of
        the float32 copy the reference makes first (:807,824,1046).  CPU tensors take the host API's own writer."""
        if not audio.is_cuda:
            return super()._save_wav(path, audio, sample_rate)
        import wave
        pcm = self._native_ctx().pcm16(audio).cpu().numpy()
        with wave.open(path, "wb") as wf:
            wf.setnchannels(1)
            wf.setsampwidth(2)
            wf.setframerate(sample_rate)
            wf.writeframes(pcm.tobytes())

    def _finish_items(self, items: Sequence[Sequence[torch.Tensor]]):
        """join -> loudness -> decay for every item, one launch (base_tts.py:912-926)."""
        outs, stats = self._post([list(it) for it in items], _native.POST_PIPELINE)
        return [(o.unsqueeze(0) if s.all_silent else o, s.decay_ratio, bool(s.decay_ok)) for o, s in zip(outs, stats)]


class MI355XQwenTTS(DataParallelPipeline, HipAudioLeaves, BaseTTS):
    """Qwen3-TTS generation on one MI355X.  Same keyword arguments as the reference's ``QwenTTS``."""

    MAX_MODEL_CHARS = 4000
    BYTES_PER_CHAR_ESTIMATE = 500_000

    def __init__(self, device: str = "cuda", seed: int = 789, deterministic: bool = False,
                 reference_audio: Optional[str] = None, reference_text: Optional[str] = None, speaker: Optional[str] = None,
                 language: str = "English", model_path: str = "Qwen/Qwen3-TTS-12Hz-1.7B-Base",
                 max_chars_per_segment: Optional[int] = None, batch_size: int = 32, max_iterations: int = 10,
                 accent_drift_threshold: float = 0.17, text_similarity_threshold: float = 0.85,
                 sound_decay_threshold: float = 0.3, drift_model_path: Optional[str] = None,
                 phonetic_mapping: Optional[Dict[str, str]] = None, speaker_encoder_path: Optional[str] = None,
                 speaker_similarity: str = "model", max_voices: int = 1):
        # Defaults are QwenTTS.__init__'s (providers/qwen.py:48-66) with ONE deviation: batch_size 32 instead of 5.  The reference
        # stores batch_size and never reads it (qwen.py:59,83), so no behaviour of its can depend on the value; here it is the
        # number of decode rows (BASELINE.json's headline batch).  max_iterations keeps the reference's 10: a caller who swaps
        # providers keeps the validation retries (they run whenever validators are installed or the tensor-level hooks are set).
        super().__init__(device, seed, deterministic, phonetic_mapping=phonetic_mapping)
        if reference_audio is not None and reference_text is None:
            raise ValueError("reference_text (transcript of reference audio) is required when reference_audio is set")
        if not str(device).startswith("cuda"):
            raise ValueError("MI355XQwenTTS runs on an AMD GPU only (device='cuda' or 'cuda:N'); there is no CPU path")
        self.reference_audio_path = reference_audio
        self.reference_text = reference_text
        self.speaker = speaker
        self.language = language
        self.voice_cloning = reference_audio is not None
        self.model_path = model_path
        self.drift_model_path = drift_model_path
        # The GE2E speaker encoder (speaker.SpeakerEmbedder; the .npz of tools/export_speaker_encoder.py).  With it a drift classifier
        # of 256 + 30 features needs no drift_embed, and speaker_similarity="ge2e" answers _compute_speaker_similarity with the
        # reference's arithmetic.  Without it (the default) nothing changes.
        if speaker_similarity not in ("model", "ge2e"):
            raise ValueError(f"speaker_similarity = {speaker_similarity!r}: 'model' (the talker's own speaker encoder) or 'ge2e'")
        if speaker_similarity == "ge2e" and not speaker_encoder_path:
            raise ValueError("speaker_similarity='ge2e' needs speaker_encoder_path (the .npz written by tools/export_speaker_encoder.py)")
        self.speaker_encoder_path = speaker_encoder_path
        self.speaker_similarity = speaker_similarity
        self._speaker_embedder = None                          # speaker.SpeakerEmbedder on this provider's context, made at first use
        self._ge2e_ref = None                                  # (voice key, unit embedding of the reference clip)
        self._max_chars_explicit = max_chars_per_segment is not None
        self.max_chars_per_segment = max_chars_per_segment if max_chars_per_segment is not None else 1000
        self.batch_size = batch_size
        self.force_sentence_split = False
        self.max_iterations = max_iterations
        self.accent_drift_threshold = accent_drift_threshold
        self.text_similarity_threshold = text_similarity_threshold
        self.sound_decay_threshold = sound_decay_threshold
        self._engine = None
        self._ctx = None
        self._speed_pitch = None                               # speedpitch.SpeedPitch, made by the first call that needs it
        self._drift_scorer = None                              # the caller's drift_scorer, if one was set
        self._drift_native = None                              # (HandcraftedFeatures, DriftForest, scorer) built from drift_model_path
        self.drift_embed = None                                # batch callable (audios, sample_rate) -> [n][k]: the embedding dimensions
        self.drift_optimal_threshold: Optional[float] = None   # the exported file's metadata, known once the file is loaded
        self._lock = threading.RLock()
        self._voice_key = None
        # The voice bank (an extension: the reference holds one voice per instance).  max_voices entries in the engine: the
        # constructor's voice and up to max_voices - 1 named ones (add_voice), which generate(voices=...) / stream(voice=...) name per text.
        if not 1 <= int(max_voices) <= 8:
            raise ValueError(f"max_voices = {max_voices!r}: 1 .. 8")
        self.max_voices = int(max_voices)
        self._bank: Dict[str, tuple] = {}                      # name -> (reference_audio, reference_text, speaker, language)
        self._bank_loaded: Dict[str, tuple] = {}               # name -> the configuration the engine's entry was built from
        self._ge2e_bank: Dict[str, object] = {}                # name -> unit GE2E embedding of the voice's reference clip
        # decode-schedule figures of this instance's engine calls, accumulated until cleared: kept / launched row-frames
        # ("frames" / "padded_frames": their quotient is the row occupancy), rt_generate calls, row hand-overs
        self.last_schedule: Dict[str, int] = {}

    # ---------------------------------------------------------------- native handles
    def _device_ordinal(self) -> int:
        d = str(self.device)
        return int(d.split(":")[1]) if ":" in d else 0

    def _native_ctx(self):
        eng = self._engine
        if eng is not None:
            return eng.ctx
        if self._ctx is None:
            self._ctx = _native.Context(self._device_ordinal())
        return self._ctx

    def _load_engine(self):
        with self._lock:
            if self._engine is None:
                from .engine import Engine
                if self._ctx is not None:
                    self._close_speed_pitch()                  # (they live on the context that goes away here)
                    self._close_drift()
                    self._ctx.close()
                    self._ctx = None
                self._engine = Engine(self.model_path, self._device_ordinal(), max_batch=max(1, min(128, int(self.batch_size))),
                                      max_voices=self.max_voices)
                self._bank_loaded = {}
                self._dp_bank_sent = {}                        # (a new engine holds no bank voice: data-parallel runs broadcast them again)
                # the reference refines the limit from the checkpoint's max_position_embeddings (qwen.py:131-139); a checkpoint
                # without one keeps MAX_MODEL_CHARS.  (The KV allocation - cfg.max_positions - is a separate number.)
                hf_pos = int(getattr(self._engine.cfg, "hf_max_position_embeddings", 0) or 0)
                self._max_model_chars = min(self.MAX_MODEL_CHARS, hf_pos) if hf_pos > 0 else self.MAX_MODEL_CHARS
            return self._engine

    def _voice_config_key(self):
        """The mode checks of QwenTTS._generate_audio (qwen.py:231-242), and what identifies the configured voice."""
        is_custom = "CustomVoice" in self.model_path
        if is_custom and not self.speaker:
            raise ValueError("CustomVoice model requires a named speaker. Select a built-in voice (e.g. Vivian, Ryan) "
                             "or provide reference audio with a Base model for voice cloning.")
        if not is_custom and not self.voice_cloning:
            raise ValueError("Qwen Base model requires reference audio for voice cloning. "
                             "Use a CustomVoice model with a named speaker, or provide reference audio.")
        return (self.speaker, self.language) if is_custom else (self.reference_audio_path, self.reference_text, self.language)

    # ---------------------------------------------------------------- the voice bank
    @property
    def voices(self) -> List[str]:
        """Names of the bank voices (the constructor's voice has none: it is what a text without a voice speaks with)."""
        return sorted(self._bank)

    def add_voice(self, name: str, reference_audio: Optional[str] = None, reference_text: Optional[str] = None,
                  speaker: Optional[str] = None, language: Optional[str] = None) -> None:
        """Register a voice beside the constructor's, by the constructor's mode rules (``_voice_config_key``): a named speaker with a
        CustomVoice model, reference audio and its transcript with a Base model.  It is made resident on the GPU by the first call
        that names it.  ValueError: no name, a mode the model does not have, a full bank."""
        self._no_session("add_voice")
        if not isinstance(name, str) or not name:
            raise ValueError("add_voice: a voice needs a name")
        is_custom = "CustomVoice" in self.model_path
        if is_custom and not speaker:
            raise ValueError("CustomVoice model requires a named speaker. Select a built-in voice (e.g. Vivian, Ryan) "
                             "or provide reference audio with a Base model for voice cloning.")
        if not is_custom and reference_audio is None:
            raise ValueError("Qwen Base model requires reference audio for voice cloning. "
                             "Use a CustomVoice model with a named speaker, or provide reference audio.")
        if reference_audio is not None and reference_text is None:
            raise ValueError("reference_text (transcript of reference audio) is required when reference_audio is set")
        if name not in self._bank and len(self._bank) >= self.max_voices - 1:
            raise ValueError(f"the voice bank is full: {len(self._bank)} named voice(s) beside the constructor's (max_voices={self.max_voices})")
        with self._lock:
            self._bank[name] = (reference_audio, reference_text, speaker, language or self.language)
            self._ge2e_bank.pop(name, None)

    def remove_voice(self, name: str) -> None:
        self._no_session("remove_voice")
        with self._lock:
            if name not in self._bank:
                raise ValueError(f"unknown voice {name!r}")
            del self._bank[name]
            self._ge2e_bank.pop(name, None)
            if name in getattr(self, "_dp_bank_sent", {}):     # (a data-parallel run broadcasts it again if the name comes back)
                self._dp_bank_sent = {k: v for k, v in self._dp_bank_sent.items() if k != name}
            if self._bank_loaded.pop(name, None) is not None and self._engine is not None and name in self._engine.voices:
                self._engine.remove_voice(name)

    def _resolve_voices(self, voices, n: int) -> Optional[List[Optional[str]]]:
        """``voices`` of a call -> one bank name (or None: the constructor's voice) per text, or None when the call names none.
        ValueError before anything is launched: an unknown name, a list of the wrong length."""
        if voices is None:
            return None
        names = [voices] * n if isinstance(voices, str) else list(voices)
        if len(names) != n:
            raise ValueError(f"voices: {len(names)} entries for {n} text(s)")
        for v in names:
            if v is not None and v not in self._bank:
                raise ValueError(f"unknown voice {v!r} (add_voice first; bank: {self.voices})")
        return names if any(v is not None for v in names) else None

    def _ensure_bank(self, eng, names) -> None:
        """The bank voices a call names, resident in the engine (built once per configuration)."""
        for name in sorted({v for v in names if v is not None}):
            cfg = self._bank[name]
            if self._bank_loaded.get(name) == cfg and name in eng.voices:
                continue
            audio, text, speaker, language = cfg
            from .voice import VoiceConditioning
            cond = VoiceConditioning(language, speaker, None, [], None) if "CustomVoice" in self.model_path else \
                eng.conditioning_from_audio(audio, text, language)
            eng.add_voice(name, cond)
            self._bank_loaded[name] = cfg

    def _dp_share_bank(self, td, rank: int, dev, names) -> None:
        """Data-parallel: rank 0 builds each bank voice the call names that the ranks do not hold yet; the others import its prefix
        into the same entry.  The ranks agree by name and configuration, as they do for the constructor's voice by ``_voice_key``."""
        from . import dist as D
        eng = self._load_engine()
        for name in sorted({v for v in names if v is not None}):
            cfg = self._bank[name]
            if getattr(self, "_dp_bank_sent", {}).get(name) == cfg:
                continue
            err = None
            try:
                if rank == 0:
                    with self._lock:
                        self._ensure_bank(eng, [name])
            except BaseException as e:  # noqa: BLE001  (re-raised below, on every rank)
                err = e
            self._dp_agree(td, dev, err, f"voice conditioning of {name!r}")
            index = eng.voices[name][0] if rank == 0 else (eng.voices[name][0] if name in eng.voices else eng.free_voice_entry())
            D.broadcast_voice(eng, td, src=0, comm_device=dev, voice_index=index, name=name)
            self._bank_loaded[name] = cfg
            self._dp_bank_sent = dict(getattr(self, "_dp_bank_sent", {}), **{name: cfg})

    def _dp_share_voice(self, td, rank: int, dev) -> None:
        from . import dist as D
        if self._call_voices is not None:
            self._dp_share_bank(td, rank, dev, self._call_voices)
        eng, err, key = None, None, None
        try:
            eng = self._load_engine()
            key = self._voice_config_key()
            if key != self._voice_key and rank == 0:
                with self._lock:
                    self._ensure_voice(eng)
        except BaseException as e:  # noqa: BLE001  (re-raised below, on every rank)
            err = e
        self._dp_agree(td, dev, err, "voice conditioning")
        # (`_dp_voice_sent` only changes here, on every rank at once - every rank runs the same calls with the same configuration -
        # so the ranks agree on whether the broadcast is due)
        if getattr(self, "_dp_voice_sent", None) != key:
            D.broadcast_voice(eng, td, src=0, comm_device=dev)
            self._voice_key = key
            self._dp_voice_sent = key

    def _ensure_voice(self, eng) -> None:
        is_custom = "CustomVoice" in self.model_path
        key = self._voice_config_key()
        if key == self._voice_key:
            return
        if is_custom:
            eng.set_builtin_voice(self.speaker, self.language)
        else:
            eng.set_voice_from_audio(self.reference_audio_path, self.reference_text, self.language)
        self._voice_key = key

    def _estimate_cost(self, segment: str) -> Optional[float]:
        eng = self._engine
        if eng is not None:
            return float(eng.frames_for(segment, len(eng.tokenizer.encode(segment))))
        return float(max(1, len(segment.split())))

    def _compute_speaker_similarity(self, wav_tensor: torch.Tensor, voice: Optional[str] = None) -> float:
        """Cosine similarity between generated audio and the reference voice (base_tts.py:325-346, which embeds both with
        resemblyzer on the CPU and is never called by the reference's own pipeline).  Here both embeddings come from the model's
        OWN speaker encoder on the GPU - the statistics-pooling head of the audio encoder that also conditions the talker
        (rt_voice_encode) - so the score says how close the output is in the space the model itself clones from.  Not comparable
        in value with resemblyzer's; same range and direction (1 = same voice).
        With ``speaker_similarity="ge2e"`` it is the reference's arithmetic instead: the dot product of the unit GE2E embeddings
        (speaker.SpeakerEmbedder) of the reference clip and of the output; the reference clip's embedding is cached per voice.
        ``voice``: the bank voice the audio was generated with (None: the constructor's) - the comparison is against that voice's
        own reference."""
        self._resolve_voices(voice, 1)
        if self.speaker_similarity == "ge2e":
            return self._ge2e_similarity(wav_tensor, voice)
        eng = self._load_engine()
        with self._lock:
            if voice is None:
                self._ensure_voice(eng)
                ref = None if eng.voice is None else eng.voice.speaker_embed
            else:
                self._ensure_bank(eng, [voice])
                ref = eng.voices[voice][1].speaker_embed
            if ref is None:
                raise ValueError("speaker similarity needs a cloned voice (reference audio with a Base model)")
            pcm = wav_tensor.detach().to(torch.float32).reshape(-1).cpu().numpy()
            cap = eng.model.rt_cfg.enc.max_ref_frames * eng.cfg.codec.total_upsample     # (samples the encoder's frame budget covers)
            _, emb = eng.model.encode_voice(pcm[:cap])
        ref = ref.detach().to(torch.float32).cpu().reshape(-1)
        return float(torch.dot(ref, emb) / (ref.norm() * emb.norm()).clamp_min(1e-12))

    def _ge2e_reference_audio(self, voice: Optional[str] = None):
        """(samples, sample rate) of the configured reference clip, as the voice cloning reads it."""
        clip = self.reference_audio_path if voice is None else self._bank[voice][0]
        if not clip:
            raise ValueError("speaker similarity needs a cloned voice (reference audio with a Base model)")
        import wave
        from .voice import load_audio
        path = str(clip)
        sr = self.sample_rate                                  # (a .npy clip is at the model's rate, as the cloning path takes it)
        if not path.endswith(".npy"):
            with wave.open(path, "rb") as wf:
                sr = int(wf.getframerate())                    # the file's own rate: the encoder's resampler brings it to 16 kHz
        return torch.from_numpy(load_audio(path, sr)), sr

    def _ge2e_similarity(self, wav_tensor: torch.Tensor, voice: Optional[str] = None) -> float:
        with self._lock:
            emb = self._speaker_embed()
            if voice is not None:                              # a bank voice: its reference embedding is cached under its name
                if voice not in self._ge2e_bank:
                    ref_pcm, ref_sr = self._ge2e_reference_audio(voice)
                    self._ge2e_bank[voice] = emb(ref_pcm, ref_sr).astype("float64")
                ref = self._ge2e_bank[voice]
            else:
                key = (self.reference_audio_path,)
                if self._ge2e_ref is None or self._ge2e_ref[0] != key:
                    ref_pcm, ref_sr = self._ge2e_reference_audio()
                    self._ge2e_ref = (key, emb(ref_pcm, ref_sr).astype("float64"))
                ref = self._ge2e_ref[1]
            out = emb(wav_tensor.detach().reshape(-1), self.sample_rate).astype("float64")
            return float(ref @ out)

    def _cut_batches(self, todo: List[int], work, bs: int) -> List[List[int]]:
        """The engine decodes any number of segments on its ``batch_size`` rows with continuous batching (finished rows are handed
        to the next queued segment, Engine.synthesize): the whole work list goes down in one call instead of being cut here."""
        if len(todo) > bs and bs <= 128:
            return [list(todo)]
        return super()._cut_batches(todo, work, bs)

    # ---------------------------------------------------------------- provider contract
    def _generate_audio(self, text: Union[str, List[str]], **kwargs) -> Union[torch.Tensor, List[torch.Tensor]]:
        self._no_session("_generate_audio")
        single = isinstance(text, str)
        texts = [text] if single else list(text)
        eng = self._load_engine()
        token = kwargs.get("cancellation_token")
        flag = C.c_int32(0)
        stop = threading.Event()
        watcher = None
        if token is not None:                                   # forward CancellationToken.cancel() into the native frame loop
            def watch():
                while not stop.wait(0.02):
                    if token.is_cancelled():
                        flag.value = 1
                        return
            watcher = threading.Thread(target=watch, daemon=True)
            watcher.start()
        try:
            with self._lock:
                names = self._resolve_voices(kwargs.get("voices"), len(texts))
                if names is None or any(v is None for v in names):
                    self._ensure_voice(eng)
                if names is not None:
                    self._ensure_bank(eng, names)
                wavs = eng.synthesize(texts, seed=int(self.seed), item_ids=kwargs.get("item_ids"), cancel_flag=flag, stats=self.last_schedule,
                                      voices=names)
        except _native.CancelledError as e:
            raise CancelledException(str(e))
        finally:
            stop.set()
            if watcher is not None:
                watcher.join(timeout=1.0)
        return wavs[0] if single else wavs

    def generate(self, texts, output_path: Optional[str] = None, cancellation_token: Optional[CancellationToken] = None,
                 format: str = "wav", speed: float = 1.0, pitch_semitones: float = 0.0, progress_callback: Optional[Callable[[str], None]] = None,
                 voices=None):
        """``BaseTTS.generate`` (base_tts.py:960-1101), inherited unchanged - except on the WORKER ranks of a data-parallel run
        (DataParallelPipeline): those do their share of the texts, deliver it to rank 0 and return nothing (``None`` for one
        text, a list of ``None`` for a list) without writing any file; rank 0 returns and saves everything.
        ``voices`` (an extension): a bank name for every text, or a list as long as ``texts`` whose ``None`` entries mean the
        constructor's voice; the segments of a text speak with its voice.  ValueError before anything runs: an unknown name, a list
        of the wrong length."""
        self._no_session("generate")
        n_texts = 1 if isinstance(texts, str) else len(texts)
        names = self._resolve_voices(voices, n_texts)
        if names is None:
            return self._generate_call(texts, output_path, cancellation_token, format, speed, pitch_semitones, progress_callback)
        with self._lock:                                        # (the call's voices are instance state while the inherited body runs)
            self._call_voices = names
            try:
                return self._generate_call(texts, output_path, cancellation_token, format, speed, pitch_semitones, progress_callback)
            finally:
                self._call_voices = None

    def _generate_call(self, texts, output_path, cancellation_token, format, speed, pitch_semitones, progress_callback):
        dp = self._dp()
        if dp is None or dp[1] == 0:
            return super().generate(texts, output_path, cancellation_token, format, speed, pitch_semitones, progress_callback)
        if format not in ("wav", "mp3", "flac", "ogg"):          # the check rank 0 makes before it enters the pipeline (base_tts.py:996-999)
            from .api import FormatConversionError
            raise FormatConversionError(f"Unsupported format '{format}'. Supported: flac, mp3, ogg, wav")
        single = isinstance(texts, str)
        try:
            self._run_pipeline([texts] if single else list(texts), cancellation_token or CancellationToken(), progress_callback)
        except CancelledException as e:
            logger.warning(f"Generation cancelled: {e}")
        except ValueError:
            raise
        except Exception as e:  # noqa: BLE001  (as the inherited generate does: log, return nothing)
            logger.error(f"Error in TTS generation: {e}")
        return None if single else [None] * len(texts)

    def stream(self, text: str, cancellation_token: Optional[CancellationToken] = None, speed: float = 1.0,
               pitch_semitones: float = 0.0, voice: Optional[str] = None):
        """``BaseTTS.stream`` (base_tts.py:1132-1190): one result per segment, no crossfade, failed segments skipped - with the
        same audio per segment, produced in two calls instead of one per segment: the FIRST segment alone (time to first
        audio = one short decode), then ALL the others in one batched call while the caller is busy with the first.
        Every segment keeps RNG stream 0, which is what a one-segment ``_generate_audio`` call uses, so the results equal the
        sequential loop's."""
        from .api import GenerationResult
        self._no_session("stream")
        token = cancellation_token or CancellationToken()
        self._resolve_voices(voice, 1)                          # (``voice``: a bank name; ValueError for an unknown one before anything runs)
        vkw = {} if voice is None else {"voices": voice}
        segments = self._split_text_into_segments(self._apply_phonetic_mapping(text), self._compute_max_chars())
        if int(getattr(self, "stream_chunk_frames", 0) or 0) > 0:
            if voice is not None:
                raise ValueError("sub-segment streaming (stream_chunk_frames) speaks with the constructor's voice only")
            yield from self._stream_chunks(segments, token, speed, pitch_semitones)
            return

        def finish(raw: torch.Tensor):
            audio = self._post_process_audio(raw)
            audio = self._apply_fades(self._remove_dc_offset(self._trim_silence(audio, True, True)), True, True)
            if speed != 1.0 or pitch_semitones != 0.0:
                audio = self._apply_speed_pitch(audio, speed, pitch_semitones)
            n_samples = audio.shape[-1] if audio.dim() == 2 else audio.numel()
            return GenerationResult(audio=audio, sample_rate=self.sample_rate, duration_sec=n_samples / self.sample_rate,
                                    segments_count=1, format="wav")

        for first, group in ((0, segments[:1]), (1, segments[1:])):
            if not group or token.is_cancelled():
                continue
            self._set_seeds()
            try:
                raws: List[Optional[torch.Tensor]] = list(self._generate_audio(list(group), item_ids=[0] * len(group), cancellation_token=token, **vkw))
            except CancelledException:
                return
            except Exception as first_error:  # noqa: BLE001  (the batch failed: let every segment fail or pass on its own)
                raws = []
                for seg in group:
                    try:
                        raws.append(self._generate_audio(seg, cancellation_token=token, **vkw))
                    except CancelledException:
                        return
                    except Exception as e:  # noqa: BLE001
                        logger.warning(f"Segment {first + len(raws) + 1} failed: {e} (batched call: {first_error})")
                        raws.append(None)
            for k, raw in enumerate(raws):
                if token.is_cancelled():
                    return
                if raw is None:
                    continue
                try:
                    yield finish(raw)
                except Exception as e:  # noqa: BLE001
                    logger.warning(f"Segment {first + k + 1} failed: {e}")

    # Opt-in SUB-SEGMENT streaming (an extension: the reference hands audio over per segment): with ``stream_chunk_frames`` = n > 0,
    # ``stream()`` yields the first n codec frames of a segment (n x 80 ms of audio) as soon as they are decoded and vocoded, then
    # the rest in pieces of ``stream_next_chunk_frames`` while the decode goes on - one GenerationResult per piece, to be played
    # back to back.  Loudness gain and DC offset are taken from a segment's first piece and kept (rt_stream_chunk); trims and
    # fades happen at the segment's two ends only.
    stream_chunk_frames = 0
    stream_next_chunk_frames = 36

    def _stream_chunks(self, segments, token, speed, pitch_semitones):
        from .api import GenerationResult
        eng = self._load_engine()
        params = self._post_params(0)
        for seg_idx, seg in enumerate(segments):
            if token.is_cancelled():
                return
            self._set_seeds()
            flag = C.c_int32(0)
            state = [0.0, 1.0]
            try:
                with self._lock:
                    self._ensure_voice(eng)
                    started = False                                  # audible audio of this segment has been handed out
                    for raw, last in eng.stream_wav(seg, seed=int(self.seed), item_id=0, first_chunk=int(self.stream_chunk_frames),
                                                    chunk=int(self.stream_next_chunk_frames), cancel_flag=flag):
                        if token.is_cancelled():
                            flag.value = 1
                            return
                        audio = self._native_ctx().stream_chunk(params, raw, state, first=not started, last=last) if raw.numel() else raw
                        if not started and raw.numel():
                            if state[1] > 0.0:
                                started = True
                            else:                                    # a chunk of lead-in silence: nothing measured, nothing to play -
                                continue                             # the next chunk is the segment's first (gain, trim, fade-in)
                        if audio.numel() == 0:
                            continue
                        if speed != 1.0 or pitch_semitones != 0.0:
                            audio = self._apply_speed_pitch(audio, speed, pitch_semitones)
                        n_samples = audio.shape[-1] if audio.dim() == 2 else audio.numel()
                        yield GenerationResult(audio=audio, sample_rate=self.sample_rate, duration_sec=n_samples / self.sample_rate,
                                               segments_count=1, format="wav")
            except _native.CancelledError:
                return
            except Exception as e:  # noqa: BLE001  (as the reference: a failed segment is skipped, base_tts.py:1166-1168)
                logger.warning(f"Segment {seg_idx + 1} failed: {e}")

    # ---------------------------------------------------------------- serving sessions (an extension)
    _session = None                                            # the serving session in flight (serve), which owns the engine's run

    def _no_session(self, what: str) -> None:
        s = self._session
        if s is not None and not s.is_worker():
            raise RuntimeError(f"{what}: a serving session is open on this instance and owns its decode rows - submit the text to the "
                               "session, or close it first")

    def serve(self, rows: Optional[int] = None, voices: Optional[Sequence[str]] = None, stream_chunk_frames: int = 12,
              stream_next_chunk_frames: int = 36, max_text_tokens: int = 256, horizon: int = 4096, timeout: float = 120.0):
        """A serving session: requests join ONE decode batch in flight instead of queueing behind each other's calls.

            with tts.serve(voices=["b"]) as session:
                h1 = session.submit("A text", stream=True)            # any thread
                h2 = session.submit("Another one", voice="b")
                for piece in h1: ...                                  # GenerationResults, as stream() yields them
                result = h2.result(timeout=30)                        # the GenerationResult generate() returns

        The constructor's voice and the bank voices ``voices`` are made resident and the run is opened on ``rows`` decode rows
        (default: ``batch_size``); one worker thread drives it (serving.Session).  ``handle.result()`` is what ``generate(text,
        voices=voice)`` returns for that text alone with ``max_iterations == 1`` (no validation loop and no decay retry in a session,
        as in ``stream()``); iterating a ``stream=True`` handle yields the pieces of sub-segment streaming with the two chunk sizes -
        with a bank voice too.  A request's audio is bit for bit what it gets alone, whoever else is connected.  A segment of more
        than ``max_text_tokens`` tokens fails its request (``ValueError``).  ``horizon``: the frame-counter values of one run - when
        they are spent the worker drains the run, opens another and goes on with the queue; callers see nothing of it.  While the
        session is open ``generate`` / ``stream`` / ``add_voice`` on this instance raise; closing it (leaving the ``with`` block)
        cancels pending requests - their handles raise - and restores them.  Every wait has a timeout (``timeout`` seconds unless
        the call gives one) that raises ``TimeoutError``."""
        from .serving import EngineRun, Session
        self._no_session("serve")
        names = [v for v in (voices or []) if v is not None]
        eng = self._load_engine()
        with self._lock:
            if self._session is not None:
                raise RuntimeError("serve: a serving session is already open on this instance")
            self._resolve_voices(names or None, len(names))
            self._ensure_voice(eng)
            self._ensure_bank(eng, names)
            self._set_seeds()
            run = EngineRun(self, eng, rows, [None] + sorted(set(names)), int(max_text_tokens), None, int(horizon))

            def release():
                self._session = None
            session = Session(run, int(stream_chunk_frames), int(stream_next_chunk_frames), float(timeout), on_close=release)
            self._session = session
        return session

    def _apply_speed_pitch(self, audio: torch.Tensor, speed: float, pitch_semitones: float) -> torch.Tensor:
        """``BaseTTS._apply_speed_pitch`` (base_tts.py:618-650) on the GPU, without torchaudio: the resampler and the phase-vocoder
        pitch shift of csrc/speedpitch.hip (speedpitch.py), on this provider's context.  Reached only with ``speed != 1`` or
        ``pitch_semitones != 0`` (generate / stream test that first, base_tts.py:1020)."""
        if speed == 1.0 and pitch_semitones == 0.0:
            return audio
        with self._lock:
            if self._speed_pitch is None:                      # (released with the context it is made on: _load_engine, close)
                from .speedpitch import SpeedPitch
                self._speed_pitch = SpeedPitch(self._native_ctx())
            return self._speed_pitch(audio, speed, pitch_semitones, sample_rate=self.sample_rate)

    def _close_speed_pitch(self) -> None:
        if self._speed_pitch is not None:
            self._speed_pitch.close()
            self._speed_pitch = None

    # ---------------------------------------------------------------- drift validation from an exported classifier
    @property
    def drift_scorer(self):
        """The tensor-level drift hook (BatchedPipeline): the caller's when one was set; else, when ``drift_model_path`` names an
        exported classifier (``.npz``, tools/export_drift_classifier.py), the native one - feature extractor and forest on this
        provider's context, built at first use; else None, and nothing changes."""
        if self._drift_scorer is not None or not self.drift_model_path:
            return self._drift_scorer
        return self._native_drift_scorer()

    @drift_scorer.setter
    def drift_scorer(self, scorer) -> None:
        self._drift_scorer = scorer

    def _native_drift_scorer(self):
        """HandcraftedFeatures + DriftForest + make_forest_scorer for ``drift_model_path``.  A configuration that cannot work is a
        ``ValueError`` at first use, never a silently skipped check.  ``accent_drift_threshold`` stays the caller's: the file's
        ``optimal_threshold`` is metadata, as in the reference, offered as ``drift_optimal_threshold``."""
        with self._lock:
            if self._drift_native is not None:
                return self._drift_native[2]
            path = str(self.drift_model_path)
            if not path.lower().endswith(".npz"):
                raise ValueError(f"drift_model_path = {path!r}: this provider never unpickles a model.  Export the classifier once with "
                                 "`python tools/export_drift_classifier.py IN.pkl OUT.npz` and point drift_model_path at the .npz")
            from . import forest as F
            from .features import HandcraftedFeatures, make_forest_scorer
            tables = F.load(path)
            width = int(tables["n_features"])
            embed = self.drift_embed
            if embed is None and self.speaker_encoder_path and width != F.HANDCRAFTED:
                embed = self._speaker_embed()                  # (a list of clips -> [n][256], dim = 256): one embedding call per chunk
            if width != F.HANDCRAFTED and embed is None:
                raise ValueError(f"drift_model_path = {path!r} takes {width} features: the {width - F.HANDCRAFTED} dimensions in front of the "
                                 f"{F.HANDCRAFTED} hand-crafted ones are the speaker embedding, which this provider does not compute - set "
                                 "drift_embed to a batch callable (audios, sample_rate) -> [n][k]")
            if width == F.HANDCRAFTED and self.drift_embed is not None:
                raise ValueError(f"drift_model_path = {path!r} takes {width} features, all hand-crafted: drift_embed has no place in it")
            ctx = self._native_ctx()
            ex = forest = None
            try:
                ex = HandcraftedFeatures(ctx)
                forest = F.DriftForest(ctx, tables)
                scorer = make_forest_scorer(ex, forest, embed)
            except Exception:
                for h in (forest, ex):
                    if h is not None:
                        h.close()
                raise
            self._drift_native = (ex, forest, scorer)
            self.drift_optimal_threshold = float(tables["optimal_threshold"])
            return scorer

    def train_drift_classifier(self, dataset_dir: str, voice_id: Optional[str] = None, output_path: Optional[str] = None,
                               progress_callback=None) -> str:
        """The reference's ``train_drift_classifier`` (__init__.py:69) on this provider's context: ``forest_train.train`` over
        ``dataset_dir/good`` and ``dataset_dir/bad`` - the folders ``_auto_sort_audio`` fills - with the rows the validation will see:
        [256 GE2E | 30 hand-crafted] when ``speaker_encoder_path`` (or ``drift_embed``) is configured, the 30 alone otherwise.  Then
        ``drift_model_path`` points at the written ``.npz`` and the cached native scorer is dropped, so the next validation scores with
        the new model.  Returns the path.  Nothing changes unless this is called."""
        from . import forest_train
        with self._lock:
            embed = self.drift_embed
            if embed is None and self.speaker_encoder_path:
                embed = self._speaker_embed()
            path = forest_train.train(dataset_dir, voice_id=voice_id, output_path=output_path, progress_callback=progress_callback,
                                      ctx=self._native_ctx(), embed=embed)
            if self._drift_native is not None:                 # (the speaker embedder stays: the next scorer uses it again)
                ex, forest, _ = self._drift_native
                self._drift_native = None
                forest.close()
                ex.close()
            self.drift_model_path = path
            self.drift_optimal_threshold = None
            return path

    def _close_drift(self) -> None:
        if self._drift_native is not None:
            ex, forest, _ = self._drift_native
            self._drift_native = None
            forest.close()
            ex.close()
        if self._speaker_embedder is not None:                 # (it lives on the same context)
            self._speaker_embedder.close()
            self._speaker_embedder = None

    def _speaker_embed(self):
        """The GE2E encoder of ``speaker_encoder_path`` on this provider's context, built at first use."""
        with self._lock:
            if self._speaker_embedder is None:
                if not self.speaker_encoder_path:
                    raise ValueError("no speaker_encoder_path: the GE2E speaker encoder is not configured")
                from .speaker import SpeakerEmbedder
                self._speaker_embedder = SpeakerEmbedder(self._native_ctx(), str(self.speaker_encoder_path))
            return self._speaker_embedder

    @property
    def sample_rate(self) -> int:
        return 24000 if self._engine is None else self._engine.cfg.sample_rate

    def word_times(self, audio: torch.Tensor, text):
        """When each word of ``text`` (a string, or token ids) is spoken in ``audio`` (one window of generated audio at ``sample_rate``):
        the transcriber's forced alignment (stt.WhisperTranscriber.align), a list of stt.SttWord with times in seconds - for captions,
        highlighting and lip-sync.  The text is the known target, so the result does not depend on what a transcription would hear."""
        align = getattr(getattr(self, "transcriber", None), "align", None)
        if align is None:
            raise ValueError("word_times needs a transcriber with forced alignment: set `transcriber` to a stt.WhisperTranscriber "
                             "(the option that is missing: transcriber=WhisperTranscriber(...))")
        return align([audio], self.sample_rate, [text])[0]

    def close(self) -> None:
        if self._session is not None:
            self._session.close()
        with self._lock:
            self._close_speed_pitch()                          # (before the context they live on)
            self._close_drift()
            if self._engine is not None:
                self._engine.close()
                self._engine = None
            if self._ctx is not None:
                self._ctx.close()
                self._ctx = None
        if torch.cuda.is_available():
            torch.cuda.empty_cache()

    @classmethod
    def provider_info(cls) -> ProviderInfo:
        return ProviderInfo(name=PROVIDER_NAME, supports_voice_cloning=True,
                            supported_languages=["English", "Chinese", "Japanese", "Korean"],
                            builtin_voices=[VoiceInfo(id=v, name=v, language="English") for v in BUILTIN_VOICES])


def register(name: str = PROVIDER_NAME) -> str:
    """``TTSFactory.register_provider(name, MI355XQwenTTS)`` on whichever host API is active (see api.py)."""
    TTSFactory.register_provider(name, MI355XQwenTTS)
    return name

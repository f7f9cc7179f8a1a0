"""The provider end to end on the GPU: reference pipeline fixtures with the HIP leaves, and the real
model path (tiny config) through generate() / stream() / factory registration."""
import json
import os
import wave

import numpy as np
import pytest
import torch

from oracle import postprocess as OP
from rho_tts_amd import api, config
from rho_tts_amd.provider import BatchedPipeline, HipAudioLeaves, MI355XQwenTTS, register

pytestmark = pytest.mark.gpu
SR = 24000

from tests.test_pipeline_host import fake_wave, run, same  # noqa: E402


class HipFake(BatchedPipeline, HipAudioLeaves, api.BaseTTS):
    """Reference-style fake generator + the HIP post-processing leaves."""

    def __init__(self, batch_size=4, device="cpu"):
        super().__init__(device=device)
        self.batch_size, self.calls, self.out_device = batch_size, [], device
        from rho_tts_amd import _native
        self._c = _native.Context(0)

    def _native_ctx(self):
        return self._c

    def _generate_audio(self, text, **kw):
        texts = [text] if isinstance(text, str) else list(text)
        self.calls += texts
        out = [torch.from_numpy(fake_wave(t)).to("cuda" if self.out_device != "cpu" else "cpu") for t in texts]
        return out[0] if isinstance(text, str) else out

    def _finish_items(self, items):          # the reference's fake has no loudness stage (base _post_process_audio is a no-op)
        from rho_tts_amd import _native
        outs, stats = self._post([list(i) for i in items], _native.POST_PIPELINE & ~_native.POST_LOUDNESS)
        return [(o, s.decay_ratio, bool(s.decay_ok)) for o, s in zip(outs, stats)]

    @property
    def sample_rate(self):
        return SR


def rec(res):
    out = []
    for r in res:
        a, nseg, meta = r
        a = a.reshape(-1).cpu().numpy()
        out.append({"len": int(a.shape[0]), "segments": int(nseg), "abs_sum": float(np.abs(a.astype(np.float64)).sum()),
                    "decay_ratio": float(meta["decay_ratio"]), "meta_keys": sorted(meta.keys())})
    return out


@pytest.mark.parametrize("dev", ["cpu", "cuda"])
def test_reference_pipeline_fixtures_with_hip_leaves(golden_pipe, dev):
    g = golden_pipe
    for case, setup in (("single_one_segment", {}), ("three_segments_forced", {}),
                        ("max_chars_30", {"force_sentence_split": False, "max_chars_per_segment": 30})):
        t = HipFake(device=dev)
        t._max_chars_explicit = True
        for k, v in setup.items():
            setattr(t, k, v)
        got = rec(t._run_pipeline(g[case]["texts"], api.CancellationToken()))
        for a, w in zip(got, g[case]["out"]):
            assert a["len"] == w["len"] and a["segments"] == w["segments"]
            assert abs(a["abs_sum"] - w["abs_sum"]) < 1e-5 * w["abs_sum"]
            assert abs(a["decay_ratio"] - w["decay_ratio"]) < 1e-5
        assert t.calls == g[case]["calls"]


def test_leaf_methods_behave_like_the_reference(golden_post):
    t = HipFake()
    x = torch.from_numpy(golden_post["leaf/k1/x"])
    assert t._trim_silence(x).shape == (24240,)
    assert t._trim_silence(x.unsqueeze(0)).shape == (24240,)                    # 2-D in -> 1-D out (base_tts.py:392)
    assert t._trim_silence(torch.zeros(24000)).shape == (1, 240)                # all-silent quirk (:379-380)
    assert abs(float(t._remove_dc_offset(x).mean())) < 1e-7
    f = t._apply_fades(torch.ones(2000))
    assert float(f[0]) < 0.01 and float(f[-1]) < 0.01 and float(f[1000]) == 1.0
    assert t._apply_fades(torch.ones(100)).tolist() == [1.0] * 100              # shorter than two fades: untouched
    assert t._smooth_segment_join([]) is None
    r, ok = t._validate_sound_decay(torch.from_numpy(golden_post["loud/k4/x"]))
    assert abs(r - 0.393182) < 1e-5 and ok
    assert t._validate_sound_decay(torch.zeros(0)) == (1.0, True)
    t.trim_silence = False
    assert t._trim_silence(x).shape == x.shape


@pytest.fixture(scope="module")
def tiny_provider(tmp_path_factory):
    d = tmp_path_factory.mktemp("voice")
    ref = d / "ref.wav"
    i = np.arange(SR * 2)
    pcm = (0.3 * np.sin(2 * np.pi * 150 * i / SR) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * i / SR)) * 32767).astype("<i2")
    with wave.open(str(ref), "wb") as wf:
        wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(SR); wf.writeframes(pcm.tobytes())
    saved = dict(api.TTSFactory._providers)
    name = register()
    p = api.TTSFactory.get_tts_instance(name, reference_audio=str(ref), reference_text="a short reference sentence",
                                        model_path="tiny", batch_size=4)
    yield p
    p.close()
    api.TTSFactory._providers = saved


def test_generate_through_the_factory(tiny_provider, tmp_path):
    p = tiny_provider
    assert isinstance(p, MI355XQwenTTS) and p.voice_cloning
    r = p.generate("Hello there general test of the path")
    assert isinstance(r, api.GenerationResult) and r.sample_rate == 24000 and r.segments_count == 1
    assert r.audio.dim() == 1 and r.audio.numel() > 100 and r.decay_ratio is not None
    assert abs(r.duration_sec - r.audio.numel() / 24000) < 1e-9
    rms_db = 20 * np.log10(float(torch.sqrt(torch.mean(r.audio.float() ** 2))) + 1e-12)
    assert abs(rms_db + 23.0) < 1.0 and float(r.audio.abs().max()) <= 0.95       # loudness stage ran
    texts = [f"Sentence number {i} with some more words in it" for i in range(6)]
    rs = p.generate(texts, output_path=str(tmp_path / "o"))
    assert len(rs) == 6 and all(x is not None and os.path.exists(x.path) for x in rs)
    again = p.generate(texts)
    for a, b in zip(rs, again):
        assert torch.equal(a.audio.cpu(), b.audio.cpu())                         # same seed, same texts -> same audio
    p.seed = 790
    other = p.generate(texts[:2])
    assert not torch.equal(other[0].audio.cpu(), rs[0].audio.cpu())
    p.seed = 789


def test_speaker_similarity_on_the_models_own_encoder(tiny_provider):
    """_compute_speaker_similarity (base_tts.py:325-346) on the GPU speaker encoder: the reference clip against itself is 1,
    a different signal scores lower, the value is a cosine."""
    p = tiny_provider
    with wave.open(p.reference_audio_path, "rb") as wf:
        ref = np.frombuffer(wf.readframes(wf.getnframes()), "<i2").astype(np.float32) / 32768.0
    same = p._compute_speaker_similarity(torch.from_numpy(ref))
    assert abs(same - 1.0) < 1e-4, same
    g = torch.Generator().manual_seed(5)
    noise = 0.1 * torch.randn(SR, generator=g)
    other = p._compute_speaker_similarity(noise.cuda())
    assert -1.0 <= other < same - 1e-3, other


def test_batched_equals_one_at_a_time(tiny_provider):
    p = tiny_provider
    texts = ["Alpha beta gamma delta", "One two", "A somewhat longer piece of text to speak here"]
    # 3 texts: one static batch.  11 texts on 4 rows: ONE continuous-batching call (finished rows handed to queued texts)
    texts = texts + [" ".join(["word"] * k) + f" number {k}" for k in (9, 1, 14, 3, 6, 2, 11, 5)]
    both = p.generate(texts)
    assert p._engine.model.generate_stats()["hand_overs"] >= 1
    p.batch_size = 1
    try:
        single = p.generate(texts)
    finally:
        p.batch_size = 4
    for a, b in zip(both, single):
        assert torch.equal(a.audio.cpu(), b.audio.cpu())


def test_stream_cancel_and_config_errors(tiny_provider):
    p = tiny_provider
    p.max_chars_per_segment, p._max_chars_explicit, p.force_sentence_split = 30, True, True
    try:
        parts = list(p.stream("First sentence here. Second sentence there. Third one."))
    finally:
        p.max_chars_per_segment, p._max_chars_explicit, p.force_sentence_split = 1000, False, False
    assert len(parts) == 3 and all(x.segments_count == 1 and x.audio.numel() > 0 for x in parts)
    # the provider streams in two calls (first segment alone, the others batched): same audio as the per-segment loop of BaseTTS.stream
    p.max_chars_per_segment, p._max_chars_explicit, p.force_sentence_split = 30, True, True
    try:
        ref_parts = list(api.BaseTTS.stream(p, "First sentence here. Second sentence there. Third one."))
    finally:
        p.max_chars_per_segment, p._max_chars_explicit, p.force_sentence_split = 1000, False, False
    assert len(ref_parts) == 3
    for a, b in zip(parts, ref_parts):
        assert torch.equal(a.audio.cpu(), b.audio.cpu())
    tok = api.CancellationToken()
    tok.cancel()
    assert p.generate("Anything", cancellation_token=tok) is None
    q = MI355XQwenTTS(model_path="tiny")                                          # Base model without reference audio
    with pytest.raises(ValueError):
        q.generate("Hello")
    q.close()
    c = MI355XQwenTTS(model_path="CustomVoice-tiny", speaker="Ryan")
    r = c.generate("Built in voice")
    assert r is not None and r.audio.numel() > 0
    c.close()


def test_checkpoint_directory_gives_the_same_audio_as_the_synthetic_state(tmp_path):
    """a3: the loader path a real checkpoint takes (safetensors shards + config.json in a local directory, qwen.py:96-197) yields
    the same model as the in-memory synthetic state it was written from: identical codes and waveforms at fixed lengths; and
    with end-of-sequence live (what a real checkpoint decodes with) generation stays within its frame budget."""
    from rho_tts_amd import weights
    from rho_tts_amd.engine import Engine
    cfg = config.tiny()
    d = str(tmp_path / "tiny-CustomVoice")
    weights.save_checkpoint(cfg, weights.synthetic_state(cfg, 789), d, shard_bytes=300_000)
    texts = ["Hello there general test.", "One sentence only", "A third and rather longer sentence follows here."]
    frames = [7, 5, 9]
    a = Engine(d, device_ordinal=0, max_batch=4)
    try:
        assert not a.synthetic and a.cfg == cfg
        a.ignore_eos = True
        a.set_builtin_voice("ryan")
        wa = [w.cpu() for w in a.synthesize(texts, seed=5, max_frames=frames)]
        a.ignore_eos = None                                  # as a checkpoint decodes: stop at EOS, budget 8 + 6 frames per token
        live = a.generate_codes(texts, seed=5)
        for t, c in zip(texts, live):
            assert 0 <= c.shape[0] <= a.frames_for(t, len(a.tokenizer.encode(t)))
    finally:
        a.close()
    b = Engine("tiny", device_ordinal=0, max_batch=4, synthetic=True)
    try:
        b.set_builtin_voice("ryan")
        wb = [w.cpu() for w in b.synthesize(texts, seed=5, max_frames=frames)]
    finally:
        b.close()
    assert all(torch.equal(x, y) for x, y in zip(wa, wb))
    # ... and through the provider (model path containing "CustomVoice" -> built-in speaker, qwen.py:231)
    tts = MI355XQwenTTS(model_path=d, speaker="Ryan", batch_size=4)
    try:
        res = tts.generate(texts[:2])
        assert res is not None and all(r is not None and r.audio.numel() > 0 for r in res)
    finally:
        tts.close()


def test_eos_checked_every_k_frames_equals_every_frame():
    """End-of-sequence flags live on the device; the host looks at them every 8 frames (rt_debug_tune 1408) instead of copying
    and waiting every frame (1401).  Same codes and lengths either way, with forced and with sampled EOS."""
    from rho_tts_amd import _native, weights
    from rho_tts_amd._native_model import NativeModel, RtSampling
    cfg = config.tiny()
    ctx = _native.Context(0)
    nm = NativeModel(ctx, cfg, max_batch=8)
    try:
        nm.load_state({k: v.cuda() for k, v in weights.synthetic_state(cfg, 789).items()})
        nm.set_voice("chinese", "ryan", None, [], None)
        G = cfg.n_groups
        g = torch.Generator().manual_seed(3)
        texts = [[int(v) for v in torch.randint(0, 400, (int(n),), generator=g)] for n in (3, 5, 2, 7, 4)]
        frames = [30, 21, 12, 26, 30]
        eos = cfg.codec_eos_id
        forced = [torch.randint(0, 60, (f, G), generator=g) for f in frames]
        forced[0][17, 0] = eos                          # ends at frame 17 (not a multiple of 8)
        forced[1][8, 0] = eos                           # ends exactly at a check boundary
        forced[3][3, 0] = eos
        out = {}
        for every in (1, 8, 5):
            nm.lib.rt_debug_tune(1400 + every, 0)
            out[every] = (nm.generate(texts, frames, RtSampling(0, 1, 1, 1, 1), ignore_eos=False, forced_codes=forced),
                          nm.generate(texts, frames, RtSampling(1, 1.5, 64, 1.0, 1.0), seed=11, ignore_eos=False, min_frames=2))
        assert [c.shape[0] for c in out[1][0]] == [17, 8, 12, 3, 30]
        for every in (8, 5):
            for a, b in zip(out[1], out[every]):
                assert all(torch.equal(x, y) for x, y in zip(a, b))
    finally:
        nm.lib.rt_debug_tune(1408, 0)
        nm.close()
        ctx.close()


def test_bench_collective_path_on_rccl_with_one_rank(tmp_path):
    """bench.py's multi-GPU step - RCCL broadcast of the voice-prefix KV blob, length all-gather, padded gather of the
    waveforms, MAX all-reduce of the step time - launched exactly as the driver launches it (torch.distributed.run, backend
    nccl = RCCL), with the one rank a one-GPU box has.  The N > 1 logic is covered by the world-size-2 gloo tests; this one
    proves every collective call is accepted by the RCCL backend on the hardware."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RHO_TTS_AMD_FORCE_DIST="1", MASTER_ADDR="127.0.0.1")
    for corpus in ([], ["--corpus", "24"]):
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                            "--master-port", "29533", os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", "--model",
                            "small" if corpus else "tiny",                      # (the corpus' 24-word texts need more KV rows than `tiny` has)
                            "--batch", "4", "--ref-seconds", "1", "--no-cpu-baseline", "--no-roofline"] + corpus,
                           cwd=root, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-3000:]
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["n_gpus"] == 1 and line["value"] > 0 and line["scaling"] == ("strong" if corpus else "weak")


def test_c4_corpus_through_the_provider():
    """VERDICT r2 #1b: BASELINE.json configs[3] at ITS size on one GPU - 512 ragged texts (6-24 words) on the 1.7B preset with
    the 30-s clone prefix, through ``MI355XQwenTTS.generate`` in data-parallel mode on an RCCL process group (one rank; the
    N > 1 logic is the world-size-2 gloo test of tests/test_dist_cpu.py): complete, in corpus order, row occupancy >= 0.9 with
    the lengths as estimated AND with every text ending within +-30 % of its estimate, and sampled items bit-equal to
    themselves regenerated alone."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RHO_TTS_AMD_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", RHO_TTS_AMD_SYNTHETIC="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                        "--master-port", "29537", os.path.join(root, "tests", "dp_corpus_worker.py"), "--texts", "512", "--jitter", "0", "0.3"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-4000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    print("\n" + json.dumps(out))
    assert out["texts"] == 512 and len(out["runs"]) == 2
    for run in out["runs"]:
        assert run["complete"] and run["order_ok"] and run["distinct_lengths"] >= 15, run
        assert run["occupancy"] >= 0.9, run
        assert run["alone_checked"] >= 8 and run["alone_equal"] == run["alone_checked"], run
        assert run["generate_calls"] == 1 and run["hand_overs"] >= 10, run          # ONE continuous-batching call per pass
        assert run["audio_s"] > 1000.0, run


def _bench(args, env=None, launcher=None, timeout=900):
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable] + (launcher or []) + [os.path.join(root, "bench.py")] + args
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    e.update(env or {})
    r = subprocess.run(cmd, cwd=root, env=e, capture_output=True, text=True, timeout=timeout)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    return r, (json.loads(lines[-1]) if lines else None)


def test_bench_gpus_flag_starts_its_own_ranks():
    """`python bench.py --gpus 2` WITHOUT a launcher must run a job of two ranks (here: two gloo ranks sharing the
    one GPU of the box - RCCL needs a GPU per rank) and say so in the line; with the nccl backend and one GPU it must fail."""
    common = ["--steps", "1", "--warmup", "1", "--model", "tiny", "--batch", "4", "--ref-seconds", "1", "--no-cpu-baseline", "--no-roofline"]
    r, line = _bench(["--gpus", "2", "--backend", "gloo"] + common)
    assert r.returncode == 0, r.stdout[-1500:] + "\n" + r.stderr[-3000:]
    assert line["n_gpus"] == 2 and line["ranks"]["world"] == 2 and line["ranks"]["rccl_ranks_seen"] == 2 and line["ranks"]["backend"] == "gloo"
    assert len(line["ranks"]["devices"]) == 2 and line["config"]["global_batch"] == 8
    r, line = _bench(["--gpus", "2"] + common)                    # nccl: one GPU per rank or nothing
    assert r.returncode != 0 and line is None and "GPU(s) visible" in r.stderr


def test_bench_one_gpu_direct_and_under_the_launcher_agree():
    """`python bench.py --gpus 1` and the driver's `torch.distributed.run --nproc-per-node 1 bench.py --gpus 1` (RCCL group of one
    rank, every collective of the multi-GPU step taken) measure the same workload: values within 3 %."""
    # (two warm-up steps: the first collectives of a process group set up their channels lazily - with one, 10 % of a 4-step run)
    common = ["--gpus", "1", "--steps", "5", "--warmup", "2", "--no-cpu-baseline", "--no-roofline"]
    r1, direct = _bench(common)
    assert r1.returncode == 0, r1.stderr[-3000:]
    r2, ranked = _bench(common, env={"RHO_TTS_AMD_FORCE_DIST": "1", "MASTER_ADDR": "127.0.0.1"},
                        launcher=["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port", "29541"])
    assert r2.returncode == 0, r2.stderr[-3000:]
    assert direct["ranks"]["rccl_ranks_seen"] is None and direct["ranks"]["world"] == 1
    assert ranked["ranks"] == dict(ranked["ranks"], world=1, backend="nccl", rccl_ranks_seen=1)
    assert abs(direct["value"] - ranked["value"]) <= 0.03 * direct["value"], (direct["value"], ranked["value"])


def test_bench_plain_run_dumps_the_last_step(tmp_path):
    """A plain `bench.py` run times exactly --steps steps, reports ms_per_step, measures nothing beyond the headline (no roofline,
    no CPU baseline: those are --full), and --dump-outputs writes the waveforms of its last step - the same ones, bit for bit, in
    a second run with the same flags."""
    common = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--model", "tiny", "--batch", "4", "--ref-seconds", "1"]
    got = []
    for name in ("a", "b"):
        r, line = _bench(common + ["--dump-outputs", str(tmp_path / name)])
        assert r.returncode == 0, r.stdout[-1500:] + "\n" + r.stderr[-3000:]
        assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["roofline"] is None and line["cpu_baseline"] is None and "ttfa_ms_one_text" not in line["extra"]
        files = sorted(os.listdir(tmp_path / name))
        assert files == [f"waveform_{i:04d}.npy" for i in range(4)], files
        got.append([np.load(tmp_path / name / f) for f in files])
    for x, y in zip(*got):
        assert x.dtype == np.float32 and np.array_equal(x, y)


def test_pinned_ring_views_live_until_the_call_after_next():
    """dist.waveforms_to_host(copy=False) hands out views of a two-buffer pinned ring (bench.py reads a step's waveforms before the
    step after next): the views of one call survive the next call and equal the copying form's result."""
    from rho_tts_amd import dist as D
    g = torch.Generator().manual_seed(3)
    a = [torch.randn(1000 + 37 * i, generator=g).cuda() for i in range(5)] + [None, torch.zeros(0).cuda()]
    b = [torch.randn(777, generator=g).cuda()]
    va = D.waveforms_to_host(a, copy=False)
    keep = [None if w is None else w.clone() for w in va]
    vb = D.waveforms_to_host(b, copy=False)                     # the other buffer of the ring
    assert all((x is None and y is None) or torch.equal(x, y) for x, y in zip(va, keep))
    assert torch.equal(vb[0], b[0].cpu()) and va[5] is None and va[6].numel() == 0
    ca = D.waveforms_to_host(a, copy=True)
    assert all((x is None and y is None) or torch.equal(x, y.cpu()) for x, y in zip(ca, a))

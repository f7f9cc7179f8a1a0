"""The voice bank on the GPU: several resident voices, a voice per item, and every item bit for bit what it gets alone with that voice
on the single-voice path - here a SECOND model created without max_voices, the voice set by the calls that existed before the bank.

1. the multi-voice decode attention on its own (rt_debug_attention_fused_voices): an exact census of the cache rows every row reads,
   under rt_debug_tune 1501 (the matrix-core launch, alone and beside the vector launch) and under the shipped 1500 (vector launch);
2. preset `small` (head_dim 128), under the shipped decode attention (rt_debug_tune 1500: the vector form for every voice) and
   under the matrix-core form (1501: voices of >= 64 prefix rows take it, shorter ones the vector form - mixed classes): static
   batch, continuous batching with a re-voiced block, mixed attention classes, and the bank model without item voices;
3. preset `tiny` (head_dim 32: the vector forms throughout);
4. voice blobs between bank entries."""
import contextlib
import ctypes

import pytest
import torch

from oracle.model import Voice
from rho_tts_amd import config, weights

pytestmark = pytest.mark.gpu


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def ctx():
    from rho_tts_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ 1. key census per voice
@pytest.mark.parametrize("mfma,d,heads,kvh,lens", [
    (1, 128, 4, 2, (64, 97, 97)),    # matrix cores (rt_debug_tune 1501): an exact tile edge, zero-padded tiles, an equal-length pair
    (0, 32, 4, 2, (5, 33, 33)),      # vector form (head_dim 32 has no other)
    (1, 128, 4, 2, (40, 64, 97)),    # mixed classes under 1501: block 0 in the vector launch, blocks 1 and 2 in the matrix-core launch
    (0, 128, 4, 2, (64, 97, 97)),    # the shipped switch (1500): the same voices, every block in the vector launch
    (0, 128, 4, 2, (40, 64, 97)),
])
def test_every_block_reads_the_prefix_of_its_own_voice(ctx, mfma, d, heads, kvh, lens):
    assert ctx.lib.rt_debug_tune(1500 + mfma, 0) == 0
    try:
        _census_per_voice(ctx, d, heads, kvh, lens)
    finally:
        assert ctx.lib.rt_debug_tune(1500, 0) == 0


def _census_per_voice(ctx, d, heads, kvh, lens):
    """q = 0: every score is 0, the softmax uniform, the output the mean of the V rows in the context.  Voice v's prefix V row at
    position p is the indicator of (p + 7 v) mod d, a row's own V row at p the indicator of p mod d: a row that reads another voice's
    prefix (even one of equal length), another length, or a row it should not, changes an integer count - seen bit for bit."""
    g = torch.Generator().manual_seed(23)
    M, max_pos, nv = 12, 256, 3
    slots, width = M + nv, (heads + 2 * kvh) * d
    POISON = 64.0
    block_voice = [0, 1, 2]
    eye = torch.eye(d)
    own = eye[torch.arange(max_pos) % d]
    row_lp = torch.tensor([lens[block_voice[r // 4]] for r in range(M)])
    pos = (row_lp + torch.randint(1, 41, (M,), generator=g)).to(torch.int32)
    pos[0], pos[-1] = lens[0] + 1, lens[2] + 40
    vc = torch.full((slots, kvh, max_pos, d), POISON)
    for r in range(M):
        vc[r, :, int(row_lp[r]): int(pos[r])] = own[int(row_lp[r]): int(pos[r])]
    for v in range(nv):
        vc[M + v, :, : lens[v]] = eye[(torch.arange(lens[v]) + 7 * v) % d]
    kc = torch.randn(slots, kvh, max_pos, d, generator=g)
    qkv = torch.zeros(M, width)
    qkv[:, heads * d: (heads + kvh) * d] = torch.randn(M, kvh * d, generator=g)
    qkv[:, (heads + kvh) * d:] = own[pos.long()].repeat(1, kvh)
    inv = 1.0 / (1e6 ** (torch.arange(0, d, 2, dtype=torch.float32) / d))
    fr = torch.arange(max_pos, dtype=torch.float32)[:, None] * inv[None]
    cos, sin = fr.cos().contiguous().cuda(), fr.sin().contiguous().cuda()
    k0, v0 = kc.to(torch.bfloat16), vc.to(torch.bfloat16)
    kd, vd = k0.cuda(), v0.cuda()
    out = torch.zeros(M, heads * d, dtype=torch.bfloat16, device="cuda")
    ones = torch.ones(d).cuda()
    qkv_d, slot_d, pos_d = qkv.cuda(), torch.arange(M, dtype=torch.int32).cuda(), pos.cuda()
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rt_debug_attention_fused_voices(ctx.handle, ptr(qkv_d), M, heads, kvh, d, ptr(ones), ptr(ones), 1e-6, ptr(cos), ptr(sin),
                                                      ptr(slot_d), ptr(pos_d), 0, ptr(kd), ptr(vd), slots, max_pos, nv, (ctypes.c_int32 * nv)(*lens),
                                                      (ctypes.c_int32 * 3)(*block_voice), ptr(out)), "rt_debug_attention_fused_voices")
    torch.cuda.synchronize()
    got = out.float().cpu().view(M, heads, d)
    for r in range(M):
        v, lp, n = block_voice[r // 4], int(row_lp[r]), int(pos[r]) + 1
        count = eye[(torch.arange(lp) + 7 * v) % d].sum(0) + own[lp:n].sum(0)
        want = (count / float(n)).to(torch.bfloat16).float()
        assert torch.equal(got[r], want[None].expand(heads, d)), (r, v, lp, n, float((got[r] - want).abs().max()))
    # the appended K / V rows landed in the rows' own slots, and nothing else moved: prefix slots and POISON rows untouched
    k1, v1 = kd.cpu(), vd.cpu()
    touched = torch.zeros(slots, max_pos, dtype=torch.bool)
    touched[torch.arange(M), pos.long()] = True
    assert torch.equal(v1.transpose(1, 2)[touched].float(), own[pos.long()].to(torch.bfloat16).float()[:, None].expand(M, kvh, d))
    assert not torch.equal(k1.transpose(1, 2)[touched], k0.transpose(1, 2)[touched])
    assert torch.equal(k1.transpose(1, 2)[~touched], k0.transpose(1, 2)[~touched])
    assert torch.equal(v1.transpose(1, 2)[~touched], v0.transpose(1, 2)[~touched])


def test_bad_block_tables_are_refused_on_the_host(ctx):
    d, M = 32, 4
    z = torch.zeros(M, 8 * d, device="cuda")
    kv = torch.zeros(6, 2, 64, d, dtype=torch.bfloat16, device="cuda")
    i32 = torch.zeros(M, dtype=torch.int32, device="cuda")
    out = torch.zeros(M, 4 * d, dtype=torch.bfloat16, device="cuda")

    def call(nv, lens, blocks, m=M):
        return ctx.lib.rt_debug_attention_fused_voices(ctx.handle, ptr(z), m, 4, 2, d, None, None, 1e-6, ptr(z), ptr(z), ptr(i32), ptr(i32), 0, ptr(kv),
                                                       ptr(kv), 6, 64, nv, (ctypes.c_int32 * len(lens))(*lens), (ctypes.c_int32 * len(blocks))(*blocks), ptr(out))
    assert call(2, [5, 5], [2]) == 1 and call(2, [5, 65], [0]) == 1 and call(9, [5] * 9, [0]) == 1 and call(2, [5, 5], [-1]) == 1
    assert call(2, [5, 5], [0], m=0) == 1 and call(7, [5] * 7, [0]) == 1          # (7 voices do not fit 6 slots)


# ------------------------------------------------------------------------------------------------ models
SAMPLING = (1, 0.9, 50, 1.0, 1.05)


def clone(cfg, n_ref, seed):
    g = torch.Generator().manual_seed(seed)
    return Voice("english", speaker_embed=torch.randn(cfg.talker.hidden, generator=g) * 0.05,
                 ref_text_ids=[int(v) for v in torch.randint(0, cfg.text_vocab - 64, (5,), generator=g)],
                 ref_codes=torch.randint(0, cfg.codec.codebook_size, (n_ref, cfg.n_groups), generator=g))


def set_voice(nm, v):
    return nm.set_voice(v.language, v.speaker, v.speaker_embed, v.ref_text_ids, v.ref_codes)


class Pair:
    """A bank model with `voices` resident in entries 0 .. and a plain model (no max_voices) that gives every item alone."""

    def __init__(self, ctx, preset, voices, max_batch=16):
        from rho_tts_amd._native_model import NativeModel, RtSampling
        self.cfg = config.PRESETS[preset]()
        state = {k: v.cuda() for k, v in weights.synthetic_state(self.cfg, 789).items()}
        self.bank = NativeModel(ctx, self.cfg, max_batch=max_batch, max_voices=4)
        self.bank.load_state(state)
        self.plain = NativeModel(ctx, self.cfg, max_batch=max_batch)
        self.plain.load_state(state)
        self.voices, self.sp = voices, RtSampling(*SAMPLING)
        self.lens = []
        for i, v in enumerate(voices):
            self.bank.select_voice(i)
            self.lens.append(set_voice(self.bank, v))
        self.bank.select_voice(0)
        self._alone, self._plain_voice, self.form = {}, None, 0

    @contextlib.contextmanager
    def decode_form(self, mfma):
        """rt_debug_tune 1500 + mfma for both models: 0 the shipped vector form, 1 the matrix cores (four rows per workgroup)."""
        assert self.bank.lib.rt_debug_tune(1500 + mfma, 0) == 0
        self.form = mfma
        try:
            yield
        finally:
            assert self.bank.lib.rt_debug_tune(1500, 0) == 0
            self.form = 0

    def close(self):
        self.bank.close()
        self.plain.close()

    def items(self, n, seed):
        g = torch.Generator().manual_seed(seed)
        texts = [[int(t) for t in torch.randint(0, self.cfg.text_vocab - 64, (int(k),), generator=g)] for k in torch.randint(3, 10, (n,), generator=g)]
        frames = [int(f) for f in torch.randint(3, 9, (n,), generator=g)]
        return texts, frames, [300 + 11 * i for i in range(n)]

    def alone(self, v, text, frames, item_id):
        key = (self.form, v, tuple(text), frames, item_id)
        if key not in self._alone:
            if self._plain_voice != v:
                assert set_voice(self.plain, self.voices[v]) == self.lens[v]
                self._plain_voice = v
            self._alone[key] = self.plain.generate([text], [frames], self.sp, seed=5, item_ids=[item_id])[0]
        return self._alone[key]

    def check(self, texts, frames, ids, voices, **kw):
        got = self.bank.generate(texts, frames, self.sp, seed=5, item_ids=ids, voices=voices, **kw)
        assert [c.shape[0] for c in got] == frames and all(int(c.abs().sum()) > 0 for c in got)
        for v in sorted(set(voices)):                                  # (grouped: the plain model changes voice once per voice)
            for i in [i for i in range(len(texts)) if voices[i] == v]:
                assert torch.equal(got[i], self.alone(v, texts[i], frames[i], ids[i])), (i, v)
        return got


@pytest.fixture(scope="module")
def small(ctx):
    cfg = config.small()
    p = Pair(ctx, "small", [clone(cfg, 56, 5), clone(cfg, 90, 6), clone(cfg, 56, 7), Voice("chinese", speaker="ryan")])
    yield p
    p.close()


A, B, C, D = 0, 1, 2, 3


def test_small_prefix_lengths_are_the_ones_the_cases_need(small):
    a, b, c, d = small.lens
    assert a >= 64 and a % 32 and b > a and c == a and d < 64, small.lens
    assert small.bank.voice_capacity() == 4 and small.plain.voice_capacity() == 1
    for i, n in enumerate(small.lens):
        small.bank.select_voice(i)
        assert small.bank.prefix_len() == n
    small.bank.select_voice(0)


@pytest.mark.parametrize("mfma", [0, 1])
def test_small_static_batch_of_three_voices(small, mfma):
    texts, frames, ids = small.items(10, 31)
    with small.decode_form(mfma):
        small.check(texts, frames, ids, [A, B, A, C, B, B, A, C, A, B])
        # (the voices matter: the same item alone with another voice - even one of equal prefix length - gets other codes)
        assert not torch.equal(small.alone(A, texts[0], frames[0], ids[0]), small.alone(B, texts[0], frames[0], ids[0]))
        assert not torch.equal(small.alone(A, texts[0], frames[0], ids[0]), small.alone(C, texts[0], frames[0], ids[0]))
    assert small.bank.generate_stats()["hand_overs"] == 0


@pytest.mark.parametrize("mfma", [0, 1])
def test_small_continuous_batching_re_voices_a_block(small, mfma):
    texts, frames, ids = small.items(14, 32)
    voices = [A, B, A, C, B, B, A, C, A, B, C, C, A, B]
    for every in (4, 1):
        small.bank.lib.rt_debug_tune(1700 + every, 0)
        try:
            with small.decode_form(mfma):
                small.check(texts, frames, ids, voices, max_rows=8)
        finally:
            small.bank.lib.rt_debug_tune(1704, 0)
        st = small.bank.generate_stats()
        assert st["rows"] == 8 and st["hand_overs"] >= 1 and st["frames_kept"] == sum(frames)
        assert small.bank.revoiced_blocks() >= 1


@pytest.mark.parametrize("mfma", [1, 0])
def test_small_mixed_attention_classes(small, mfma):
    """Under 1501 voices A and B (>= 64 prefix rows) take the matrix cores and D (a built-in speaker, 9 rows) the vector form: a step
    is two launches, each over its own blocks, and a re-voiced block changes lists."""
    texts, frames, ids = small.items(9, 33)
    with small.decode_form(mfma):
        small.check(texts, frames, ids, [A, D, B, D, A, B, D, A, D])
        small.check(texts, frames, ids, [D, A, B, D, A, B, D, A, D], max_rows=8)   # ... and through hand-overs
        assert small.bank.generate_stats()["hand_overs"] >= 1


def test_small_one_row_switch_falls_back_to_the_default_form(small):
    """rt_debug_tune 1502 (the matrix cores with one row per workgroup) has no multi-voice instantiation: a multi-voice run takes the
    DEFAULT form, the vector unit for every voice - each item is what it gets alone under the shipped switch."""
    texts, frames, ids = small.items(6, 37)
    want = [small.alone(v, t, f, i) for v, t, f, i in zip([A, D, B, D, A, B], texts, frames, ids)]       # under 1500
    assert small.bank.lib.rt_debug_tune(1502, 0) == 0
    try:
        got = small.bank.generate(texts, frames, small.sp, seed=5, item_ids=ids, voices=[A, D, B, D, A, B])
    finally:
        assert small.bank.lib.rt_debug_tune(1500, 0) == 0
    assert all(torch.equal(x, y) for x, y in zip(got, want))


def test_small_bank_model_without_item_voices_is_the_plain_model(small):
    texts, frames, ids = small.items(6, 34)
    want = [small.alone(A, t, f, i) for t, f, i in zip(texts, frames, ids)]
    got = small.bank.generate(texts, frames, small.sp, seed=5, item_ids=ids)
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    got = small.bank.generate(texts, frames, small.sp, seed=5, item_ids=ids, voices=[A] * 6)      # one distinct voice: the same run
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    # another entry selected, or named for every item while entry 0 stays selected: that voice's codes
    want_b = [small.alone(B, t, f, i) for t, f, i in zip(texts, frames, ids)]
    got = small.bank.generate(texts, frames, small.sp, seed=5, item_ids=ids, voices=[B] * 6)
    assert all(torch.equal(x, y) for x, y in zip(got, want_b)) and small.bank.prefix_len() == small.lens[A]
    small.bank.select_voice(B)
    try:
        got = small.bank.generate(texts, frames, small.sp, seed=5, item_ids=ids)
        assert all(torch.equal(x, y) for x, y in zip(got, want_b))
    finally:
        small.bank.select_voice(A)
    # item voices are consumed by the call they were given to
    got = small.bank.generate(texts, frames, small.sp, seed=5, item_ids=ids)
    assert all(torch.equal(x, y) for x, y in zip(got, want))


def test_small_refusals_come_before_any_launch(small):
    texts, frames, ids = small.items(3, 35)
    nm = small.bank
    with pytest.raises(ValueError):
        nm.generate(texts, frames, small.sp, voices=[A, 4, A])                     # outside the bank
    with pytest.raises(ValueError):
        nm.generate(texts, frames, small.sp, voices=[A, B])                        # wrong length
    rc = nm.lib.rt_generate_item_voices(nm.handle, (ctypes.c_int32 * 2)(A, B), 2)
    assert rc == 0
    with pytest.raises(ValueError):
        nm.generate(texts, frames, small.sp)                                       # two voices left over for three items
    assert len(nm.generate(texts, frames, small.sp)) == 3                          # ... and forgotten
    with pytest.raises(RuntimeError):                                              # teacher forcing with two voices
        nm.generate(texts, frames, small.sp, voices=[A, B, A], forced_codes=[torch.zeros(f, small.cfg.n_groups, dtype=torch.int64) for f in frames])
    with pytest.raises(ValueError):
        nm.select_voice(4)
    with pytest.raises(ValueError):
        small.plain.select_voice(1)
    from rho_tts_amd._native_model import NativeModel
    with pytest.raises(ValueError):
        NativeModel(nm.ctx, small.cfg, max_batch=4, max_voices=9)


def test_small_voice_blobs_move_between_entries(small):
    """export entry 2, clear it, import into entry 1: the items that named entry 2 get the same codes from entry 1."""
    texts, frames, ids = small.items(5, 36)
    nm = small.bank
    want = small.check(texts, frames, ids, [C, A, C, A, C])
    nm.select_voice(B)
    blob_b = nm.export_voice()
    nm.select_voice(C)
    blob = nm.export_voice()
    nm.clear_voice(C)
    assert nm.prefix_len() == 0
    with pytest.raises(ValueError):
        nm.generate(texts, frames, small.sp, voices=[C, A, C, A, C])              # entry 2 is not set any more
    try:
        nm.select_voice(B)
        nm.import_voice(small.lens[C], blob)
        assert nm.prefix_len() == small.lens[C]
        nm.select_voice(A)
        got = nm.generate(texts, frames, small.sp, seed=5, item_ids=ids, voices=[B, A, B, A, B])
        assert all(torch.equal(x, y) for x, y in zip(got, want))
    finally:                                                                       # the fixture's voices back in place
        nm.select_voice(B)
        nm.import_voice(small.lens[B], blob_b)
        nm.select_voice(C)
        nm.import_voice(small.lens[C], blob)
        nm.select_voice(A)
    small.check(texts, frames, ids, [C, B, C, A, B])


# ------------------------------------------------------------------------------------------------ 3. tiny: the vector forms
def test_tiny_speakers_and_a_clone_static_and_queued(ctx):
    cfg = config.tiny()
    p = Pair(ctx, "tiny", [Voice("english", speaker="vivian"), Voice("chinese", speaker="ryan"), clone(cfg, 9, 8)], max_batch=8)
    try:
        assert p.lens[0] == p.lens[1] and p.lens[2] > p.lens[0] and cfg.talker.head_dim == 32 and p.bank.max_positions == 256
        texts, frames, ids = p.items(11, 41)
        p.check(texts[:7], frames[:7], ids[:7], [0, 1, 2, 1, 0, 2, 2])
        p.check(texts, frames, ids, [0, 1, 2, 1, 0, 2, 2, 1, 1, 0, 2], max_rows=8)
        assert p.bank.generate_stats()["hand_overs"] >= 1
        # rows 1..3 are free from the first frame beside item 0; item 5 waits for a row of voice 1's block and runs frames 120 .. 240.
        # Free rows restart behind their prefix at the hand-over instead of stepping on to position 9 + 240 + the polling slack,
        # past the 256 positions
        texts, ids = texts[:6], ids[:6]
        p.check(texts, [120] * 6, ids, [0, 1, 1, 1, 1, 1], max_rows=8)
        st = p.bank.generate_stats()
        assert st["hand_overs"] >= 1 and st["frames_run"] >= 240 and st["rows"] == 8
        with pytest.raises(RuntimeError):                              # prefix + suffix + frames beyond the positions: refused up front
            p.bank.generate(texts, [250] * 6, p.sp, voices=[0, 1, 1, 1, 1, 1], max_rows=8)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 5. through the provider
def test_provider_items_equal_two_single_voice_providers(tmp_path):
    """add_voice + _generate_audio(voices=[None, "b", None]): every waveform bit for bit the item's from a provider that has only
    that voice, with the same item ids (synthetic weights, preset small)."""
    import wave

    import numpy as np

    from rho_tts_amd.provider import MI355XQwenTTS
    sr = 24000

    def clip(name, f0):
        i = np.arange(sr * 2)
        pcm = (0.3 * np.sin(2 * np.pi * f0 * i / sr) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * i / sr)) * 32767).astype("<i2")
        with wave.open(str(tmp_path / name), "wb") as wf:
            wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(sr); wf.writeframes(pcm.tobytes())
        return str(tmp_path / name)
    a, b = clip("a.wav", 150), clip("b.wav", 210)
    texts, ids = ["The first of three short texts", "A second one in another voice", "And the third closes the batch"], [5, 6, 7]
    kw = dict(model_path="small", batch_size=4, max_iterations=1)
    bank = MI355XQwenTTS(reference_audio=a, reference_text="the first reference", max_voices=2, **kw)
    only_a = MI355XQwenTTS(reference_audio=a, reference_text="the first reference", **kw)
    only_b = MI355XQwenTTS(reference_audio=b, reference_text="a second reference sentence", **kw)
    try:
        bank.add_voice("b", b, "a second reference sentence")
        got = bank._generate_audio(texts, item_ids=ids, voices=[None, "b", None])
        want_a = only_a._generate_audio([texts[0], texts[2]], item_ids=[5, 7])
        want_b = only_b._generate_audio([texts[1]], item_ids=[6])
        assert torch.equal(got[0], want_a[0]) and torch.equal(got[2], want_a[1]) and torch.equal(got[1], want_b[0])
        assert not torch.equal(got[1], only_a._generate_audio([texts[1]], item_ids=[6])[0])
        with pytest.raises(ValueError):
            bank._generate_audio(texts, item_ids=ids, voices=[None, "c", None])
        with pytest.raises(ValueError):
            bank.add_voice("c", a, "the first reference")                          # max_voices = 2: one named voice
    finally:
        for p in (bank, only_a, only_b):
            p.close()

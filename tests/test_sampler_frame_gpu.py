"""The sampler launch in the form the decode loop gives it (generate.hip, rt_gen_run::enqueue_a), through rt_debug_sample_frame:
seed and frame read on the device, a frame of its own per row, end of sequence by min_frames, forced and free rows in one launch,
frame-strided outputs, several logit slabs, and the fused embedding of the drawn code with and without the q/k/v table.

Tokens are compared with tests/sampling_ref.py: every DECIDED draw (margin >= 2^-20, see that file) must be the reference's token;
at most 1 % of a test's draws may be undecided.  Everything else is bit for bit: the summed logits, copies of table rows, the
embedding against rt_debug_embed_rowsq at the same tokens; every buffer holds 6 frames of a sentinel and only the launch's own frame
may change.  Each test prints its draws / undecided / smallest decided margin."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import rowops_ref as R
from tests import sampler_frame_cases as K
from tests.sampling_ref import CAP, DECIDED, SamplingParams

pytestmark = pytest.mark.gpu

SENT = -77
U24 = 2.0 ** -24
M, NF = K.M, K.NF
OUT_STRIDE = 4
OUT_FS, EOS_FS, FORCED_FS = M * OUT_STRIDE + 3, M + 1, M + 2


@pytest.fixture(scope="module")
def ctx():
    from rho_tts_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


def P(t):
    return None if t is None else t.data_ptr()


def dev(t):
    return None if t is None else t.contiguous().cuda()


def rt_sampling(sp):
    from rho_tts_amd._native_model import RtSampling
    return RtSampling(int(sp.do_sample), sp.temperature, sp.top_k, sp.top_p, sp.repetition_penalty)


class Launch:
    """One rt_debug_sample_frame call on sentinel-filled buffers of NF frames."""

    def __init__(self, ctx, slabs, sp, frame, frame_off=None, group=0, sup_from=None, eos=-1, eos_live=0, min_frames=0, forced=None,
                 seen=None, emb=None, qkv=None, rowsq_n=1, items=K.ITEMS, seed=K.SEED, null=(), M_arg=None, emb_H=None, qkv_n=None,
                 with_copy=True):
        from rho_tts_amd._native_model import RtDebugSampleFrame
        n_slabs, rows, V = slabs.shape
        self.V, self.frame = V, frame
        self.copy_fs = rows * V + 5
        d = self.d = dict(
            logits=dev(slabs), items=torch.tensor(items, dtype=torch.int64).cuda(), seed=torch.tensor([seed - (1 << 64) if seed >= 1 << 63 else seed]).cuda(),
            frame=torch.tensor([frame], dtype=torch.int32).cuda(), off=dev(frame_off), seen=seen,
            out=torch.full((NF, OUT_FS), SENT, dtype=torch.int32, device="cuda"), flag=torch.full((NF, EOS_FS), SENT, dtype=torch.int32, device="cuda"),
            copy=torch.full((NF, self.copy_fs), float(SENT), device="cuda") if with_copy else None, forced=None)
        if forced is not None:
            fb = torch.full((NF, FORCED_FS), 1, dtype=torch.int32)             # (other frames force code 1: a wrong stride would show)
            fb[frame, :rows] = forced
            d["forced"] = fb.cuda()
        a = RtDebugSampleFrame()
        a.d_logits, a.d_item_ids, a.d_seed, a.d_frame, a.d_frame_off = P(d["logits"]), P(d["items"]), P(d["seed"]), P(d["frame"]), P(d["off"])
        a.d_seen, a.d_forced, a.d_out, a.d_eos_flag, a.d_logits_copy = P(seen), P(d["forced"]), P(d["out"]), P(d["flag"]), P(d["copy"])
        a.out_fs, a.eos_fs, a.forced_fs, a.copy_fs = OUT_FS, EOS_FS, FORCED_FS, self.copy_fs
        a.sp = rt_sampling(sp)
        a.n_slabs, a.M, a.V = n_slabs, rows if M_arg is None else M_arg, V
        a.suppress_from, a.group = V if sup_from is None else sup_from, group
        a.eos_token, a.eos_live, a.min_frames, a.out_stride = eos, eos_live, min_frames, OUT_STRIDE
        if emb is not None:
            table, norm_w = emb
            H = table.shape[1]
            d.update(table=dev(table), norm_w=dev(norm_w), rowsq=torch.full((rows, rowsq_n), float(SENT), device="cuda"),
                     x=torch.full((rows, H), float(SENT), device="cuda"), a=torch.full((rows, H), float(SENT), dtype=torch.bfloat16, device="cuda"))
            a.d_emb_table, a.d_emb_norm_w, a.d_emb_rowsq, a.d_emb_x, a.d_emb_a_bf16 = P(d["table"]), P(d["norm_w"]), P(d["rowsq"]), P(d["x"]), P(d["a"])
            a.emb_H, a.emb_rowsq_n = H if emb_H is None else emb_H, rowsq_n
        if qkv is not None:
            n = qkv.shape[1]
            d.update(qkv=dev(qkv), qkv_out=torch.full((rows * n + 64,), float(SENT), device="cuda"))
            a.d_emb_qkv_table, a.d_emb_qkv_out, a.emb_qkv_n = P(d["qkv"]), P(d["qkv_out"]), n if qkv_n is None else qkv_n
        for name in null:
            setattr(a, name, None)
        torch.cuda.synchronize()
        self.rc = ctx.lib.rt_debug_sample_frame(ctx.handle, C.byref(a))
        self.out, self.flag = d["out"].cpu(), d["flag"].cpu()
        self.copy = d["copy"].cpu() if with_copy else None

    def tokens(self):
        return self.out[self.frame, :M * OUT_STRIDE:OUT_STRIDE].tolist()

    def flags(self):
        return self.flag[self.frame, :M].tolist()

    def check_frame_slots(self, what, flags=True):
        """Only this frame's slots of out / eos_flag / logits_copy changed, and all of them did."""
        w = torch.zeros(NF, OUT_FS, dtype=torch.bool)
        w[self.frame, :M * OUT_STRIDE:OUT_STRIDE] = True
        R.check_untouched(self.out, torch.tensor(SENT, dtype=torch.int32), w, what + ": out")
        assert not bool((self.out[w] == SENT).any()), what + ": a row of out was not written"
        w = torch.zeros(NF, EOS_FS, dtype=torch.bool)
        if flags:
            w[self.frame, :M] = True
            assert not bool((self.flag[w] == SENT).any()), what + ": a flag was not written"
        R.check_untouched(self.flag, torch.tensor(SENT, dtype=torch.int32), w, what + ": eos_flag")
        if self.copy is not None:
            w = torch.zeros(NF, self.copy_fs, dtype=torch.bool)
            w[self.frame, :M * self.V] = True
            R.check_untouched(self.copy, torch.tensor(float(SENT)), w, what + ": logits_copy")

    def untouched(self, what):
        """A refused call wrote nothing."""
        assert self.rc != 0, what + ": launched instead of being refused"
        assert bool((self.out == SENT).all()) and bool((self.flag == SENT).all()), what + ": a refused call wrote its outputs"


class Tally:
    """Decided draws must match; the undecided ones are counted against the cap."""

    def __init__(self):
        self.n = self.undecided = 0
        self.min_margin = np.inf

    def add(self, got, want, margins, what):
        for r, (g, w, m) in enumerate(zip(got, want, margins)):
            self.n += 1
            if m < DECIDED:
                self.undecided += 1
                continue
            assert g == w, f"{what}: row {r} drew {g}, the reference {w} (margin {m:.3e})"
            self.min_margin = min(self.min_margin, m)

    def close(self, what):
        print(f"{what}: {self.n} draws, {self.undecided} undecided, smallest decided margin {self.min_margin:.3e}")
        assert self.undecided <= CAP * self.n, f"{what}: {self.undecided} of {self.n} draws undecided"


def seen_dev(seen):
    return seen.to(torch.uint8).cuda()


# ================================================================================================ instantiations, slabs, frames
@pytest.mark.parametrize("V,n_slabs", K.SLAB_CASES)
def test_slabs_frames_and_item_ids(ctx, V, n_slabs):
    """4 / 8 / 16 waves and the LDS kernel, logits in 1 and 3 slabs (summed in float32 in slab order: logits_copy bit for bit), the
    frame counter at 0, 1 and 5 with a start per row, 64-bit item ids, a device seed with a high half; min_frames 2 with the end
    of sequence live - it carries the largest logit in every third row and so is drawn now and then."""
    sup, eos = K.layout(V)
    slabs, logits = K.slab_case(V, n_slabs)
    t = Tally()
    for sp in (K.SP_A, K.SP_B):
        for frame in (0, 1, 5):
            off = K.frame_offsets(frame)
            what = f"V={V} slabs={n_slabs} T={sp.temperature} frame={frame}"
            seen0 = torch.rand(M, V, generator=K.gen(frame)) < 0.05
            seen = seen_dev(seen0)
            L = Launch(ctx, slabs, sp, frame, off, group=frame % 3, sup_from=sup, eos=eos, eos_live=1, min_frames=2, seen=seen)
            ctx.check(L.rc, "rt_debug_sample_frame")
            toks, margins, out, flags, after = K.reference(logits, sp, frame, off, frame % 3, sup, eos, 1, 2, seen=seen0)
            t.add(list(zip(L.tokens(), L.flags())), list(zip(out, flags)), margins, what)
            L.check_frame_slots(what)
            R.check_bits(L.copy[frame, :M * V].reshape(M, V), logits, what + ": logits_copy")
            got_seen = seen.cpu().bool()
            for r in range(M):                       # the history gains the drawn token and nothing else
                tok = eos if L.flags()[r] else L.tokens()[r]
                want = seen0[r].clone()
                want[tok] = True
                assert torch.equal(got_seen[r], want), (what, r)
    t.close(f"slabs V={V} n={n_slabs}")


# ================================================================================================ end of sequence
@pytest.mark.parametrize("eos_live", [0, 1])
@pytest.mark.parametrize("V", [700, 3072, 6000])
def test_end_of_sequence_by_min_frames(ctx, V, eos_live):
    """min_frames 2, frame counter 3, starts 0 .. 3: a row whose end-of-sequence logit is the largest draws it under greedy and
    under top_k = 1 exactly when the end of sequence is live and the row's OWN frame is >= 2; then out = 0, flag = 1 and the id is
    marked seen.  Otherwise the flag is 0 and the token is the reference's."""
    sup, eos = K.layout(V)
    slabs, logits = K.slab_case(V, 1)
    frame = 3
    off = torch.tensor([r % 4 for r in range(M)], dtype=torch.int32)       # every own frame 0 .. 3 meets an eos row (r % 3 == 0)
    t = Tally()
    for sp in (K.GREEDY, K.TOP1, K.SP_A):
        what = f"V={V} live={eos_live} sample={sp.do_sample} k={sp.top_k}"
        seen = torch.zeros(M, V, dtype=torch.uint8, device="cuda")
        L = Launch(ctx, slabs, sp, frame, off, sup_from=sup, eos=eos, eos_live=eos_live, min_frames=2, seen=seen)
        ctx.check(L.rc, "rt_debug_sample_frame")
        toks, margins, out, flags, _ = K.reference(logits, sp, frame, off, 0, sup, eos, eos_live, 2)
        t.add(list(zip(L.tokens(), L.flags())), list(zip(out, flags)), margins, what)
        L.check_frame_slots(what)
        n_eos = 0
        for r in range(M):
            may = eos_live == 1 and frame - int(off[r]) >= 2
            if r % 3 == 0 and may and sp is not K.SP_A:
                assert (L.tokens()[r], L.flags()[r]) == (0, 1) and int(seen[r, eos]) == 1, (what, r)
                n_eos += 1
            if not may:
                assert L.flags()[r] == 0 and int(seen[r, eos]) == 0 and L.tokens()[r] < sup, (what, r)
        assert sp is K.SP_A or n_eos == (4 if eos_live else 0), (what, n_eos)
    t.close(f"eos V={V} live={eos_live}")


# ================================================================================================ forcing
@pytest.mark.parametrize("V", [700, 2048, 6000])
def test_forced_and_free_rows_in_one_launch(ctx, V):
    """forced = -1 / a code / the end-of-sequence id, by row, in frame 2's slots of the forced buffer (the other frames force code 1):
    forced rows return their token - flagged and zeroed when it is the end of sequence, although it is not live - and mark it seen;
    the other rows draw."""
    sup, eos = K.layout(V)
    slabs, logits = K.slab_case(V, 1)
    frame, off, forced = 2, K.frame_offsets(2), K.forced_rows(V)
    t = Tally()
    for sp in (K.GREEDY, K.SP_B):
        what = f"V={V} sample={sp.do_sample}"
        seen = torch.zeros(M, V, dtype=torch.uint8, device="cuda")
        L = Launch(ctx, slabs, sp, frame, off, sup_from=sup, eos=eos, eos_live=0, min_frames=2, forced=forced, seen=seen)
        ctx.check(L.rc, "rt_debug_sample_frame")
        toks, margins, out, flags, after = K.reference(logits, sp, frame, off, 0, sup, eos, 0, 2, forced=forced, seen=torch.zeros(M, V, dtype=torch.bool))
        t.add(list(zip(L.tokens(), L.flags())), list(zip(out, flags)), margins, what)
        L.check_frame_slots(what)
        got_seen = seen.cpu()
        for r in range(M):
            if r % 3 == 1:
                assert (L.tokens()[r], L.flags()[r]) == (int(forced[r]), 0), (what, r)
            if r % 3 == 2:
                assert (L.tokens()[r], L.flags()[r]) == (0, 1), (what, r)
            if r % 3:
                assert int(got_seen[r].sum()) == 1 and int(got_seen[r, int(forced[r])]) == 1, (what, r)
            else:
                assert L.flags()[r] == 0 and int(got_seen[r].sum()) == 1 and int(got_seen[r, L.tokens()[r]]) == 1, (what, r)
    t.close(f"forcing V={V}")


# ================================================================================================ penalty history
@pytest.mark.parametrize("V", [700, 3072])
def test_penalty_history_over_three_frames(ctx, V):
    """Three consecutive launches (frames 0, 1, 2) on the same `seen` buffer with penalty 1.3 and integer logits, so that tokens
    repeat; the reference carries its own history (tests/test_sampling_ref_cpu.py: a sampler without the history draws other
    tokens here).  Where a draw is undecided the reference's history takes the GPU's token: both are valid continuations."""
    sup, eos = K.layout(V)
    logits = K.integer_case(V)
    t = Tally()
    for sp in (K.SP_B, SamplingParams(True, 0.9, 50, 1.0, 1.3)):
        seen = torch.zeros(M, V, dtype=torch.uint8, device="cuda")
        hist = torch.zeros(M, V, dtype=torch.bool)
        for frame in range(3):
            what = f"V={V} T={sp.temperature} frame={frame}"
            L = Launch(ctx, logits[None], sp, frame, None, sup_from=sup, eos=eos, eos_live=0, min_frames=2, seen=seen, with_copy=False)
            ctx.check(L.rc, "rt_debug_sample_frame")
            toks, margins, out, flags, hist = K.reference(logits, sp, frame, [0] * M, 0, sup, eos, 0, 2, seen=hist)
            t.add(L.tokens(), out, margins, what)
            got_seen = seen.cpu().bool()
            undecided = torch.tensor([m < DECIDED for m in margins])
            assert torch.equal(got_seen[~undecided], hist[~undecided]), what + ": history"
            hist[undecided] = got_seen[undecided]
    t.close(f"history V={V}")


# ================================================================================================ fused embedding
def embed_rowsq_hook(ctx, table, norm_w, tokens, rowsq_n, qkv=None):
    """rt_debug_embed_rowsq's f32-table mode at the same tokens."""
    rows, H = len(tokens), table.shape[1]
    idx = torch.tensor(tokens, dtype=torch.int32).cuda()
    rs = torch.full((rows, rowsq_n), float(SENT), device="cuda")
    x = torch.full((rows, H), float(SENT), device="cuda")
    a = torch.full((rows, H), float(SENT), dtype=torch.bfloat16, device="cuda")
    td, wd, qd = dev(table), dev(norm_w), dev(qkv)
    qo = None if qkv is None else torch.full((rows * qkv.shape[1],), float(SENT), device="cuda")
    torch.cuda.synchronize()
    rc = ctx.lib.rt_debug_embed_rowsq(ctx.handle, (C.c_void_p * 1)(), (C.c_int64 * 1)(), 0, P(td), P(idx), 1, None, 0, rows, H, None, P(rs), rowsq_n, P(x), P(a),
                                      P(wd), None, None, P(qd), P(qo), 0 if qkv is None else qkv.shape[1], 0)
    ctx.check(rc, "rt_debug_embed_rowsq")
    return rs.cpu(), x.cpu(), a.cpu(), None if qo is None else qo.cpu()


@pytest.mark.parametrize("rowsq_n", [1, 16])
@pytest.mark.parametrize("V,H", K.EMBED_CASES)
def test_fused_embedding_without_the_table(ctx, V, H, rowsq_n):
    """A predictor pass: the drawn code's row of the f32 table becomes x, bf16(norm_w .* x) and the rowsq seed - equal to embed_ref
    at the tolerances of test_embed_rowsq_f32_table, and to rt_debug_embed_rowsq's own output at the same tokens bit for bit.
    H = 2080 with V = 700 (256 threads): four lanes run the row loop's second round."""
    slabs, logits = K.slab_case(V, 1, seed=H)
    table = torch.randn(V, H, generator=K.gen(4000 + H))
    norm_w = 1 + 0.1 * torch.randn(H, generator=K.gen(4001 + H))
    frame, off = 1, K.frame_offsets(1)
    L = Launch(ctx, slabs, K.SP_A, frame, off, group=1, emb=(table, norm_w), rowsq_n=rowsq_n, null=("d_eos_flag",))
    ctx.check(L.rc, "rt_debug_sample_frame")
    what = f"V={V} H={H} rowsq_n={rowsq_n}"
    toks, margins, out, flags, _ = K.reference(logits, K.SP_A, frame, off, 1, V, -1, 0, 0)
    t = Tally()
    t.add(L.tokens(), out, margins, what)
    L.check_frame_slots(what, flags=False)
    got = L.tokens()
    rs, x, a = L.d["rowsq"].cpu(), L.d["x"].cpu(), L.d["a"].cpu()
    x_ref, mag = R.embed_ref([], torch.tensor(got)[:, None], None, table)
    R.check_close(x, x_ref, 16 * U24 * mag, what + ": x")
    R.check_bits(x, table[torch.tensor(got)], what + ": x is a copy of the table row")
    R.check_rel(rs[:, 0], R.rowsq_ref(x_ref), 1e-5, what + ": sum of squares")
    R.check_bits(rs[:, 1:], torch.zeros_like(rs[:, 1:]), what + ": the other partial slots")
    R.check_bits(a, R.bf16(norm_w * x), what + ": bf16(norm_w * x)")
    hs, hx, ha, _ = embed_rowsq_hook(ctx, table, norm_w, got, rowsq_n)
    R.check_bits(x, hx, what + ": x against k_embed_rowsq")
    R.check_bits(a, ha, what + ": a against k_embed_rowsq")
    R.check_bits(rs, hs, what + ": rowsq against k_embed_rowsq")
    t.close(f"embedding {what}")


@pytest.mark.parametrize("V,H,qkv_n", K.TABLE_CASES)
def test_fused_embedding_with_the_qkv_table(ctx, V, H, qkv_n):
    """Table mode: tiled x and the code's q/k/v row are copies bit for bit, a and rowsq keep the sentinel, the guard behind the last
    q/k/v row keeps its bytes.  (700, 2080, 2060) runs both tail loops of the 256-thread instantiation: 260 octets of x for 256
    threads, 515 16-byte pieces of q/k/v for 2 x 256."""
    slabs, logits = K.slab_case(V, 1, seed=H)
    table = torch.randn(V, H, generator=K.gen(4000 + H))
    norm_w = 1 + 0.1 * torch.randn(H, generator=K.gen(4001 + H))
    qkv = torch.randn(V, qkv_n, generator=K.gen(4002 + H))
    frame, off = 1, K.frame_offsets(1)
    forced = torch.full((M,), -1, dtype=torch.int32)
    forced[5], forced[6] = 0, V - 1                                  # the table's first and last rows, whatever is drawn
    L = Launch(ctx, slabs, K.SP_A, frame, off, group=2, emb=(table, norm_w), qkv=qkv, rowsq_n=16, forced=forced, null=("d_eos_flag",))
    ctx.check(L.rc, "rt_debug_sample_frame")
    what = f"V={V} H={H} qkv_n={qkv_n}"
    toks, margins, out, flags, _ = K.reference(logits, K.SP_A, frame, off, 2, V, -1, 0, 0, forced=forced)
    t = Tally()
    t.add(L.tokens(), out, margins, what)
    L.check_frame_slots(what, flags=False)
    got = torch.tensor(L.tokens())
    assert int(got[5]) == 0 and int(got[6]) == V - 1
    R.check_bits(L.d["x"].cpu(), table[got], what + ": x")
    qo = L.d["qkv_out"].cpu()
    R.check_bits(qo[:M * qkv_n].reshape(M, qkv_n), qkv[got], what + ": q/k/v rows")
    R.check_bits(qo[M * qkv_n:], torch.full((64,), float(SENT)), what + ": guard behind the last q/k/v row")
    R.check_bits(L.d["a"].cpu(), torch.full((M, H), float(SENT), dtype=torch.bfloat16), what + ": a keeps the sentinel")
    R.check_bits(L.d["rowsq"].cpu(), torch.full((M, 16), float(SENT)), what + ": rowsq keeps the sentinel")
    hx, hq = embed_rowsq_hook(ctx, table, norm_w, got.tolist(), 16, qkv)[1::2]
    R.check_bits(L.d["x"].cpu(), hx, what + ": x against k_embed_rowsq")
    R.check_bits(qo[:M * qkv_n], hq, what + ": q/k/v against k_embed_rowsq")
    t.close(f"table {what}")


# ================================================================================================ refusals
def test_refusals(ctx):
    """A status, nothing launched: the outputs keep the sentinel."""
    slabs, _ = K.slab_case(64, 1)
    table, norm_w, qkv = torch.randn(64, 64, generator=K.gen(1)), torch.ones(64), torch.randn(64, 128, generator=K.gen(2))
    sp = K.SP_A

    def refused(what, slabs=slabs, sp=sp, **kw):
        L = Launch(ctx, slabs, sp, 1, K.frame_offsets(1), **kw)
        L.untouched(what)
        assert ctx.lib.rt_last_error(ctx.handle), what
        return L

    refused("top_k 0", sp=SamplingParams(True, 0.9, 0, 1.0, 1.0))
    refused("top_k 65", sp=SamplingParams(True, 0.9, 65, 1.0, 1.0))
    refused("temperature 0", sp=SamplingParams(True, 0.0, 50, 1.0, 1.0))
    refused("V = 16385", slabs=torch.zeros(1, M, 16385), with_copy=False)
    big = torch.zeros(1, M, 6000)
    L = refused("embedding with V = 6000", slabs=big, emb=(torch.zeros(6000, 64), norm_w), with_copy=False)
    R.check_bits(L.d["x"].cpu(), torch.full((M, 64), float(SENT)), "embedding with V = 6000: x")
    for H in (68, 2056):          # 2056 = 8 * 257: a multiple of 8 that the tiled layout cannot hold (k-tiles of 32 columns)
        L = refused(f"H = {H}", slabs=K.slab_case(700, 1)[0], emb=(torch.zeros(700, H), torch.ones(H)))
        R.check_bits(L.d["x"].cpu(), torch.full((M, H), float(SENT)), f"H = {H}: x")
        R.check_bits(L.d["rowsq"].cpu(), torch.full((M, 1), float(SENT)), f"H = {H}: rowsq")
    refused("a table without the embedding", emb=(table, norm_w), qkv=qkv, null=("d_emb_table",))
    L = refused("qkv_n 6", emb=(table, norm_w), qkv=qkv, qkv_n=6)
    R.check_bits(L.d["qkv_out"].cpu(), torch.full((M * 128 + 64,), float(SENT)), "qkv_n 6: q/k/v out")
    for name in ("d_logits", "d_item_ids", "d_seed", "d_frame", "d_out"):
        refused(f"null {name}", null=(name,))
    refused("M = 0", M_arg=0)
    refused("a forced token outside the embedding table", emb=(table, norm_w), forced=torch.full((M,), 64, dtype=torch.int32))
    assert ctx.lib.rt_debug_sample_frame(ctx.handle, None) != 0

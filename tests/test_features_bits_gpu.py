"""The drift-feature extractor (csrc/features.hip) against bits recorded on an MI355X from the last build in which
rt_features_extract and rt_features_extract_batch launched their front-half kernels separately (tests/golden/features_bits.npz,
written by tests/golden/make_features_bits.py).  Both entry points now run one path with one workspace set, so "the batch gives the
single call's bits" holds by construction; what pins the bits themselves is this fixture: either entry point, any order of the
clips, any neighbour, and a handle whose workspaces have grown for a larger call before a smaller one.  Every comparison is
np.array_equal."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch

from rho_tts_amd import _native
from rho_tts_amd import features as PF
from tests.test_features_batch_gpu import KINDS as BATCH_KINDS
from tests.test_features_batch_gpu import clip
from tests.test_oracle_features import voiced

pytestmark = pytest.mark.gpu

SR = 24000
FULL_CMND = ("short", "voiced300")                 # the clips whose whole difference function is in the fixture
PD, PI = C.POINTER(C.c_double), C.POINTER(C.c_int32)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "features_bits.npz")


def inputs():
    """kind -> (float32 samples, sample rate): the five clips of tests/test_features_batch_gpu.py at 24 kHz (38 frames down to the
    2 frames of ``short``), and a clip already at 16 kHz, which takes the branch without the resampler."""
    d = {k: (clip(k), SR) for k in BATCH_KINDS}
    d["voiced16k"] = (voiced(0.7, 16000, 300.0), 16000)
    return d


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(GOLDEN))
    for kind, (x, _) in inputs().items():          # first: the inputs are the recorded ones (a failure, never a skip)
        assert hashlib.sha256(x.tobytes()).hexdigest() == str(g[f"sha256_{kind}"]), f"input {kind} is not the recorded one"
    return g


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dev():
    return {k: (torch.from_numpy(x).cuda(), sr) for k, (x, sr) in inputs().items()}


@pytest.fixture(scope="module")
def ex(ctx):
    e = PF.HandcraftedFeatures(ctx)
    e.set_pitch_model()
    yield e
    e.close()


def fresh(ctx, pitch_model=True):
    e = PF.HandcraftedFeatures(ctx)
    if pitch_model:
        e.set_pitch_model()
    return e


def check_raw(e, dev, gold, kind):
    stats, cmnd, lpc = e.raw(*dev[kind])
    assert np.array_equal(stats, gold[f"stats_{kind}"]), kind
    assert np.array_equal(lpc, gold[f"lpc_{kind}"]), kind
    assert np.array_equal(np.array(cmnd.shape), gold[f"cmnd_shape_{kind}"]), kind
    if kind in FULL_CMND:
        assert np.array_equal(cmnd, gold[f"cmnd_{kind}"]), kind


def check_batch(e, dev, gold, kinds):
    """One batch() and one f0_states() call over ``kinds`` (any order, any subset of the five): every row is the fixture's."""
    xs = [dev[k][0] for k in kinds]
    batch, states = e.batch(xs, SR), e.f0_states(xs, SR)
    assert batch.shape == (len(kinds), 30) and len(states) == len(kinds)
    for row, st, k in zip(batch, states, kinds):
        assert np.array_equal(row, gold["batch"][BATCH_KINDS.index(k)]), (kinds, k)
        assert np.array_equal(st, gold[f"states_{k}"]), (kinds, k)


def test_the_fixture_is_small_and_complete(gold):
    assert os.path.getsize(GOLDEN) < 100 * 1024
    assert gold["batch"].shape == (5, 30)
    assert tuple(gold["cmnd_shape_voiced"]) == (38, 329) and tuple(gold["cmnd_shape_short"]) == (2, 329)
    assert all(len(gold[f"states_{k}"]) == gold[f"cmnd_shape_{k}"][0] for k in BATCH_KINDS)


@pytest.mark.parametrize("kind", list(BATCH_KINDS) + ["voiced16k"])
def test_single_entry_point_gives_the_recorded_bits(ex, dev, gold, kind):
    check_raw(ex, dev, gold, kind)


def test_batch_entry_point_gives_the_recorded_bits(ex, dev, gold):
    check_batch(ex, dev, gold, BATCH_KINDS)
    one = ex.batch([dev["voiced16k"][0]], 16000)                            # no resampler: the caller's buffer is the 16-kHz clip
    assert one.shape == (1, 30)
    assert np.array_equal(one[0, :26], gold["stats_voiced16k"])
    assert tuple(one[0, 28:30]) == PF.formants_from_lpc(gold["lpc_voiced16k"])


def test_order_and_neighbours_do_not_matter(ex, dev, gold):
    check_batch(ex, dev, gold, BATCH_KINDS[::-1])
    rest = [k for k in BATCH_KINDS if k != "short"]
    check_batch(ex, dev, gold, ["short"])
    check_batch(ex, dev, gold, ["short"] + rest)
    check_batch(ex, dev, gold, rest + ["short"])


def test_one_workspace_set_grows_and_is_reused(ctx, dev, gold):
    """A smaller call after a larger one must not see the larger one's gmax, states or frames, whichever entry point made it."""
    e = fresh(ctx)
    try:
        check_raw(e, dev, gold, "short")
        check_batch(e, dev, gold, BATCH_KINDS)
        check_raw(e, dev, gold, "short")
    finally:
        e.close()
    e = fresh(ctx)
    try:
        check_batch(e, dev, gold, BATCH_KINDS)
        check_batch(e, dev, gold, ["short"])
    finally:
        e.close()
    e = fresh(ctx, pitch_model=False)
    try:
        check_raw(e, dev, gold, "voiced")
        check_raw(e, dev, gold, "short")
    finally:
        e.close()


def test_single_call_needs_no_pitch_model(ctx, dev, gold):
    e = fresh(ctx, pitch_model=False)
    try:
        for kind in ("voiced300", "voiced16k"):
            check_raw(e, dev, gold, kind)
    finally:
        e.close()


def test_single_call_refusals(ex, dev, gold):
    x = dev["short"][0]
    torch.cuda.synchronize()
    n_lags = ex.max_period - ex.min_period + 1

    def native(n_samples, cap, with_cmnd=True):
        stats, lpc, cmnd = np.zeros(26), np.zeros(PF.LPC_ORDER + 1), np.zeros((max(cap, 1), n_lags))
        nm, npf = C.c_int32(), C.c_int32()
        rc = ex.lib.rt_features_extract(ex.handle, C.c_void_p(x.data_ptr()), n_samples, SR, ex.min_period, ex.max_period, PF.LPC_ORDER,
                                        stats.ctypes.data_as(PD), C.byref(nm), cmnd.ctypes.data_as(PD) if with_cmnd else None, cap, C.byref(npf),
                                        lpc.ctypes.data_as(PD))
        return rc, stats, lpc, cmnd, npf.value
    assert native(1, 8)[0] == _native.RT_ERR_INVALID                        # below two samples
    assert native(x.numel(), 1)[0] == _native.RT_ERR_LENGTH                 # two pitch frames, room for one
    rc, stats, lpc, cmnd, npf = native(x.numel(), 2)
    assert rc == _native.RT_OK and npf == 2 and np.array_equal(cmnd, gold["cmnd_short"])
    rc, stats, lpc, _, npf = native(x.numel(), 0, with_cmnd=False)          # no difference function wanted: k_feat_cmnd is skipped
    assert rc == _native.RT_OK and npf == 2
    assert np.array_equal(stats, gold["stats_short"]) and np.array_equal(lpc, gold["lpc_short"])

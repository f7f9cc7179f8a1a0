"""bench.py --dump-outputs: the waveforms of the last timed step as float32 .npy files, within a size limit (a seeded sample of
the items beyond it), so two builds can be compared output for output.  The file writing is host code and is checked here."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _waves(lengths, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [None if n is None else torch.randn(n, generator=g) for n in lengths]


def test_dump_writes_every_waveform_as_float32(tmp_path):
    waves = _waves([100, 0, None, 37])
    (tmp_path / "waveform_0099.npy").write_bytes(b"stale")               # left by an earlier run: removed
    (tmp_path / "notes.txt").write_text("kept")
    kept = bench.dump_outputs(waves, str(tmp_path))
    assert kept == [0, 1, 3]
    assert sorted(os.listdir(tmp_path)) == ["notes.txt", "waveform_0000.npy", "waveform_0001.npy", "waveform_0003.npy"]
    for i in kept:
        a = np.load(tmp_path / f"waveform_{i:04d}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, waves[i].numpy())


def test_dump_over_the_limit_is_a_fixed_seeded_sample(tmp_path):
    waves = _waves([1000] * 20)                                          # 4000 bytes each
    a = bench.dump_outputs(waves, str(tmp_path / "a"), limit=30_000)
    b = bench.dump_outputs(waves, str(tmp_path / "b"), limit=30_000)
    assert a == b and len(a) == 7 and a != list(range(7))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 30_000
    for i in a:
        assert np.array_equal(np.load(tmp_path / "a" / f"waveform_{i:04d}.npy"), waves[i].numpy())


def test_steps_below_one_is_refused():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]

"""dist.broadcast_voice with a bank entry, rehearsed on two gloo ranks with a fake engine (no GPU): the blob of the named entry travels,
lands in the same entry on the receiving rank under its name, and the entry that was selected before the call is selected after it."""
import multiprocessing as mp
import os
import socket

import torch

from rho_tts_amd import dist as D


class _BankModel:
    def __init__(self, rank):
        self.rank, self.selected_voice, self.selections = rank, 0, []
        self.entries = {0: (5, torch.arange(10.0)), 2: (7, torch.arange(14.0) + 100)} if rank == 0 else {}

    def select_voice(self, v):
        self.selected_voice = v
        self.selections.append(v)

    def export_voice(self):
        return self.entries[self.selected_voice][1].to(torch.bfloat16)

    def prefix_len(self):
        return self.entries[self.selected_voice][0]

    def import_voice(self, n, blob):
        self.entries[self.selected_voice] = (n, blob.float().clone())


class _BankEngine:
    def __init__(self, rank):
        self.device, self.model, self.voice, self.voices, self._prefix_len = torch.device("cpu"), _BankModel(rank), None, {}, {}


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        eng = _BankEngine(rank)
        eng.model.select_voice(1)                                       # something else is selected when the broadcast is asked for
        D.broadcast_voice(eng, dist, src=0, voice_index=2, name="narrator")
        ok = eng.model.selected_voice == 1 and eng.model.selections == [1, 2, 1]
        D.broadcast_voice(eng, dist, src=0, voice_index=0)                  # the engine's own voice: entry 0, selection restored too
        ok = ok and eng.model.selected_voice == 1 and eng.model.selections == [1, 2, 1, 0, 1]
        if rank == 1:
            ok = ok and eng.model.entries[2][0] == 7 and eng.model.entries[2][1].tolist() == [100.0 + i for i in range(14)]
            ok = ok and eng.model.entries[0][0] == 5 and eng.model.entries[0][1].tolist() == [float(i) for i in range(10)]
            ok = ok and eng.voices["narrator"][0] == 2 and eng._prefix_len[2] == 7 and eng.voice is not None
        else:
            ok = ok and eng.voices == {}                                # rank 0 registered its voice itself, before the call
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


def test_a_bank_entry_travels_to_the_same_entry_and_the_selection_is_kept():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res == {0: True, 1: True}

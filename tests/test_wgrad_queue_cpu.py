"""The deferred weight-gradient queue (hip/wgrad.py::WgQueue) on the host alone: stubs stand in for the launchers and the
streams, the operands are meta tensors, the bank is a stand-in with the three attributes the queue reads.  What is pinned:
when the queue flushes (members, bytes), what it holds until the join, what drop() forgets, and how a group with a
repeated slot is cut into calls."""
import contextlib
import types

import pytest
import torch

from easevoice_trainer_amd.hip import wgrad as W


class _Stream:
    def __init__(self):
        self.waited = []

    def wait_stream(self, other):
        self.waited.append(other)


class _Slot:
    packed_member = False

    def __init__(self, name, bank):
        self.name, self.bank = name, bank


@pytest.fixture
def rig(monkeypatch):
    """a bank stand-in with its queue; rig.calls lists what reached the launchers: ("one", slot name) per single launch,
    ("group", [slot names]) per grouped call"""
    cur, side = _Stream(), _Stream()
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: cur)
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(W.L, "role_stream", lambda device, role: side)
    calls = []
    monkeypatch.setattr(W, "_bwd_weight_now", lambda slot, *rest: calls.append(("one", slot.name)))
    real_call = W._bwd_weight_group_call

    def group_call(members):
        if len(members) == 1:
            return real_call(members)             # a one-member run: the real code hands it to the single launcher
        calls.append(("group", [j.slot.name for j in members]))

    monkeypatch.setattr(W, "_bwd_weight_group_call", group_call)
    bank = types.SimpleNamespace(device=torch.device("cpu"), defer_n=4, defer_bytes=1 << 30, parts_on=False)
    bank.wgq = W.WgQueue(bank)
    return types.SimpleNamespace(bank=bank, q=bank.wgq, calls=calls, cur=cur, side=side,
                                 slots={n: _Slot(n, bank) for n in "ABCD"})


def _job(rig, name, elems=8):
    """a job over meta operands: x and dy of `elems` bf16 elements each (4 * elems bytes), y a tensor of its own"""
    x, dy, y = (torch.empty(elems, dtype=torch.bfloat16, device="meta") for _ in range(3))
    return W.WgJob(rig.slots[name], x, dy, y, 1, elems, 1.0, 0, 1.0)


def test_record_knows_its_bytes_and_operands(rig):
    j = _job(rig, "A", 8)
    assert j.nbytes == 2 * 8 * 2 and j.held == (j.x, j.dy, j.y)
    assert W.WgGroup([j, _job(rig, "B", 4)]).nbytes == 32 + 16
    assert (j.slot, j.nseq, j.lin, j.in_slope, j.out_act, j.out_slope) == (rig.slots["A"], 1, 8, 1.0, 0, 1.0)


def test_flush_fires_at_defer_n_members_and_not_before(rig):
    q = rig.q                                    # defer_n = 4
    W._bwd_weight(*_job(rig, "A"))
    assert q.count() == 1 and not rig.calls
    W._bwd_weight_group([tuple(_job(rig, "B")), _job(rig, "C")])  # a group counts with its members: 3 waiting
    assert q.count() == 3 and len(q.pending) == 2 and not rig.calls
    assert all(isinstance(j, W.WgJob) for j in q.pending[1])      # a member given as its nine fields becomes a record
    W._bwd_weight(*_job(rig, "D"))                               # the fourth member
    assert rig.calls == [("one", "A"), ("group", ["B", "C"]), ("one", "D")]
    assert q.count() == 0 and rig.bank.wgq.pending == []
    # the fork: the side stream waits for the stream that flushes and for every stream that queued
    assert rig.side.waited and all(s is rig.cur for s in rig.side.waited)
    # a group alone reaches the count too
    rig.calls.clear()
    W._bwd_weight_group([_job(rig, n) for n in "ABC"])
    assert not rig.calls
    W._bwd_weight_group([_job(rig, n) for n in "AB"])             # 5 >= 4
    assert rig.calls == [("group", ["A", "B", "C"]), ("group", ["A", "B"])]


def test_flush_fires_at_the_byte_budget(rig):
    rig.bank.defer_n, rig.bank.defer_bytes = 1000, 100
    W._bwd_weight(*_job(rig, "A", 12))           # 48 bytes
    assert rig.q.nbytes == 48 and not rig.calls
    W._bwd_weight(*_job(rig, "B", 12))           # 96
    assert rig.q.nbytes == 96 and not rig.calls
    W._bwd_weight(*_job(rig, "C", 1))            # 100: the budget
    assert [c[1] for c in rig.calls] == ["A", "B", "C"] and rig.q.nbytes == 0
    rig.calls.clear()
    W._bwd_weight_group([_job(rig, "A", 20), _job(rig, "B", 20)])     # a group's bytes are its members': 160
    assert rig.calls == [("group", ["A", "B"])]


def test_flush_holds_the_operands_and_join_releases_them(rig):
    rig.bank.defer_n = 1000
    jobs = [_job(rig, n) for n in "ABC"]
    W._bwd_weight(*jobs[0])
    W._bwd_weight_group(jobs[1:])
    assert not rig.q.held and rig.q.nbytes == 3 * 32
    rig.q.flush()
    assert rig.q.pending == [] and rig.q.nbytes == 0 and rig.q.count() == 0
    held = [t for triple in rig.q.held for t in triple]
    want = [t for j in jobs for t in (j.x, j.dy, j.y)]
    assert len(held) == len(want) == 9 and all(a is b for a, b in zip(held, want))
    assert rig.calls == [("one", "A"), ("group", ["B", "C"])]
    rig.q.flush()                                # nothing waits: nothing happens
    assert len(rig.calls) == 2
    assert not rig.cur.waited
    rig.q.join()
    assert rig.q.held == [] and rig.cur.waited == [rig.side]      # the current stream waited for the side stream
    assert len(rig.calls) == 2


def test_join_flushes_what_waits(rig):
    rig.bank.defer_n = 1000
    W._bwd_weight(*_job(rig, "A"))
    rig.q.join()
    assert rig.calls == [("one", "A")] and rig.q.pending == [] and rig.q.held == [] and rig.q.nbytes == 0


def test_drop_clears_everything_without_a_launch(rig):
    rig.bank.defer_n = 1000
    W._bwd_weight(*_job(rig, "A"))
    rig.q.flush()                                # held operands of launches that run ...
    rig.calls.clear()
    W._bwd_weight(*_job(rig, "B"))               # ... and entries that still wait
    W._bwd_weight_group([_job(rig, "C"), _job(rig, "D")])
    assert rig.q.pending and rig.q.held and rig.q.nbytes and rig.q.streams
    rig.q.drop()
    assert rig.calls == []
    assert rig.q.pending == [] and rig.q.held == [] and rig.q.nbytes == 0 and not rig.q.streams and rig.q.count() == 0
    assert rig.cur.waited == [rig.side]          # what already runs is waited for
    rig.q.join()                                 # and nothing is left to launch
    assert rig.calls == []


def test_a_repeated_slot_starts_the_next_call(rig):
    rig.bank.defer_n = 0                         # no queue: the group is launched where it is declared
    W._bwd_weight_group([_job(rig, n) for n in "ABAC"])
    assert rig.calls == [("group", ["A", "B"]), ("group", ["A", "C"])]
    rig.calls.clear()
    W._bwd_weight_group([_job(rig, n) for n in "ABA"])            # a one-member run goes to the single launcher
    assert rig.calls == [("group", ["A", "B"]), ("one", "A")]
    rig.calls.clear()
    rig.bank.defer_n = 1000                      # the same cut behind the queue
    W._bwd_weight_group([_job(rig, n) for n in "ABAC"])
    assert not rig.calls
    rig.q.flush()
    assert rig.calls == [("group", ["A", "B"]), ("group", ["A", "C"])]


def test_a_group_is_of_one_bank_and_has_no_packed_member(rig):
    other = _Slot("X", types.SimpleNamespace())
    with pytest.raises(W.L.EvtError):
        W._bwd_weight_group([_job(rig, "A"), W.WgJob(other, None, None, None, 1, 8, 1.0, 0, 1.0)])
    rig.slots["B"].packed_member = True
    with pytest.raises(W.L.EvtError):
        W._bwd_weight_group([_job(rig, "A"), _job(rig, "B")])
    with pytest.raises(W.L.EvtError):
        W._bwd_weight(*_job(rig, "B"))
    assert not rig.calls and not rig.q.pending

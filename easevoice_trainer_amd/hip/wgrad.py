"""Weight gradients of the convolutions: the record of one job, the bank's deferred queue (WgQueue: the backward
schedule -- what is queued, what flushes, which stream runs it and waits) and the launchers."""
import ctypes as C
from collections import namedtuple

import torch

from . import lib as L
from . import trace as T


class WgJob(namedtuple("WgJob", "slot x dy y nseq lin in_slope out_act out_slope")):
    """one weight gradient: the convolution's slot, its operands (x, dy, and the output y where the activation derivative
    is taken in the kernel) and the launch geometry"""
    __slots__ = ()

    @property
    def nbytes(self):        # operand bytes the queue holds for this job
        return self.x.numel() * self.x.element_size() + self.dy.numel() * self.dy.element_size()

    @property
    def held(self):          # the tensors that must stay alive until the side stream has run the launch
        return self.x, self.dy, self.y


class WgGroup(list):
    """a DECLARED group of weight gradients as one entry of the queue: the WgJobs of convolutions that become ready
    together (the layers of a WN stack), handed over by the module that owns them -- what is in a group never depends on
    when the queue is flushed"""

    @property
    def nbytes(self):
        return sum(j.nbytes for j in self)


GROUP_FLUSH = False  # measurements: True = a declared group is released to the side stream at once


class WgQueue:
    """the deferred weight-gradient launches of one bank (bank.defer_n, bank.defer_bytes: WeightBank.__init__ has the
    measurements): entries wait here and go to the bank's side stream in one fork"""

    __slots__ = ("bank", "pending", "streams", "nbytes", "held", "side")

    def __init__(self, bank):
        self.bank = bank
        self.pending = []        # WgJob | WgGroup, in the order they were pushed
        self.streams = set()     # the streams entries were pushed from
        self.nbytes = 0          # operand bytes of `pending`
        self.held = []           # operands of launches handed to the side stream, kept until the join
        self.side = None

    def side_stream(self):
        if self.side is None:
            self.side = L.role_stream(self.bank.device, "bank")
        return self.side

    def count(self):         # convolutions waiting (a declared group counts with all its members: WeightBank.queued)
        return sum(len(e) if isinstance(e, WgGroup) else 1 for e in self.pending)

    def push(self, entry):
        bank = self.bank
        self.pending.append(entry)
        self.streams.add(torch.cuda.current_stream(bank.device))   # a branch stream of the discriminators, or the main one
        self.nbytes += entry.nbytes
        # A group waits in the queue like its members would (count() takes them one by one, so the flushes stay where
        # they were).  Measured on the s2 step (profiles/wgrad_groups_step_ab.txt): groups of a whole stack counted as ONE
        # entry left the WN stacks -- the end of the generator's backward -- for the join, +0.5 ms; released at once
        # (GROUP_FLUSH) in runs of eight layers, their long blocks crowd the backward-data chain, +1.0 ms.
        if ((GROUP_FLUSH and isinstance(entry, WgGroup)) or self.count() >= bank.defer_n
                or self.nbytes >= bank.defer_bytes):
            self.flush()

    def flush(self):
        """hand the queued launches to the side stream (one fork)"""
        if not self.pending:
            return
        side = self.side_stream()
        side.wait_stream(torch.cuda.current_stream(self.bank.device))
        for st in self.streams:          # operands queued from another stream than the one that flushes
            side.wait_stream(st)
        self.streams.clear()
        with torch.cuda.stream(side):
            for e in self.pending:
                if isinstance(e, WgGroup):         # a declared group: one entry, one call
                    _bwd_weight_group_now(e)
                else:
                    _bwd_weight_now(*e)
        for e in self.pending:
            self.held.extend(j.held for j in (e if isinstance(e, WgGroup) else (e,)))
        self.pending.clear()
        self.nbytes = 0

    def join(self):
        """flush, and the current stream waits for the side stream; the held operands are released"""
        self.flush()
        if self.side is not None and self.held:
            torch.cuda.current_stream(self.bank.device).wait_stream(self.side)
        self.held.clear()

    def drop(self):
        """forget what is queued without launching it, wait for what already runs (WeightBank.zero_dw on a stale queue)"""
        if self.pending or self.held:
            self.pending.clear()
            self.streams.clear()
            self.nbytes = 0
            if self.side is not None:
                torch.cuda.current_stream(self.bank.device).wait_stream(self.side)
            self.held.clear()


def _bwd_weight(slot, x, dy, y, nseq, lin, in_slope, out_act, out_slope):
    bank = slot.bank
    if slot.packed_member:
        raise L.EvtError("weight gradient of a packed projection member requested on its own: inside a bf16 runtime the "
                         "q / k / v projections of a windowed attention layer run (and are differentiated) as one pack")
    if bank.defer_n > 0 and T.TRACE is None:
        bank.wgq.push(WgJob(slot, x, dy, y, nseq, lin, in_slope, out_act, out_slope))
        return
    _bwd_weight_now(slot, x, dy, y, nseq, lin, in_slope, out_act, out_slope)


def _bwd_weight_group(members):
    """weight gradients of several convolutions at once (members: WgJobs or their nine fields as tuples, all of one bank):
    evt_conv1d_bwd_weight_group launches those that meet in one kernel together, each with fewer splits -- fewer slabs
    written and folded -- than it would need alone.  A traced run launches them one by one, as before."""
    members = WgGroup(WgJob._make(j) for j in members)
    if not members:
        return
    bank = members[0].slot.bank
    for j in members:
        if j.slot.packed_member or j.slot.bank is not bank:
            raise L.EvtError("a weight-gradient group takes convolutions of one bank, none of them a packed projection member")
    if T.TRACE is not None:
        for j in members:
            _bwd_weight_now(*j)
    elif bank.defer_n > 0:
        bank.wgq.push(members)
    else:
        _bwd_weight_group_now(members)


def _bwd_weight_group_now(members):
    # two launches into one gradient image have an order: a slot that comes again starts the next call
    run, seen = [], set()
    for j in members:
        if id(j.slot) in seen:
            _bwd_weight_group_call(run)
            run, seen = [], set()
        run.append(j)
        seen.add(id(j.slot))
    _bwd_weight_group_call(run)


def _bwd_weight_group_call(members):
    if len(members) == 1:
        _bwd_weight_now(*members[0])
        return
    arr = (L.WgradMember * len(members))()
    keep = []
    for r, j in zip(arr, members):
        slot = j.slot
        p = slot.params(j.nseq, j.lin, j.in_slope, j.out_act, j.out_slope)
        dbias = _dbias_of(slot.module)
        sp = _wgrad_parts(slot, dbias) if slot.bank.parts_on else None
        keep.append((p, sp))
        r.p, r.x, r.dy = C.addressof(p), j.x.data_ptr(), j.dy.data_ptr()
        r.y = j.y.data_ptr() if (j.out_act != L.ACT_NONE and j.y is not None) else None
        r.dw, r.dbias = slot.dw.data_ptr(), (dbias.data_ptr() if dbias is not None else None)
        r.sp = C.addressof(sp) if sp is not None else None
    L.check(L.lib().evt_conv1d_bwd_weight_group(arr, len(members), L.stream_ptr()), "evt_conv1d_bwd_weight_group")
    for j, (_p, sp) in zip(members, keep):
        if sp is not None:
            j.slot.wg_used, j.slot.wg_dirty = max(j.slot.wg_used, int(sp.used)), True


def _dbias_of(m):
    if m.bias is None:
        return None
    if m.bias.grad is None:
        m.bias.grad = torch.zeros_like(m.bias)
    return m.bias.grad


def _wgrad_parts(slot, dbias):
    """the slot's evt_wgrad_parts record, brought up to date for the next launch into its image"""
    sp = slot._wgp
    if sp is None:
        sp = slot._wgp = L.WgradParts()
        sp.dw_extra = slot.dw_extra.data_ptr() if slot.parts > 1 else None
        sp.part_stride = slot.img_stride
        sp.db_part = slot.db_part.data_ptr() if (dbias is not None and not slot.module.transposed) else None
        sp.used_dev = slot.used.data_ptr()
        sp.parts = slot.parts
    sp.prev_used, sp.dirty0 = slot.wg_used, int(slot.wg_dirty)
    ws = slot.bank.scratch()
    sp.ws, sp.ws_floats = ws.data_ptr(), ws.numel()
    return sp


def _bwd_weight_now(slot, x, dy, y, nseq, lin, in_slope, out_act, out_slope):
    m = slot.module
    p = slot.params(nseq, lin, in_slope, out_act, out_slope)
    dbias = _dbias_of(m)
    e0 = T.t0()
    if slot.bank.parts_on:
        sp = _wgrad_parts(slot, dbias)
        L.check(L.lib().evt_conv1d_bwd_weight_parts(C.byref(p), L.ptr(x), L.ptr(dy),
                                                    L.ptr(y if out_act != L.ACT_NONE else None), L.ptr(slot.dw),
                                                    L.ptr(dbias), C.byref(sp), L.stream_ptr()),
                "evt_conv1d_bwd_weight_parts")
        slot.wg_used, slot.wg_dirty = max(slot.wg_used, int(sp.used)), True
    else:
        L.check(L.lib().evt_conv1d_bwd_weight(C.byref(p), L.ptr(x), L.ptr(dy),
                                              L.ptr(y if out_act != L.ACT_NONE else None), L.ptr(slot.dw), L.ptr(dbias),
                                              L.stream_ptr()), "evt_conv1d_bwd_weight")
    if e0 is not None:
        T.t1_conv(e0, "bwd_weight", m, nseq, lin, dy.numel() if out_act != L.ACT_NONE else 0)

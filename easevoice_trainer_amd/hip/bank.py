"""The prepared-weight banks of the fused conv family: per-conv slots (geometry + views into the arenas), the trained
bank (REG / ALT images, fp32 gradient images and slabs, device tables, the queue of hip/wgrad.py), the frozen fp32 bank."""
import ctypes as C
import os

import torch
from torch import nn

from . import lib as L
from .wgrad import WgQueue


def align128(elems):
    """image stride in elements: keeps every image 256-byte aligned.  THE stride of an image in the REG / gradient arenas,
    of the slabs the weight-gradient kernels write and of the slabs the fold reads (ConvSlot.img_stride)"""
    return (elems + 127) // 128 * 128


class ConvSlot:
    """Per-conv record inside a WeightBank: geometry + views into the prepared-weight arenas."""

    __slots__ = ("module", "layout", "img_stride", "reg", "alt", "dw", "bank", "_pcache", "packed_member", "parts",
                 "dw_extra", "db_part", "used", "wg_used", "wg_dirty", "_wgp")

    def __init__(self, module, layout, bank):
        self.module, self.layout, self.bank = module, layout, bank
        self.img_stride = align128(layout.reg_elems)
        self.reg = self.alt = self.dw = None
        self._pcache = {}
        self.packed_member = False   # True: the weight gradient of this conv is produced by a PackedConv over it
        # deterministic split-K (evt_conv1d_bwd_weight_parts): slabs of the gradient image beyond `dw`, partial bias
        # gradients, the device counters the kernels write, and the host's copy of the slab count of this step
        self.parts, self.dw_extra, self.db_part, self.used, self.wg_used, self._wgp = 1, None, None, None, 0, None
        self.wg_dirty = False        # a weight-gradient launch of this step has written into `dw` already

    def params(self, nseq, lin, in_slope, out_act, out_slope):
        key = (nseq, lin, in_slope, out_act, out_slope, self.bank.impl)
        p = self._pcache.get(key)
        if p is None:
            m = self.module
            p = L.ConvParams(self.bank.dt, nseq, lin, m.cin, m.cout, m.k, m.stride, m.pad, m.dil, m.groups,
                             1 if m.transposed else 0, in_slope, out_act, out_slope, self.bank.impl)
            self._pcache[key] = p
        return p


def conv_layout(dt, cin, cout, k, stride, pad, dil, groups, transposed) -> L.WLayout:
    p = L.ConvParams(dt, 1, max(64, k * dil + 1), cin, cout, k, stride, pad, dil, groups, 1 if transposed else 0,
                     1.0, 0, 1.0, 0)
    lay = L.WLayout()
    L.check(L.lib().evt_conv1d_layout(C.byref(p), C.byref(lay)), "evt_conv1d_layout")
    return lay


def _lay_out(bank, convs, dtype):
    """one ConvSlot per convolution (bank.slots, m._slot) and the REG / ALT arenas with every slot's views into them;
    returns the slots' offsets in the REG arena and its length (the fp32 gradient arena of a trained bank mirrors it)"""
    bank.slots, offs, reg_n, alt_n = [], [], 0, 0
    for m in convs:
        lay = conv_layout(bank.dt, m.cin, m.cout, m.k, m.stride, m.pad, m.dil, m.groups, m.transposed)
        s = ConvSlot(m, lay, bank)
        m._slot = s
        bank.slots.append(s)
        offs.append((reg_n, alt_n))
        reg_n += s.img_stride
        alt_n += align128(lay.alt_elems)
    bank.reg_arena = torch.zeros(max(reg_n, 1), dtype=dtype, device=bank.device)
    bank.alt_arena = torch.zeros(max(alt_n, 1), dtype=dtype, device=bank.device)
    for s, (ro, ao) in zip(bank.slots, offs):
        s.reg = bank.reg_arena[ro: ro + s.layout.reg_elems]
        s.alt = bank.alt_arena[ao: ao + s.layout.alt_elems]
    return [ro for ro, _ao in offs], reg_n


class PackedConv:
    """Several equal-shaped k = 1 convolutions of ONE input as a single convolution with the concatenated output channels
    (the q | k | v projections of an attention layer: three [C, C] weights -> one dense [3C, C] GEMM, one launch each way
    instead of three).  Exists only when the members' parameters are adjacent in the runtime's arena (ParamArena honours
    the owner's `arena_adjacent()`): `v` / `bias` and their gradients are then plain views over the members' storage,
    so the packed dW image unfolds straight into the members' .grad -- nothing is copied, the members stay usable."""
    weight_norm, kdims, transposed, groups, stride, pad, dil, k = False, 1, False, 1, 1, 0, 1, 1

    def __init__(self, members):
        m0 = members[0]
        self.members = members
        self.cin, self.cout = m0.cin, sum(m.cout for m in members)
        n, es = m0.weight.numel(), m0.weight.element_size()
        ws, bs = [m.weight for m in members], [m.bias for m in members]

        def adjacent(ts, numel):
            return all(t.data_ptr() == ts[0].data_ptr() + i * numel * es and t.is_contiguous() for i, t in enumerate(ts))

        ok = (all(m.cin == m0.cin and m.cout == m0.cout and m.k == 1 and not m.weight_norm and m.kdims == 1 and
                  m.bias is not None for m in members) and adjacent(ws, n) and adjacent(bs, m0.cout)
              and all(t.grad is not None for t in ws + bs) and adjacent([t.grad for t in ws], n)
              and adjacent([t.grad for t in bs], m0.cout))
        self.ok = ok
        if ok:
            self.v = torch.as_strided(ws[0].data, (self.cout, self.cin, 1), (self.cin, 1, 1))
            self.v.grad = torch.as_strided(ws[0].grad, (self.cout, self.cin, 1), (self.cin, 1, 1))
            self.bias = torch.as_strided(bs[0].data, (self.cout,), (1,))
            self.bias.grad = torch.as_strided(bs[0].grad, (self.cout,), (1,))
        self._slot = None

    def lout(self, lin):
        return lin


def slab_count(image_bytes, d0, budget=48 << 20, cap=32):
    """slabs of one convolution's gradient image for the deterministic split-K weight gradient (= the most position splits
    its kernel may use).  A small image can afford many (the reduction of a 128 -> 128 k11 vocoder layer runs over 40960
    positions for 180 K outputs); a 21 MB image (1024 -> 1024 k5) gets 3.  `cap` (32; measured on the s2 step: 26.2 ms,
    64: 26.5, 8: 30.9, 2: 52) bounds what evt_wn_grad_multi has to fold per image; two kinds of layer go beyond it, because
    all their parallelism comes from the split: images of a few KB (the 16- / 32-channel vocoder stages: 11 - 45 KB for
    160 K - 330 K positions) and layers with at most 64 output channels (one or two output tiles: 64 -> 64 k11 over 81920
    positions, in the step: 66 us with 32 slabs, 23 us with 128).  The s2 generator's slabs come to 5.2 GB, the
    discriminators' to 0.7 GB, of the 288 GB.  The count is an UPPER bound: a convolution launched with others of its
    WN stack (evt_conv1d_bwd_weight_group) fills the chip with their tiles and uses about half the splits it needs alone;
    the kernels record how many slabs hold sums, and the fold reads those."""
    limit = 256 if image_bytes <= (64 << 10) else (128 if d0 <= 64 else cap)
    return max(1, min(limit, -(-budget // max(image_bytes, 1))))


class WeightBank:
    """All prepared conv weights of one model: REG/ALT images in the compute dtype, fp32 dW images,
    and the device tables for the two multi-tensor launches (fold before forward, grad after backward)."""

    def __init__(self, model: nn.Module, dtype: torch.dtype, device, impl=L.IMPL_AUTO):
        L.set_half(dtype)     # a 16-bit compute dtype selects the build of the library that serves it
        self.dt = L.dt_code(dtype)
        self.dtype, self.device, self.impl = dtype, torch.device(device), impl
        self.weight_grads = True
        # EVT_WGRAD_DEFER=N (default 48; 0 = off): weight-gradient launches are queued and handed to a side HIP stream N at
        # a time -- ONE fork per batch instead of one per convolution -- so the backward-data chain (the critical path:
        # every launch waits for the one before it) shares the chip with the weight gradients, which depend on nothing
        # but their two operands.  grads() joins.  The operands are held until the join.  Measured on MI355X, s2 step
        # under HIP-graph replay, three interleaved rounds: 27.85-27.95 ms without, 27.14-27.18 ms with N = 64; small N
        # is slower under replay: one fork per convolution was measured at -1.6 ms/step with eager launches and
        # +7 ms/step under HIP-graph replay (fork/join edges per conv).
        # Round 6, under the branch streams (profiles/r06_streams.txt): the generator's ~150 launches flushed every 48 instead
        # of every 64 is 0.3 ms ahead (40-56 level except 52; 32 and 80-96 behind -- it matters which stretch of the backward a
        # flush lands beside); the discriminators' 42 stay one flush at the end either way (in pieces: +0.2 ms).
        # A declared group (_bwd_weight_group: four gradients of a WN stack) is one entry of the queue that counts with all
        # its members (queued()); re-swept with the groups: 16 / 24 / 32 / 64 are 0.7 - 2.1 ms behind 48.
        self.defer_n = int(os.environ.get("EVT_WGRAD_DEFER", "48")) if self.device.type == "cuda" else 0
        self.wgq = WgQueue(self)
        self.anchor = torch.zeros(1, device=device, requires_grad=True)
        # the bank's convolutions: every module that carries a `_slot` (EvtConv1d and what derives from it)
        convs = [m for m in model.modules() if hasattr(m, "_slot")]
        # packed projections (see PackedConv): only for the bf16 bank -- the fused attention node that uses them is bf16
        for m in model.modules():
            fn = getattr(m, "qkv_pack_modules", None)
            members = fn() if (fn is not None and L.is_half(dtype)) else None
            m_packed = None
            if members:
                pc = PackedConv(members)
                if pc.ok:
                    convs.append(pc)
                    m_packed = pc
            if fn is not None:
                m._qkv_packed = m_packed
        reg_offs, reg_n = _lay_out(self, convs, dtype)
        for m in convs:
            if isinstance(m, PackedConv):
                for mm in m.members:
                    mm._slot.packed_member = True
        # slab 0 of every gradient image + the kernels' slab counters (two int32 per conv): ONE memset per step clears both
        ns = len(self.slots)
        self.dw_arena = torch.zeros(max(reg_n, 1) + 2 * ns, dtype=torch.float32, device=device)
        self.used_all = self.dw_arena[max(reg_n, 1):].view(torch.int32)
        # slabs 1.. (EVT_WGRAD_PARTS=0 switches the deterministic split off: fp32 atomics into the one image as before);
        # how many per image: slab_count().  Never zeroed: a slab is stored before it is read, the counters say how many
        # are valid.
        self.parts_on = (L.is_half(dtype) and self.device.type == "cuda"
                         and os.environ.get("EVT_WGRAD_PARTS", "1") != "0")
        # the slab sizes below (48 MiB per image, at most 32 slabs: 5.9 GB for the s2 models) were measured on a 288 GB
        # MI355X; on a smaller device the budget shrinks with its memory (at 1/4 of the memory: 12 MiB, 1.5 GB)
        total_mem = torch.cuda.get_device_properties(self.device).total_memory if self.device.type == "cuda" else 0
        mem_scale = min(1.0, total_mem / float(256 << 30)) if total_mem else 1.0
        budget = int(os.environ.get("EVT_WGRAD_SLAB_MB", str(max(4, int(48 * mem_scale))))) << 20
        # slabs per image: more slabs = more split-K blocks for the weight-gradient launches, and as many more bytes for the
        # fold at the end of the backward (wn_grad).  32 until the launches moved off the critical path (side stream, branch
        # streams); since then the fold's bytes weigh more: 16-24 measured level and 0.2 ms ahead of 32, 8 and 4 behind
        # (profiles/r06_streams.txt).  The WN stacks' grouped launches use fewer than the cap (profiles/wgrad_groups_after.txt:
        # the generator's fold 599 -> 512 us with whole-stack groups); the arenas keep the upper bound
        cap = 20
        # operands held for the deferred weight-gradient launches: flushed on a byte budget as well as on a count
        self.defer_bytes = max(256, int(4096 * mem_scale)) << 20
        ex_n = db_n = 0
        ex_offs = []
        for s in self.slots:
            s.parts = slab_count(s.layout.reg_elems * 4, s.layout.d0, budget, cap) if self.parts_on else 1
            ex_offs.append((ex_n, db_n))
            ex_n += (s.parts - 1) * s.img_stride
            db_n += s.parts * ((s.layout.d0 + 31) // 32 * 32)
        # scratch of the two-launch reductions (evt_wgrad_parts.ws): one buffer per stream the weight gradients run on
        self._ws = {}
        # zeros once: the kernels never store the padded taps of an image row, and the fold adds whole rows
        self.dw_extra_arena = torch.zeros(max(ex_n, 1), dtype=torch.float32, device=device) if self.parts_on else None
        self.db_part_arena = torch.zeros(max(db_n, 1), dtype=torch.float32, device=device) if self.parts_on else None
        for i, (s, ro) in enumerate(zip(self.slots, reg_offs)):
            s.dw = self.dw_arena[ro: ro + s.layout.reg_elems]
            s.used = self.used_all[2 * i: 2 * i + 2]
            if self.parts_on:
                eo, do = ex_offs[i]
                s.dw_extra = self.dw_extra_arena[eo: eo + (s.parts - 1) * s.img_stride]
                s.db_part = self.db_part_arena[do: do + s.parts * s.layout.d0]
        self._items = self._rows = None
        self._nrows = 0
        # images that also exist in MFMA fragment order (frag()): re-made behind every fold by one launch
        self._frags, self._frag_items, self._frag_rows, self._frag_tables = {}, [], [], {}
        self._frag_retired = []       # superseded device tables, kept alive for graphs captured with them

    def build_tables(self):
        """(Re)build the device descriptor tables.  Must be called after parameters (and their .grad
        buffers) have reached their final storage (ParamArena.flatten)."""
        items, rows, groups = [], [], []
        self._slot_rows = []
        self._group_of_row = {}       # first table row of a slot -> first group of that slot (and the end sentinel)
        for i, s in enumerate(self.slots):
            m = s.module
            self._slot_rows.append((len(rows), len(rows) + s.layout.d0))
            v = m.v
            if v.grad is None:
                v.grad = torch.zeros_like(v)
            g = m.weight_g if m.weight_norm else None
            if g is not None and g.grad is None:
                g.grad = torch.zeros_like(g)
            it = L.WPrepItem()
            it.v = v.data_ptr()
            it.g = g.data_ptr() if g is not None else None
            # a packed member's .grad memory is updated by the pack's rows: two blocks doing `dv += ...` on the same
            # addresses would race (lost update), so the member's own rows are switched off in evt_wn_grad_multi
            it.reg, it.alt, it.dw = s.reg.data_ptr(), s.alt.data_ptr(), (None if s.packed_member else s.dw.data_ptr())
            it.dv = v.grad.data_ptr()
            it.dg = g.grad.data_ptr() if g is not None else None
            it.lay = s.layout
            it.dtype = self.dt
            it.src_d1 = int(getattr(m, "src_d1", 0))
            if self.parts_on and not s.packed_member:
                it.dw_extra = s.dw_extra.data_ptr() if s.parts > 1 else None
                it.dw_part_stride = s.img_stride
                it.used = s.used.data_ptr()
                bias = getattr(m, "bias", None)
                if bias is not None and not m.transposed:      # fused bias gradients exist for plain convolutions only
                    if bias.grad is None:
                        bias.grad = torch.zeros_like(bias)
                    it.db_part, it.db = s.db_part.data_ptr(), bias.grad.data_ptr()
            items.append(it)
            self._group_of_row[len(rows)] = len(groups)
            rows.extend((i, r) for r in range(s.layout.d0))
            # the fold walks groups of eight consecutive rows (evt_wn_fold_groups): both images leave as 16-byte pieces
            groups.extend((i, r, min(8, s.layout.d0 - r)) for r in range(0, s.layout.d0, 8))
        self._group_of_row[len(rows)] = len(groups)
        self._items = L.struct_to_device(items, self.device)
        self._rows = torch.tensor(rows, dtype=torch.int32, device=self.device).contiguous()
        self._groups = torch.tensor(groups, dtype=torch.int32, device=self.device).contiguous()
        self._nrows = len(rows)
        self._grad_stamp = self._grad_ptrs()

    def _grad_ptrs(self):
        """addresses of every .grad the device tables point at (weights, gains, fused bias gradients)"""
        out = []
        for s in self.slots:
            m = s.module
            g = m.weight_g if m.weight_norm else None
            b = getattr(m, "bias", None)
            out.append((m.v.grad.data_ptr() if m.v.grad is not None else 0,
                        g.grad.data_ptr() if (g is not None and g.grad is not None) else 0,
                        b.grad.data_ptr() if (b is not None and b.grad is not None) else 0))
        return out

    def fold(self, lo=None, hi=None):
        """w = g*v/|v| -> REG/ALT images for every conv of the model: ONE launch (or the rows [lo, hi) of rows_of())."""
        if self._items is None:
            self.build_tables()
        lo = 0 if lo is None else lo
        hi = self._nrows if hi is None else hi
        if hi <= lo:
            return
        glo, ghi = self._group_of_row.get(lo), self._group_of_row.get(hi)
        if glo is not None and ghi is not None and os.environ.get("EVT_FOLD_GROUPS", "1") != "0":
            # row ranges start and end at layer boundaries (rows_of): the same rows as groups of eight
            grp = C.c_void_p(self._groups.data_ptr() + 12 * glo)    # (item, first row, rows) int32 triples
            L.check(L.lib().evt_wn_fold_groups(L.ptr(self._items), grp, ghi - glo, L.stream_ptr()), "evt_wn_fold_groups")
        else:
            rows = C.c_void_p(self._rows.data_ptr() + 8 * lo)       # (item, row) int32 pairs
            L.check(L.lib().evt_wn_fold_multi(L.ptr(self._items), rows, hi - lo, L.stream_ptr()), "evt_wn_fold_multi")
        self._repack_frags(lo, hi)

    def frag(self, slot, which):
        """`slot`'s REG (which = "reg") or ALT ("alt") image in MFMA FRAGMENT ORDER (evt_frag_pack: [16-row tile][K step of
        32][64 lanes][8], lane (n, g) = row 16 tile + n, K elements 32 ks + 8 g ..): what the kernels that stream a weight
        image straight from global memory into MFMA operands with ONE MFMA per fragment read (csrc/wn_layer.hip) -- a
        wave's fragment load is then 1 KiB contiguous instead of 16 rows x 64 bytes, which the vector memory path serves at
        ~12 B/clk per CU (34 -> 20 us per WN layer).  Tried for csrc/resunit_wide.hip too (9-14 MFMAs per fragment): no change
        (23.06-23.20 against 22.96-22.98 ms per step), its loads are not what it waits for -- it reads REG / ALT directly.  A copy owned by the bank: made on first request, re-made behind every fold of the slot's rows (ONE launch for
        all registered images, captured with the fold when the step is a HIP graph)."""
        key = (id(slot), which)
        f = self._frags.get(key)
        if f is None:
            lay = slot.layout
            if which == "reg":
                rows, ktot, src, elems = lay.d0, lay.reg_nchunk * lay.reg_kp * lay.reg_ck, slot.reg, lay.reg_elems
            else:
                rows, ktot, src, elems = lay.d1, lay.alt_nchunk * lay.alt_kp * lay.alt_ck, slot.alt, lay.alt_elems
            if elems != rows * ktot or rows % 16 or ktot % 32 or not L.is_half(self.dtype):
                raise L.EvtError(f"no fragment-order form for this image ({which}, {rows} x {ktot}, {self.dtype})")
            if self._items is None:
                self.build_tables()
            f = torch.empty(elems, dtype=self.dtype, device=self.device)
            it = L.FragItem()
            it.src, it.dst, it.rows, it.ktot = src.data_ptr(), f.data_ptr(), rows, ktot
            self._frags[key] = f
            self._frag_items.append(it)
            self._frag_rows.append(self._slot_rows[self.slots.index(slot)])
            # a new image changes what a fold of its rows has to re-pack: the row-range tables are rebuilt on demand, but
            # the old device tables stay ALIVE -- a HIP graph captured earlier holds their addresses
            self._frag_retired.extend(t for t, _n in self._frag_tables.values() if t is not None)
            self._frag_tables.clear()
            one = L.struct_to_device([it], self.device)
            self._frag_tables[("one", len(self._frag_items))] = (one, 1)      # kept alive
            L.check(L.lib().evt_frag_pack(L.ptr(one), 1, L.stream_ptr()), "evt_frag_pack")
            # the whole-model table is rebuilt NOW (images are registered by the first eager forward), so that the fold a
            # later graph capture records finds it instead of building it -- a host-to-device copy -- inside the capture
            if not torch.cuda.is_current_stream_capturing():
                items = list(self._frag_items)
                self._frag_tables[(0, self._nrows)] = (L.struct_to_device(items, self.device), len(items))
        return f

    def _repack_frags(self, lo, hi):
        if not self._frag_items:
            return
        tab = self._frag_tables.get((lo, hi))
        if tab is None:
            items = [it for it, (r0, r1) in zip(self._frag_items, self._frag_rows) if r0 < hi and r1 > lo]
            tab = self._frag_tables[(lo, hi)] = (L.struct_to_device(items, self.device) if items else None, len(items))
        if tab[1]:
            L.check(L.lib().evt_frag_pack(L.ptr(tab[0]), tab[1], L.stream_ptr()), "evt_frag_pack")

    def zero_dw(self):
        # weight-gradient launches of a backward that never reached grads() (a standalone user, an exception in the
        # middle of a step): they would land in the images zeroed below -- drop them, wait for what already runs
        self.wgq.drop()
        self.dw_arena.zero_()            # slab 0 of every image and the slab counters
        self._tables_checked = False     # the gradient tensors are looked at once per step, by the first grads() call
        for s in self.slots:
            s.wg_used, s.wg_dirty = 0, False

    def scratch(self):
        """16 MiB of scratch for the current stream (created on first use)"""
        key = torch.cuda.current_stream(self.device).cuda_stream
        ws = self._ws.get(key)
        if ws is None:
            ws = self._ws[key] = torch.empty(4 << 20, dtype=torch.float32, device=self.device)
        return ws

    def side_stream(self):
        return self.wgq.side_stream()

    def queued(self):
        """convolutions waiting in the queue (a declared group counts with all its members: the flushes stay where they were)"""
        return self.wgq.count()

    def flush_deferred(self):
        """hand the queued weight-gradient launches to the side stream (one fork)"""
        self.wgq.flush()

    def join_side(self):
        self.wgq.join()

    def rows_of(self, modules):
        """[lo, hi) of the row table covered by `modules` (EvtConv1d instances of this bank, contiguous in slot order):
        lets a data-parallel step finish -- and start reducing -- the gradients of one sub-model while the backward of
        the next is still running"""
        idx = sorted(i for i, s in enumerate(self.slots) if any(s.module is m for m in modules))
        if not idx or idx != list(range(idx[0], idx[-1] + 1)):
            raise L.EvtError("rows_of: the modules must be a contiguous, non-empty run of this bank's convolutions")
        if self._items is None:
            self.build_tables()
        return self._slot_rows[idx[0]][0], self._slot_rows[idx[-1]][1]

    def check_tables(self):
        """a .grad replaced since the tables were built (zero_grad(set_to_none=True), a caller assigning a new tensor) would
        leave the fused bias gradients / dv / dg writing to the old storage -- rebuild the tables.  Looked at ONCE per step
        (zero_dw() re-arms it): the data-parallel program calls grads() per sub-model, and walking every slot's three
        pointers each time was pure host time on a launch-bound path.  A capture validates before it records: the check
        runs on the eager steps that precede it, and a replaced tensor between capture and replay would invalidate the
        graph's other recorded pointers as well."""
        if self._items is None:
            self.build_tables()
        elif not getattr(self, "_tables_checked", False) and not torch.cuda.is_current_stream_capturing():
            if self._grad_stamp != self._grad_ptrs():
                self.build_tables()
            self._tables_checked = True

    def grads(self, lo=None, hi=None, join=True):
        """dW images -> weight_v.grad / weight_g.grad (or weight.grad), ACCUMULATED (+=): one launch over the whole
        model, or over the row range [lo, hi) of rows_of() -- every row must be visited exactly once per backward.
        join=False: the caller's stream already waits for the weight-gradient side stream (ModelRuntime.book_piece)."""
        if join:
            self.join_side()
        self.check_tables()
        lo = 0 if lo is None else lo
        hi = self._nrows if hi is None else hi
        if hi <= lo:
            return
        rows = C.c_void_p(self._rows.data_ptr() + 8 * lo)       # (item, row) int32 pairs
        L.check(L.lib().evt_wn_grad_multi(L.ptr(self._items), rows, hi - lo, L.stream_ptr()), "evt_wn_grad_multi")


class FrozenConv:
    """geometry + tensor getters of a convolution whose weight is never trained (ssl_proj, the RVQ codebook as a 1x1
    layer): what ConvSlot / _fwd need from a module, nothing that WeightBank would pick up from model.modules()"""
    weight_norm, kdims, transposed, groups, dil = False, 1, False, 1, 1

    def __init__(self, weight_fn, bias_fn, cin, cout, k=1, stride=1, padding=0):
        self.weight_fn, self.bias_fn = weight_fn, bias_fn
        self.cin, self.cout, self.k, self.stride, self.pad = cin, cout, k, stride, padding
        self._slot = None

    @property
    def v(self):
        w = self.weight_fn()
        return w if w.dim() == 3 else w.unsqueeze(-1)

    @property
    def bias(self):
        return self.bias_fn() if self.bias_fn is not None else None

    def lout(self, lin):
        return (lin + 2 * self.pad - (self.k - 1) - 1) // self.stride + 1


class FrozenBank:
    """fp32 images of weights outside the trained bank -- the s2 quantizer path runs in fp32 whatever the compute dtype of
    the step (models.py:912-921 disables autocast there).  Folded on first use and again whenever the tensors were
    replaced or written through torch (load_state_dict, the k-means initialisation): torch's version counters tell."""
    weight_grads = False

    def __init__(self, convs, device, impl=L.IMPL_AUTO):
        self.dt, self.dtype, self.device, self.impl = L.DT_F32, torch.float32, torch.device(device), impl
        _lay_out(self, convs, torch.float32)
        self._stamp = self._items = None

    def prepare(self):
        vs = [s.module.v for s in self.slots]
        stamp = tuple((v.data_ptr(), v._version) for v in vs)
        if stamp == self._stamp:
            return
        items, rows = [], []
        for i, (s, v) in enumerate(zip(self.slots, vs)):
            if v.dtype != torch.float32 or not v.is_contiguous() or v.device != self.device:
                raise L.EvtError("FrozenBank: contiguous fp32 weights on the bank's device expected")
            it = L.WPrepItem()
            it.v, it.g, it.reg, it.alt = v.data_ptr(), None, s.reg.data_ptr(), s.alt.data_ptr()
            it.dw = it.dv = it.dg = None
            it.lay, it.dtype = s.layout, self.dt
            items.append(it)
            rows.extend((i, r) for r in range(s.layout.d0))
        self._items = L.struct_to_device(items, self.device)
        self._rows = torch.tensor(rows, dtype=torch.int32, device=self.device).contiguous()
        L.check(L.lib().evt_wn_fold_multi(L.ptr(self._items), L.ptr(self._rows), len(rows), L.stream_ptr()),
                "evt_wn_fold_multi")
        self._stamp = stamp

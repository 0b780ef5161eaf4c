"""Grouped weight-gradient launches (evt_conv1d_bwd_weight_group, hip/wgrad.py::_bwd_weight_group).

Operands are small integers (tests/exact_inputs.py::small_int): every product and every partial sum is an integer far
below 2^24, so fp32 accumulation is exact in any order and the grouped result has to be BIT-EQUAL to the single launches and
to an integer reference computed on the host, whatever the splits -- the idiom of
tests/test_exact_int_gpu.py::test_wgrad_exact_under_every_reduction.  The members of a group that reach wgrad_ring are
launched together; wgrad_deep / wgrad_halo members (and everything else) go through the single path inside the same call,
so their cases check the routing and the bookkeeping of the group entry.
"""
import os

import pytest
import torch
import torch.nn.functional as F

import exact_inputs as X

pytestmark = pytest.mark.gpu
DT = dict(bf16=torch.bfloat16, f16=torch.float16, f32=torch.float32)

# (cin, cout, k, stride, pad, dil, transposed, weight_norm)
R5 = (64, 128, 5, 1, 2, 1, False, False)
R1 = (64, 128, 1, 1, 0, 1, False, False)
R1N = (64, 64, 1, 1, 0, 1, False, False)
R1W = (128, 256, 1, 1, 0, 1, False, False)       # 16 tiles each: sixteen of them need no split
FAMILIES = {
    # name: (members, nseq, L)
    "ring5": ([R5, R5, (64, 128, 5, 1, 2, 1, False, True)], 3, 200),          # 600 positions: tail stage of 24 rows
    "ring1": ([R1, R1N, R1], 3, 200),                                          # different tile counts in one launch, bias fused
    "deep": ([(128, 128, 7, 1, 9, 3, False, False), (128, 128, 11, 1, 5, 1, False, False)], 2, 8200),
    "halo": ([(64, 64, 3, 1, 1, 1, False, False), (64, 64, 7, 1, 9, 3, False, False),
              (64, 64, 11, 1, 25, 5, False, False)], 2, 600),
    "one": ([R5], 3, 200),
    "wn_in": ([(192, 384, 5, 1, 2, 1, False, False)] * 4, 4, 200),            # four WN in_layers: 144 tiles of 64 x (5 x 32)
    "sixteen": ([R1W] * 16, 3, 200),
    "seventeen": ([R1W] * 17, 3, 200),
    "mixed": ([R5, (64, 32, 2, 2, 0, 1, True, False), R1, R5], 3, 200),       # a k2 s2 transposed conv in the middle
}


def lout(spec, L):
    cin, cout, k, s, pad, dil, tr, wn = spec
    return (L - 1) * s - 2 * pad + dil * (k - 1) + 1 if tr else (L + 2 * pad - dil * (k - 1) - 1) // s + 1


class Setup:
    """the modules of one family in one bank, integer operands per member, and the host reference"""

    def __init__(self, gpu, name, dn, random=False):
        from easevoice_trainer_amd.hip import conv as HC
        from easevoice_trainer_amd.hip import lib as L

        self.HC, self.L, self.gpu = HC, L, gpu
        self.dtype, self.random = DT[dn], random
        L.set_half(self.dtype)
        specs, self.nseq, self.lin = FAMILIES[name]
        self.specs, self._ref = specs, {}
        g = X.gen("wgrad_group", name, random)
        mods = []
        for cin, cout, k, s, pad, dil, tr, wn in specs:
            m = HC.EvtConv1d(cin, cout, k, s, pad, dil, 1, bias=True, transposed=tr, weight_norm=wn)
            with torch.no_grad():
                w = X.dense_pm(tuple(m.v.shape), g)
                m.v.copy_(w)
                if wn:
                    m.weight_g.copy_(X.weight_g_of(w))
            mods.append(m)
        self.mods = torch.nn.ModuleList(mods).to(gpu)
        self.bank = HC.WeightBank(self.mods, self.dtype, gpu)
        self.bank.build_tables()
        self.bank.fold()
        self.bank.defer_n = 0
        self.x, self.dy = [], []          # reference layout [nseq, C, L], float64
        for spec in specs:
            shape_x, shape_dy = (self.nseq, spec[0], self.lin), (self.nseq, spec[1], lout(spec, self.lin))
            if random:
                x = torch.randn(shape_x, generator=g, dtype=torch.float64).to(self.dtype).double()
                dy = torch.randn(shape_dy, generator=g, dtype=torch.float64).to(self.dtype).double()
            else:
                x, dy = X.small_int(shape_x, g), X.small_int(shape_dy, g)
            self.x.append(x)
            self.dy.append(dy)
        self.args = [HC.WgJob(m._slot, self.dev(x), self.dev(dy), None, self.nseq, self.lin, 1.0, L.ACT_NONE, 1.0)
                     for m, x, dy in zip(self.mods, self.x, self.dy)]

    def dev(self, t):
        return t.transpose(1, 2).contiguous().to(self.gpu, self.dtype)

    def reference(self, i):
        """(dW, db) of member i: autograd of torch's convolution in float64 (fp32 for the long reductions: as exact)"""
        if i in self._ref:
            return self._ref[i]
        cin, cout, k, s, pad, dil, tr, wn = self.specs[i]
        dt = torch.float32 if (self.nseq * self.lin > 4096 and not self.random) else torch.float64
        x, dy = self.x[i].to(dt), self.dy[i].to(dt)
        w = torch.zeros(tuple(self.mods[i].v.shape), dtype=dt, requires_grad=True)
        y = F.conv_transpose1d(x, w, None, s, pad, 0, 1, dil) if tr else F.conv1d(x, w, None, s, pad, dil)
        (dw,) = torch.autograd.grad(y, w, dy)
        self._ref[i] = dw.double(), dy.sum((0, 2)).double()
        return self._ref[i]

    def run(self, grouped, times=1, zero=True, members=None, finish=True):
        """launch the members' weight gradients `times` times, then the gradient pass; returns per member
        (v.grad, g.grad or None, bias.grad) as fp32 CPU tensors, the device `used` pairs and the host's counts"""
        HC, bank = self.HC, self.bank
        args = self.args if members is None else [self.args[i] for i in members]
        if zero:
            for p in self.mods.parameters():
                if p.grad is not None:
                    p.grad.zero_()
            bank.zero_dw()
        for _ in range(times):
            if grouped:
                HC._bwd_weight_group(args)
            else:
                for a in args:
                    HC._bwd_weight(*a)
        bank.join_side()
        torch.cuda.synchronize()
        used_dev = [tuple(a.slot.used.cpu().tolist()) for a in args]
        used_host = [a.slot.wg_used for a in args]
        if not finish:           # (the gradient pass folds the slabs into slab 0: exactly once per backward)
            return None, used_dev, used_host
        bank.grads()
        torch.cuda.synchronize()
        grads = []
        for m in self.mods:
            gg = m.weight_g.grad if m.weight_norm else None
            grads.append((m.v.grad.detach().float().cpu().clone(), gg.detach().float().cpu().clone() if gg is not None else None,
                          m.bias.grad.detach().float().cpu().clone()))
        return grads, used_dev, used_host


def assert_same(a, b, what):
    for i, (ga, gb) in enumerate(zip(a, b)):
        for ta, tb, n in zip(ga, gb, ("v.grad", "g.grad", "bias.grad")):
            if ta is None:
                assert tb is None
                continue
            assert torch.equal(ta, tb), f"{what}: member {i} {n}: {int((ta != tb).sum())} of {ta.numel()} elements differ"


def assert_reference(s, grads, scale, what):
    for i, (spec, (dv, dg, db)) in enumerate(zip(s.specs, grads)):
        dw_ref, db_ref = s.reference(i)
        if not spec[7]:          # a weight-normed member shows projections of dW: judged against the single launch alone
            assert torch.equal(dv.double().reshape(dw_ref.shape), scale * dw_ref), f"{what}: member {i} dW"
        if not spec[6]:
            assert torch.equal(db.double(), scale * db_ref), f"{what}: member {i} db"


@pytest.mark.parametrize("dn", ["bf16", "f16"])
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_group_equals_single_launches_and_reference(gpu, name, dn):
    s = Setup(gpu, name, dn)
    try:
        single, used_s, _ = s.run(grouped=False)
        group, used_dev, used_host = s.run(grouped=True)
        assert_same(group, single, f"{name} {dn}")
        assert_reference(s, group, 1.0, f"{name} {dn} grouped")
        assert_reference(s, single, 1.0, f"{name} {dn} single")
        # what the kernels recorded per member is what the call returned to the host
        for i, ((u0, u1), uh) in enumerate(zip(used_dev, used_host)):
            assert u0 == uh, (name, i, u0, uh)
            if uh > 0 and not s.specs[i][6]:
                assert u1 == uh, (name, i, u1, uh)
        if name in ("sixteen", "seventeen"):
            # sixteen convolutions of 16 tiles fill the chip without a split; the seventeenth is a launch of its own
            assert used_host[:16] == [1] * 16 and max(u[0] for u in used_s) == 3, (used_host, used_s)
            assert used_host[16:] == [u[0] for u in used_s[16:]]
        if name == "one":
            assert used_host == [u[0] for u in used_s]
    finally:
        s.L.set_half(torch.bfloat16)


@pytest.mark.parametrize("dn", ["bf16", "f16"])
def test_group_accumulates_into_dirty_slabs(gpu, dn):
    s = Setup(gpu, "sixteen", dn)
    try:
        # the same group twice without zero_dw: every slab is added to
        twice, _, used = s.run(grouped=True, times=2)
        assert_reference(s, twice, 2.0, "group twice")
        # single launches (three slabs each), then the group (no split): prev_used > nsplit, slabs 1 and 2 keep their sums
        s.run(grouped=False, finish=False)
        after, used_dev, used_host = s.run(grouped=True, zero=False)
        assert used_host == [3] * 16 and [u[0] for u in used_dev] == [3] * 16
        assert_reference(s, after, 2.0, "single then group")
    finally:
        s.L.set_half(torch.bfloat16)


@pytest.mark.parametrize("dn", ["bf16", "f16"])
def test_member_with_one_slab(gpu, dn):
    s = Setup(gpu, "ring5", dn)
    try:
        s.mods[1]._slot.parts = 1           # before its first launch: the slot's record is built from it
        group, used_dev, used_host = s.run(grouped=True)
        assert used_host[1] == 1 and used_dev[1][0] == 1
        assert_reference(s, group, 1.0, "parts = 1")
        single, _, _ = s.run(grouped=False)
        assert_same(group, single, "parts = 1")
    finally:
        s.L.set_half(torch.bfloat16)


def test_fp32_members_keep_the_single_path(gpu):
    s = Setup(gpu, "ring1", "f32")
    group, _, used = s.run(grouped=True)
    single, _, _ = s.run(grouped=False)
    assert_same(group, single, "fp32")
    assert_reference(s, group, 1.0, "fp32")


@pytest.mark.parametrize("name", ["ring5", "ring1", "deep", "halo"])
def test_random_operands_within_the_conv_bound(gpu, name):
    """one random-data case per family: grouped and single against float64, with the bound tests/test_conv_gpu.py applies
    to 16-bit weight gradients (relative to the reference's largest magnitude: 3e-2 in bf16)"""
    s = Setup(gpu, name, "bf16", random=True)
    tol = 3e-2
    for grouped in (True, False):
        grads, _, _ = s.run(grouped=grouped)
        for i, (spec, (dv, dg, db)) in enumerate(zip(s.specs, grads)):
            if spec[7]:
                continue
            dw_ref, db_ref = s.reference(i)
            for got, ref, n in ((dv.double().reshape(dw_ref.shape), dw_ref, "dW"), (db.double(), db_ref, "db")):
                err = (got - ref).abs().max().item() / (ref.abs().max().item() + 1e-6)
                print(f"{name} grouped={grouped} member {i} {n}: rel err {err:.3e}")
                assert err < tol, (name, grouped, i, n, err)


def _wn_model(gpu, dtype):
    from easevoice_trainer_amd.hip import conv as HC
    from easevoice_trainer_amd.module.models import WN

    torch.manual_seed(3)
    mods = torch.nn.ModuleList([WN(192, 5, 1, 4, gin_channels=0), WN(192, 5, 1, 3, gin_channels=0),
                                HC.EvtConv1d(192, 64, 1), HC.EvtConv1d(64, 64, 7, padding=3), HC.EvtConv1d(64, 64, 7, padding=3)])
    mods = mods.to(gpu)
    bank = HC.WeightBank(mods, dtype, gpu)
    bank.build_tables()
    bank.fold()
    return mods, bank


def _wn_backward(mods, bank, x0, live, lens, wgt):
    from easevoice_trainer_amd.hip import conv as HC

    for p in mods.parameters():
        if p.grad is not None:
            p.grad.zero_()
    bank.zero_dw()
    x = x0.clone().requires_grad_(True)
    h = mods[0](x, live, lens=lens)
    h = mods[1](h, live, lens=lens)
    h = mods[2](h)
    h = HC.res_unit(h, mods[3], mods[4], 0.5)      # a wide (C = 64) vocoder unit behind the stacks
    (h.float() * wgt).sum().backward()
    bank.grads()
    torch.cuda.synchronize()
    return {n: p.grad.detach().float().cpu().clone() for n, p in mods.named_parameters()}


@pytest.mark.parametrize("dn", ["bf16", "f16"])
def test_queue_and_stream_order_give_identical_gradients(gpu, dn):
    """two WN stacks and a wide unit: the backward with the weight gradients deferred to the side stream (groups are queue
    entries), in stream order (EVT_WGRAD_DEFER=0) and with every gradient queued on its own -- the first two bit-equal (same
    launches, other stream); the third differs by the summation order of other splits alone"""
    from easevoice_trainer_amd.hip import conv as HC
    from easevoice_trainer_amd.hip import lib as L
    from easevoice_trainer_amd.hip import wn as W

    dtype = DT[dn]
    L.set_half(dtype)
    old = os.environ.get("EVT_WGRAD_DEFER")
    try:
        B, T = 4, 200
        lens = torch.tensor([T, 150, 64, 33], device=gpu, dtype=torch.int32)
        live = (torch.arange(T, device=gpu)[None, :] < lens[:, None]).float().unsqueeze(-1)
        torch.manual_seed(5)
        x0 = (torch.randn(B, T, 192, device=gpu) * live).to(dtype)
        wgt = torch.randn(B, T, 64, device=gpu)
        res = {}
        for mode in ("deferred", "stream", "ungrouped"):
            os.environ.pop("EVT_WGRAD_DEFER", None)
            if mode == "stream":
                os.environ["EVT_WGRAD_DEFER"] = "0"
            mods, bank = _wn_model(gpu, dtype)
            assert (bank.defer_n > 0) == (mode != "stream")
            W.GROUP_WGRADS = mode != "ungrouped"
            seen = []
            orig = HC._bwd_weight_group

            def spy(members):
                seen.append(len(members))
                return orig(members)

            HC._bwd_weight_group = spy
            try:
                res[mode] = _wn_backward(mods, bank, x0, live.to(dtype), lens, wgt)
            finally:
                HC._bwd_weight_group = orig
            # declared by the stacks themselves, GROUP_LAYERS layers at a time: the three-layer stack (last in the forward,
            # first in the backward) hands over 2 + 1 layers, the four-layer stack 2 + 2
            n = 2 * W.GROUP_LAYERS
            want = [n, 6 - n, n, 8 - n] if W.GROUP_LAYERS == 2 else None
            assert W.GROUP_LAYERS == 2 and seen == ([] if mode == "ungrouped" else want), (mode, seen)
            assert not bank.wgq.pending and not bank.wgq.held
        for n, a in res["deferred"].items():
            assert torch.equal(a, res["stream"][n]), n
            b = res["ungrouped"][n]
            err = (a - b).abs().max().item() / (b.abs().max().item() + 1e-6)
            assert err < 1e-5, (n, err)            # fp32 sums of the same products in another order
    finally:
        W.GROUP_WGRADS = True
        os.environ.pop("EVT_WGRAD_DEFER", None) if old is None else os.environ.__setitem__("EVT_WGRAD_DEFER", old)
        L.set_half(torch.bfloat16)


def test_zero_dw_drops_an_abandoned_group(gpu):
    s = Setup(gpu, "ring5", "bf16")
    s.bank.defer_n = 48
    s.HC._bwd_weight_group(s.args)         # stays in the queue, as behind a backward that never reached grads()
    assert len(s.bank.wgq.pending) == 1 and isinstance(s.bank.wgq.pending[0], s.HC.WgGroup) and len(s.bank.wgq.pending[0]) == 3
    s.bank.zero_dw()
    assert not s.bank.wgq.pending and not s.bank.wgq.held and s.bank.wgq.nbytes == 0
    s.bank.defer_n = 0
    group, _, _ = s.run(grouped=True)
    assert_reference(s, group, 1.0, "after an abandoned group")


def test_traced_group_is_single_launches(gpu):
    s = Setup(gpu, "ring5", "bf16")
    for defer in (0, 48):
        s.bank.defer_n = defer
        rec = []
        s.HC.set_trace(rec)
        try:
            grads, _, _ = s.run(grouped=True)
        finally:
            s.HC.set_trace(None)
        tags = [r[0] for r in rec if r[1] == "bwd_weight"]
        assert len(tags) == 3 and all(t.startswith("wgrad_ring<") and "group" not in t for t in tags), tags
        assert not s.bank.wgq.pending
        assert_reference(s, grads, 1.0, "traced")


def test_captured_group_replays_on_new_operands(gpu):
    """a WN-shaped group (four in_layers 192 -> 384 k5, 800 positions) with deferral on, captured in a HIP graph: the member
    table travels in the kernel arguments, so each replay must equal an eager run on the operands then in place"""
    s = Setup(gpu, "wn_in", "bf16")
    bank, HC = s.bank, s.HC
    bank.defer_n = 48

    def step():
        for p in s.mods.parameters():
            if p.grad is not None:
                p.grad.zero_()
        bank.zero_dw()
        HC._bwd_weight_group(s.args)
        bank.grads()

    step()                                  # eager once: streams, scratch and kernel attributes exist before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    g = X.gen("wgrad_group", "replay")
    for rep in range(2):
        s._ref.clear()
        for i, a in enumerate(s.args):
            s.x[i], s.dy[i] = X.small_int(tuple(s.x[i].shape), g), X.small_int(tuple(s.dy[i].shape), g)
            a.x.copy_(s.dev(s.x[i]))
            a.dy.copy_(s.dev(s.dy[i]))
        graph.replay()
        torch.cuda.synchronize()
        got = [(m.v.grad.detach().float().cpu().clone(), None, m.bias.grad.detach().float().cpu().clone()) for m in s.mods]
        assert_reference(s, got, 1.0, f"replay {rep}")
        bank.defer_n = 0
        eager, _, _ = s.run(grouped=True)
        bank.defer_n = 48
        assert_same(got, eager, f"replay {rep} against eager")

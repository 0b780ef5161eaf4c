"""CPU: the host side of the wide decode sessions (5..32 rows in one session, auto_reg/t2s_infer.py) with the launches
emulated on the session's buffers (tests/cpu_emu.py): which sessions a batch builds, the reference's token lists for 20
and 36 texts (tests/golden/s1_batch_infer_rows.pt), the per-row seed table and the bound on the wide-session cache."""
import os
import sys

import pytest
import torch
import yaml

from cpu_emu import cpu_emulation_decode
from util_fill import fill_module

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))


def _model():
    from easevoice_trainer_amd.auto_reg.t2s_model import Text2SemanticDecoder

    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "gpt.yaml")))
    m = Text2SemanticDecoder(cfg)
    fill_module(m, 3)
    m.eval()
    return m


def _call(m, d, rows, **kw):
    kw = {**dict(top_k=1100, top_p=1, temperature=1.0, repetition_penalty=1.35, early_stop_num=3), **kw}
    return m.infer_panel_batch_infer([d["x"][r] for r in rows], d["x_lens"][rows], d["prompts"][rows],
                                     [d["bert"][r] for r in rows], noise=d["q"][:, rows], **kw)


class _Count:
    """records the row count of every DecodeSession built while active"""

    def __enter__(self):
        from easevoice_trainer_amd.auto_reg import t2s_infer as TI

        self.TI, self.orig, self.built = TI, TI.DecodeSession, []
        built = self.built

        class Counted(self.orig):
            def __init__(self, model, B, *a, **k):
                built.append(B)
                super().__init__(model, B, *a, **k)

        TI.DecodeSession = Counted
        return self

    def __exit__(self, *exc):
        self.TI.DecodeSession = self.orig


def test_rows_sessions_and_reference_tokens():
    """20 texts: ONE session of 20 rows; 36 texts: one of 32 and one of 4 -- and both come out token for token as the
    reference's infer_panel_batch_infer decodes them (rows stopping from step 1 on, the first two at the early stop)"""
    from make_golden_s1_rows import rows_inputs

    gold = {c["args"]["R"]: c for c in torch.load(os.path.join(HERE, "golden", "s1_batch_infer_rows.pt"),
                                                   weights_only=False)["cases"]}
    with cpu_emulation_decode():
        for R, want_built in ((20, [20]), (36, [32, 4])):
            model = _model()
            d = rows_inputs(R)
            a = {k: v for k, v in gold[R]["args"].items() if k != "R"}
            with _Count() as c:
                ys, idxs = _call(model, d, list(range(R)), **a)
            assert c.built == want_built, (R, c.built)
            assert idxs == gold[R]["idx"], (R, idxs)
            assert len(ys) == R
            for r, (y, g) in enumerate(zip(ys, gold[R]["y"])):
                assert torch.equal(y.long(), g.long()), (R, r)


def test_rows_seed_table():
    """a wide session keys row b's built-in noise by (seed of its group of four, b % 4): seed + 4 * (b // 4) masked to
    31 bits, or -- without a seed -- one draw of torch's CPU generator per group of four, in order"""
    from make_golden_s1_rows import rows_inputs

    d = rows_inputs(20)
    rows = list(range(10))
    with cpu_emulation_decode():
        m = _model()
        s = 0x7FFFFFFE
        _call(m, d, rows, seed=s, early_stop_num=1)
        (S,) = m._infer()._sessions.values()
        want = [[(s + 4 * (b // 4)) & 0x7FFFFFFF, b % 4] for b in range(10)]
        assert S.B == 10 and S.row_seed.tolist() == want
        assert want[4][0] == 2                      # 0x7FFFFFFE + 4 wraps as the per-group seed of four rows did
        torch.manual_seed(31)
        _call(m, d, rows, early_stop_num=1)
        torch.manual_seed(31)
        draws = [int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) for _ in range(3)]
        assert S.row_seed.tolist() == [[draws[b // 4], b % 4] for b in range(10)]


def test_rows_wide_session_cache_is_bounded():
    """sessions of 5..32 rows are cached least-recently-used, two at most; sessions of <= 4 rows as before"""
    from make_golden_s1_rows import rows_inputs

    d = rows_inputs(20)
    with cpu_emulation_decode():
        m = _model()
        for n in (5, 6, 7):
            _call(m, d, list(range(n)), early_stop_num=1)
        assert sorted(k[0] for k in m._infer()._sessions) == [6, 7]
        _call(m, d, [0, 1], early_stop_num=1)      # a narrow session does not displace a wide one
        _call(m, d, list(range(6)), early_stop_num=1)
        _call(m, d, list(range(8)), early_stop_num=1)   # 7 is now the least recently used
        assert sorted(k[0] for k in m._infer()._sessions) == [2, 6, 8]

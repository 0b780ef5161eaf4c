"""s1 fixture of per-request sampling parameters: the REFERENCE's infer_panel_batch_infer (t2s_model.py:563-730) on the
12 texts of make_golden_s1_rows.rows_inputs(12), once per parameter set, fp32, fill_module(model, 3) weights, with the
per-row noise table of that module and early_stop_num = 12.  Request r of a mixed session is expected to decode as row r
of the run with set r % 4 (rows are independent in the reference's batch path).

    set  top_k       top_p  temperature  repetition_penalty
    A    1100        1      1.0          1.35      the set of the existing fixtures
    B    5           1      0.7          1.35      small top-k, lower temperature
    C    -100 (off)  0.8    1.0          1.0       the nucleus branch and the skipped-penalty branch
    D    15          0.9    1.3          1.2       all branches together

The noise table forces EOS by a tiny q in the EOS column; under a small top-k or a nucleus cut the EOS column may have
probability 0 there, so rows do not leave the reference's batch from the back as in make_golden_s1_rows.py.  The stand-in
sampler therefore follows the reference's own compaction (rows whose sample or arg-max is EOS leave) and reads the
noise of the ORIGINAL row, which is what a session reads at that row's table column.

    python tests/golden/make_golden_s1_mixed.py      -> tests/golden/s1_mixed_sampling.pt
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_s1_rows import rows_inputs  # noqa: E402

R, EARLY_STOP = 12, 12
SETS = [dict(top_k=1100, top_p=1, temperature=1.0, repetition_penalty=1.35),
        dict(top_k=5, top_p=1, temperature=0.7, repetition_penalty=1.35),
        dict(top_k=-100, top_p=0.8, temperature=1.0, repetition_penalty=1.0),
        dict(top_k=15, top_p=0.9, temperature=1.3, repetition_penalty=1.2)]


def make():
    import yaml
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle import refshim

    refshim.install()
    sys.path.insert(0, os.path.dirname(HERE))
    from util_fill import fill_module
    from src.easevoice.soundstorm.auto_reg.models import t2s_model as TM
    from src.easevoice.soundstorm.auto_reg.models import utils as U

    torch.set_num_threads(8)
    cfg = yaml.safe_load(open(os.path.join(refshim.REFERENCE_ROOT, "configs", "gpt.yaml")))
    model = TM.Text2SemanticDecoder(config=cfg, top_k=3)
    fill_module(model, 3)
    model.eval()
    d = rows_inputs(R)
    state = dict(step=0, alive=list(range(R)))

    def sample_one(probs):
        assert probs.size(0) == len(state["alive"])
        qrow = d["q"][state["step"]][state["alive"], :probs.size(-1)]
        return torch.argmax(probs / qrow, dim=-1, keepdim=True).to(dtype=torch.int)

    orig_sample, orig_one = TM.sample, U.multinomial_sample_one_no_sync

    def sample(logits, previous_tokens=None, **kw):
        out = orig_sample(logits, previous_tokens, **kw)
        # t2s_model.py:676-690: the penalty was applied to `logits` in place, rows with EOS leave the batch
        gone = (out[0][:, 0] == model.EOS).logical_or(torch.argmax(logits, dim=-1) == model.EOS).tolist()
        state["alive"] = [r for r, g in zip(state["alive"], gone) if not g]
        state["step"] += 1
        return out

    TM.sample, U.multinomial_sample_one_no_sync = sample, sample_one
    sets = []
    try:
        with torch.no_grad():
            for c in SETS:
                state["step"], state["alive"] = 0, list(range(R))
                # "off" is top_k = None in the reference's sample() (its torch.topk takes no negative k); this project's
                # entry points spell it top_k <= 0, which is what the fixture records
                kw = dict(c, top_k=c["top_k"] if c["top_k"] > 0 else None)
                ys, idxs = model.infer_panel_batch_infer(d["x"], d["x_lens"], d["prompts"], d["bert"],
                                                         max_len=int(d["x_lens"].max()), early_stop_num=EARLY_STOP, **kw)
                idxs = [int(i) for i in idxs]
                sets.append(dict(args=c, y=[y.clone().to(torch.int16) for y in ys], idx=idxs, steps=state["step"]))
                print(c, "-> idx", idxs, "steps", state["step"])
    finally:
        TM.sample, U.multinomial_sample_one_no_sync = orig_sample, orig_one
    torch.save(dict(R=R, early_stop_num=EARLY_STOP, sets=sets), os.path.join(HERE, "s1_mixed_sampling.pt"))


if __name__ == "__main__":
    make()

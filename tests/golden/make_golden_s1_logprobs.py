"""s1 fixture of candidates and per-token log-probabilities: the REFERENCE's infer_panel_batch_infer
(t2s_model.py:563-730) on 12 rows = 4 texts x 3 candidates, fp32, fill_module(model, 3) weights, early_stop_num = 12.
Row 3r + c is text r of make_golden_s1_rows.rows_inputs(12) with its prompt and reads noise column 3r + c of that
module's table, which forces EOS at different steps per row: candidate c of request r of a stream session is expected to
decode as row 3r + c (rows are independent in the reference's batch path).  Two parameter sets are recorded, A and D of
make_golden_s1_mixed.py.  Set D's top_k = 15 cuts the forced EOS out of every row, so all 12 rows of set D run to the
limit (idx = 12): set D covers the sampler's values under a top-k cut and a full-length run, while EOS stops at
different steps, and with them the staggered refill of a stream session, are covered by set A alone.

Per step and alive row the stand-in around sample() records
    model    log_softmax(logits, -1)[token] of the logits AS THEY ARRIVE (sample() penalises them in place),
    sampler  log(probs[token]) of the probabilities sample() draws from (after penalty, nucleus, top-k, temperature),
following the reference's batch compaction as make_golden_s1_mixed.py does.  Tokens are stored as int16, the
log-probabilities as fp32 [steps of the row][2].

    python tests/golden/make_golden_s1_logprobs.py      -> tests/golden/s1_logprobs.pt
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_s1_rows import rows_inputs  # noqa: E402
from make_golden_s1_mixed import SETS  # noqa: E402

TEXTS, CANDS, EARLY_STOP = 4, 3, 12
R = TEXTS * CANDS
SETS_USED = {"A": SETS[0], "D": SETS[3]}


def candidate_inputs():
    """the 12 rows: text r = row // 3 of rows_inputs(12), noise column = row"""
    d = rows_inputs(R)
    src = [row // CANDS for row in range(R)]
    return dict(x=[d["x"][r] for r in src], bert=[d["bert"][r] for r in src], x_lens=d["x_lens"][src],
                prompts=d["prompts"][src].contiguous(), q=d["q"])


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
    d = candidate_inputs()
    state = dict(step=0, alive=list(range(R)), lp=None, probs=None)

    def sample_one(probs):
        assert probs.size(0) == len(state["alive"])
        state["probs"] = probs.clone()
        qrow = d["q"][state["step"]][state["alive"], :probs.size(-1)]
        return torch.argmax(probs / qrow, dim=-1, keepdim=True).to(dtype=torch.int)

    orig_sample, orig_one = TM.sample, U.multinomial_sample_one_no_sync

    def sample(logits, previous_tokens=None, **kw):
        raw = logits.clone()                      # the original penalises `logits` in place
        out = orig_sample(logits, previous_tokens, **kw)
        tok = out[0][:, :1].long()
        model_lp = torch.log_softmax(raw, -1).gather(1, tok)[:, 0]
        samp_lp = torch.log(state["probs"].gather(1, tok)[:, 0])
        for k, row in enumerate(state["alive"]):
            state["lp"][row].append([float(model_lp[k]), float(samp_lp[k])])
        # t2s_model.py:676-690: rows with EOS (sample or arg-max of the penalised logits) leave the batch
        gone = (out[0][:, 0] == model.EOS).logical_or(torch.argmax(logits, dim=-1) == model.EOS).tolist()
        state["alive"] = [r for r, g in zip(state["alive"], gone) if not g]
        state["step"] += 1
        return out

    TM.sample, U.multinomial_sample_one_no_sync = sample, sample_one
    sets = {}
    try:
        with torch.no_grad():
            for name, c in SETS_USED.items():
                state.update(step=0, alive=list(range(R)), lp=[[] for _ in range(R)])
                kw = dict(c, top_k=c["top_k"] if c["top_k"] > 0 else None)
                ys, idxs = model.infer_panel_batch_infer(d["x"], d["x_lens"], d["prompts"], d["bert"],
                                                         max_len=int(d["x_lens"].max()), early_stop_num=EARLY_STOP, **kw)
                idxs = [int(i) for i in idxs]
                lps = [torch.tensor(v, dtype=torch.float32).reshape(-1, 2) for v in state["lp"]]
                sets[name] = dict(args=c, y=[y.clone().to(torch.int16) for y in ys], idx=idxs, logprobs=lps)
                print(name, c, "-> idx", idxs, "steps per row", [int(v.size(0)) for v in lps])
    finally:
        TM.sample, U.multinomial_sample_one_no_sync = orig_sample, orig_one
    torch.save(dict(texts=TEXTS, candidates=CANDS, early_stop_num=EARLY_STOP, sets=sets),
               os.path.join(HERE, "s1_logprobs.pt"))


if __name__ == "__main__":
    make()

"""s1 fixture of the wide batch path: the REFERENCE's infer_panel_batch_infer (t2s_model.py:563-730, the TTS default) on
20 and on 36 texts sharing one prompt, fp32, fill_module(model, 3) weights.  Stand-in sampler as in make_golden_s1.py: the
exponential noise comes from a seeded table, one row per text.

The reference compacts finished rows out of its batch, so the table is indexed by the surviving prefix of the rows: the
EOS schedule makes rows stop from the back (row r at step stop_step(r, R), non-increasing in r; at least two rows stop
at step 1, where the batch path first keeps the EOS column; rows 0 and 1 run into early_stop_num).  The script asserts
that the planned stops came out.  rows_inputs() regenerates the inputs for the tests (build container only for this
file's __main__: it imports the reference).

    python tests/golden/make_golden_s1_rows.py      -> tests/golden/s1_batch_infer_rows.pt
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
EARLY_STOP = 14
CASES = [dict(R=20, top_k=1100, top_p=1, temperature=1.0, repetition_penalty=1.35, early_stop_num=EARLY_STOP),
         dict(R=36, top_k=1100, top_p=1, temperature=1.0, repetition_penalty=1.35, early_stop_num=EARLY_STOP)]


def stop_step(r, R):
    """planned EOS step of row r of R (None: no EOS, the row reaches early_stop_num)"""
    if r < 2:
        return None
    return max(1, EARLY_STOP - 1 - ((r - 2) * (EARLY_STOP - 1)) // (R - 3))


def rows_inputs(R, seed=2032):
    """R texts of 8..24 ids (row 0 the longest), one shared 12-token prompt, noise q[step][row][v] with the EOS schedule"""
    g = torch.Generator().manual_seed(seed)
    lens = [24 - (7 * r) % 17 for r in range(R)]
    x = [torch.randint(0, 732, (n,), generator=g) for n in lens]
    bert = [torch.randn(1024, n, generator=g) for n in lens]
    prompt = torch.randint(0, 1024, (1, 12), generator=g)
    q = torch.empty(EARLY_STOP + 2, R, 1025).exponential_(1, generator=torch.Generator().manual_seed(seed + R))
    for r in range(R):
        s = stop_step(r, R)
        if s is not None:
            q[s, r, 1024] = 1e-30
    return dict(x=x, bert=bert, x_lens=torch.tensor(lens), prompts=prompt.expand(R, -1).contiguous(), q=q)


def expected_idx(R):
    """index convention of infer_panel_batch_infer: idx - 1 for an EOS stop, idx for the early stop"""
    return [EARLY_STOP if stop_step(r, R) is None else stop_step(r, R) - 1 for r in range(R)]


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
    state = dict(step=0, q=None)

    def sample_one(probs):
        qrow = state["q"][state["step"]][:probs.size(0), :probs.size(-1)]     # survivors are a prefix of the rows
        state["step"] += 1
        return torch.argmax(probs / qrow, dim=-1, keepdim=True).to(dtype=torch.int)

    orig = U.multinomial_sample_one_no_sync
    U.multinomial_sample_one_no_sync = sample_one
    cases = []
    try:
        with torch.no_grad():
            for c in CASES:
                R = c["R"]
                d = rows_inputs(R)
                state["step"], state["q"] = 0, d["q"]
                kw = {k: v for k, v in c.items() if k != "R"}
                ys, idxs = model.infer_panel_batch_infer(d["x"], d["x_lens"], d["prompts"], d["bert"],
                                                         max_len=int(d["x_lens"].max()), **kw)
                idxs = [int(i) for i in idxs]
                assert idxs == expected_idx(R), (R, idxs, expected_idx(R))
                cases.append(dict(args=c, y=[y.clone() for y in ys], idx=idxs, steps=state["step"]))
                print(c, "-> idx", idxs, "steps", state["step"])
    finally:
        U.multinomial_sample_one_no_sync = orig
    torch.save(dict(cases=cases), os.path.join(HERE, "s1_batch_infer_rows.pt"))


if __name__ == "__main__":
    make()

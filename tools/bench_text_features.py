"""Throughput of the phone-level BERT features (Chinese-RoBERTa, BERT-large dimensions, hidden_states[-3]):
BertFeatures.phone_level_feature one sentence at a time -- the single-sentence path, with its five small launches and a device
synchronisation behind every sentence -- against BertFeatures.phone_level_features_batch in groups of 1, 4, 8, 16 and 32
(one upload, one embedding launch, one pass of the 22 layers, one expanding launch and one device -> host copy per group),
in the same process.

Workload: 256 synthetic sentences of 5..120 characters (seeded lengths and ids, word2ph of 1..3 phones per character),
random-init weights of the real dimensions (vocabulary cut to 2048 rows: the gather does not depend on the table's
height), bf16 and fp32.  Both paths end with float32 [1024, n] features on the host.

Protocol: every mode runs once untimed, then --reps timed passes with the modes alternated; a pass is timed on the host
clock between two device synchronisations.  Reported per mode: the median pass, sentences/s, the spread (min / max seconds)
and the ratio to the `one_at_a_time` line of the same run and dtype, which is the yardstick.  `stages_ms`: one more pass per
group size with a synchronisation behind every stage (upload + embedding, encoder layers, column map + expander, copy to
the host), which shows where a larger group stops paying.  `kernels_us`: the two new launches alone per group, device
events, against the torch launches they replace on the same data (the embedding module's three gathers, add, casts and
LayerNorm launch; per sentence the slice, float cast, repeat_interleave and transposing copy).
A measurement path without a GPU fails.

    python tools/bench_text_features.py [--reps 3] [--sentences 256] [--out profiles/bert_batch.json]
"""
import argparse
import json
import os
import random
import sys
import time

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")   # before the HIP runtime loads: easevoice_trainer_amd/__init__.py

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VOCAB = 2048


def workload(n, seed=23):
    rnd = random.Random(seed)
    rs = np.random.RandomState(seed)
    chars = [rnd.randint(5, 120) for _ in range(n)]
    ids = [torch.from_numpy(rs.randint(5, VOCAB, c + 2)) for c in chars]
    word2ph = [rs.randint(1, 4, c).tolist() for c in chars]
    return ids, word2ph


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sentences", type=int, default=256)
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 4, 8, 16, 32])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bert_batch.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_text_features needs a GPU: nothing is measured without one")
    from easevoice_trainer_amd.feature_extractor import BertFeatures
    from easevoice_trainer_amd.feature_extractor.roberta import column_map, length_groups
    from easevoice_trainer_amd.hip import lib as L
    from easevoice_trainer_amd.hip.feat import bert_embed_ln_rows, phone_expand_rows

    dev = torch.device("cuda:0")
    ids, word2ph = workload(args.sentences)
    ids2d = [a.view(1, -1) for a in ids]
    lengths = [a.numel() for a in ids]
    res = {"tool": "tools/bench_text_features.py", "device": torch.cuda.get_device_name(0), "sentences": len(ids),
           "characters_min_max": [min(lengths) - 2, max(lengths) - 2], "tokens": sum(lengths),
           "phones": sum(sum(w) for w in word2ph), "reps": args.reps,
           "timing": "host clock between device synchronisations per pass, modes alternated, one untimed pass of every mode "
                     "first; medians",
           "baseline": "modes.one_at_a_time of the same run and dtype: BertFeatures.phone_level_feature per sentence",
           "dtypes": {}}
    for tag, dtype in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        torch.manual_seed(0)
        bert = BertFeatures(None, dev, dtype, vocab=VOCAB)

        def run_one():
            return [bert.phone_level_feature(a, w) for a, w in zip(ids2d, word2ph)]

        modes = [("one_at_a_time", run_one)]
        modes += [(f"batch{k}", (lambda k=k: bert.phone_level_features_batch(ids, word2ph, group=k))) for k in args.groups]
        for name, fn in modes:
            out = fn()
            assert len(out) == len(ids) and all(o.shape == (1024, sum(w)) for o, w in zip(out, word2ph)), name
            torch.cuda.synchronize()
        times = {name: [] for name, _ in modes}
        for _ in range(args.reps):
            for name, fn in modes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
                print(f"{tag} {name}: {times[name][-1]:.3f} s", file=sys.stderr, flush=True)
        out = {"modes": {}}
        for name, _ in modes:
            v = sorted(times[name])
            med = _median(v)
            out["modes"][name] = {"seconds_median": round(med, 4), "seconds_min": round(v[0], 4), "seconds_max": round(v[-1], 4),
                                  "sentences_per_s": round(len(ids) / med, 1)}
        base = out["modes"]["one_at_a_time"]["seconds_median"]
        for m in out["modes"].values():
            m["ratio_vs_one_at_a_time"] = round(base / m["seconds_median"], 3)

        # ---- the stages of a grouped pass (a synchronisation behind each) and the two new launches alone (device events)
        L.set_half(dtype)
        emb = bert.model.bert.embeddings
        tables = (emb.word_embeddings.weight, emb.position_embeddings.weight, emb.token_type_embeddings.weight,
                  emb.LayerNorm.weight, emb.LayerNorm.bias, emb.LayerNorm.eps, dtype)
        stages, kernels = {}, {}
        with torch.no_grad():
            for k in args.groups:
                st = {"upload_embed": 0.0, "encoder": 0.0, "map_expand": 0.0, "copy": 0.0}
                new_emb, old_emb, new_exp, old_exp = [], [], [], []
                for members in length_groups(lengths, k):
                    B, T = len(members), max(lengths[i] for i in members)

                    def tick(key, t0):
                        torch.cuda.synchronize()
                        st[key] += time.perf_counter() - t0
                        return time.perf_counter()

                    t0 = time.perf_counter()
                    host = np.zeros((B, T), dtype=np.int32)
                    for j, i in enumerate(members):
                        host[j, :lengths[i]] = ids[i].numpy()
                    ids_dev = torch.from_numpy(host).to(dev)
                    lens_dev = torch.tensor([lengths[i] for i in members], dtype=torch.int32).to(dev)
                    x = bert_embed_ln_rows(ids_dev, lens_dev, *tables)
                    t0 = tick("upload_embed", t0)
                    for layer in bert.model.bert.encoder.layer:
                        x = layer(x, lens_dev)
                    t0 = tick("encoder", t0)
                    src, item_off = column_map([[("rows", j * T + 1, word2ph[i])] for j, i in enumerate(members)])
                    src_dev, off_dev = torch.from_numpy(src).to(dev), torch.from_numpy(item_off).to(dev)
                    packed = phone_expand_rows(x, src_dev, off_dev, B, int(item_off[-1]))
                    t0 = tick("map_expand", t0)
                    packed.cpu()
                    tick("copy", t0)
                    # the launches alone, against what they replace
                    ids_long, tt_long = ids_dev.long(), torch.zeros(B, T, dtype=torch.long, device=dev)
                    reps = [torch.as_tensor(word2ph[i], device=dev) for i in members]
                    for rep in range(args.reps + 1):
                        e = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
                        e[0].record()
                        bert_embed_ln_rows(ids_dev, lens_dev, *tables)
                        e[1].record()
                        emb(ids_long, tt_long, dtype)
                        e[2].record()
                        phone_expand_rows(x, src_dev, off_dev, B, int(item_off[-1]))
                        e[3].record()
                        for j, i in enumerate(members):
                            torch.repeat_interleave(x[j, 1:lengths[i] - 1].float(), reps[j], dim=0).T.contiguous()
                        e[4].record()
                        torch.cuda.synchronize()
                        if rep:
                            new_emb.append(e[0].elapsed_time(e[1]) * 1e3)
                            old_emb.append(e[1].elapsed_time(e[2]) * 1e3)
                            new_exp.append(e[2].elapsed_time(e[3]) * 1e3)
                            old_exp.append(e[3].elapsed_time(e[4]) * 1e3)
                stages[f"group{k}"] = {key: round(v * 1e3, 2) for key, v in st.items()}
                kernels[f"group{k}"] = {"bert_embed_ln_rows_us_median": round(_median(new_emb), 1),
                                        "embeddings_module_us_median": round(_median(old_emb), 1),
                                        "phone_expand_rows_us_median": round(_median(new_exp), 1),
                                        "per_sentence_torch_expansion_us_median": round(_median(old_exp), 1)}
        out["stages_ms"] = stages
        out["kernels_us"] = kernels
        res["dtypes"][tag] = out
        del bert
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

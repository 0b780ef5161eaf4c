"""CPU: randomised differential tests of the host-side pieces against the REFERENCE's own code.  They widen what the other
golden fixtures pin (one seeded case each) to a few hundred random cases.  The reference's answers for these cases are
recorded in tests/golden/differential.pt by tests/golden/make_golden_differential.py, which runs the reference's modules
on the inputs the `_*_cases` generators below draw; the tests draw the same inputs, run this repository's code and compare.
Exact comparisons of large tensors are made through digests (dtype, shape, sha256 of the bytes).  Where the reference
consumes a file or state written HERE (checkpoints, optimiser state handed back), the digest of what the generator fed it
is recorded with the reference's answer, and the test checks that this repository still writes exactly that."""
import copy
import functools
import hashlib
import os
import random
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from easevoice_trainer_amd.auto_reg import utils as PU  # noqa: E402
from easevoice_trainer_amd.train import dataset as D  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "differential.pt")


@functools.lru_cache(maxsize=None)
def gold():
    return torch.load(GOLDEN, weights_only=False)


def digest(x):
    """exact identity of a (nested) value: tensors by dtype, shape and bytes, everything else by repr"""
    if torch.is_tensor(x):
        t = x.detach().cpu()
        return ("tensor", str(t.dtype), tuple(t.shape), hashlib.sha256(t.reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest())
    if isinstance(x, dict):
        return ("dict", tuple((repr(k), digest(v)) for k, v in x.items()))
    if isinstance(x, (list, tuple)):
        return (type(x).__name__, tuple(digest(v) for v in x))
    return ("value", repr(x))


def digest_hex(x):
    """one sha256 over digest(x): for values with many tensors (checkpoints, optimiser states)"""
    return hashlib.sha256(repr(digest(x)).encode()).hexdigest()


class Stub(torch.utils.data.Dataset):
    def __init__(self, lengths):
        self.lengths = lengths

    def __len__(self):
        return len(self.lengths)

    def get_sample_length(self, i):
        return self.lengths[i]


def _s2_sampler_cases():
    """(case, lengths, bounds, bs, world, rank, epochs)"""
    rng = random.Random(1)
    for case in range(40):
        n = rng.randint(5, 400)
        lengths = [rng.randint(1, 2300) for _ in range(n)]
        bounds = sorted(rng.sample(range(10, 2200), rng.randint(2, 12)))
        bs, world = rng.randint(1, 9), rng.randint(1, 4)
        inside = [v for v in lengths if bounds[0] < v <= bounds[-1]]
        if not inside:
            continue
        for rank in range(world):
            yield case, lengths, bounds, bs, world, rank, (0, rng.randint(1, 50))


def test_s2_bucket_sampler_random_cases():
    want = gold()["s2_sampler"]
    cases = list(_s2_sampler_cases())
    assert len(cases) == len(want)
    for (case, lengths, bounds, bs, world, rank, epochs), w in zip(cases, want):
        ours = D.S2BucketSampler(lengths, bs, list(bounds), num_replicas=world, rank=rank)
        for epoch, w_it in zip(epochs, w["iter"]):
            ours.set_epoch(epoch)
            assert list(iter(ours)) == w_it, (case, rank, epoch)
        assert len(ours) == w["len"] and ours.boundaries == w["boundaries"]


def _s1_sampler_cases():
    """(case, secs, bs, world, rank, drop, epochs)"""
    rng = random.Random(2)
    for case in range(40):
        n = rng.randint(1, 300)
        secs = [round(rng.uniform(0.2, 30.0), 2) for _ in range(n)]
        bs, world = rng.randint(1, 16), rng.randint(1, 4)
        drop = rng.random() < 0.3
        for rank in range(world):
            yield case, secs, bs, world, rank, drop, (0, rng.randint(1, 30))


def test_s1_bucket_sampler_random_cases():
    want = gold()["s1_sampler"]
    cases = list(_s1_sampler_cases())
    assert len(cases) == len(want)
    for (case, secs, bs, world, rank, drop, epochs), w in zip(cases, want):
        ours = D.S1BucketSampler(Stub(secs), bs, num_replicas=world, rank=rank, drop_last=drop, seed=case)
        for epoch, w_it in zip(epochs, w["iter"]):
            ours.set_epoch(epoch)
            assert list(iter(ours)) == w_it, (case, rank, epoch)
        assert len(ours) == w["len"]


def _s2_collate_cases():
    """[(ssl, spec, wav, text)] per case: the reference's item layout"""
    g = torch.Generator().manual_seed(3)
    rng = random.Random(3)
    for case in range(25):
        items_ref = []
        for _ in range(rng.randint(1, 7)):
            frames = rng.randint(33, 300)
            ssl_t = frames + rng.choice([0, 0, 1])
            ssl = torch.randn(1, 8, ssl_t, generator=g)
            spec = torch.rand(5, frames, generator=g)
            wav = torch.randn(1, frames * 640 + rng.randint(0, 639), generator=g)
            text = torch.randint(0, 700, (rng.randint(1, 40),), generator=g).float()
            items_ref.append((ssl, spec, wav, text))
        yield items_ref


def test_s2_collate_random_batches():
    want = gold()["s2_collate"]
    cases = list(_s2_collate_cases())
    assert len(cases) == len(want)
    for case, (items_ref, w) in enumerate(zip(cases, want)):
        items = [(ssl, wav, text, spec.size(1), True) for ssl, spec, wav, text in items_ref]
        ours, order = D.collate_s2(items, 5)
        for row, src in enumerate(order):
            ours[2][row, :, :items[src][3]] = items_ref[src][1]
        assert len(ours) == len(w)
        for a, b in zip(ours, w):
            assert digest(a) == b, case


def _s1_collate_cases():
    g = torch.Generator().manual_seed(4)
    rng = random.Random(4)
    for case in range(25):
        ex = []
        for i in range(rng.randint(1, 6)):
            n_ph, n_se = rng.randint(1, 50), rng.randint(1, 200)
            ex.append(dict(idx=i, phoneme_ids=[rng.randint(0, 700) for _ in range(n_ph)], phoneme_ids_len=n_ph,
                           semantic_ids=[rng.randint(0, 1023) for _ in range(n_se)], semantic_ids_len=n_se,
                           bert_feature=torch.randn(1024, n_ph, generator=g) if rng.random() < 0.7 else None))
        yield ex


S1_COLLATE_KEYS = ("phoneme_ids", "phoneme_ids_len", "semantic_ids", "semantic_ids_len", "bert_feature")


def test_s1_collate_random_batches():
    want = gold()["s1_collate"]
    ours = object.__new__(D.S1SemanticTable)
    ours.PAD = 1024
    cases = list(_s1_collate_cases())
    assert len(cases) == len(want)
    for case, (ex, w) in enumerate(zip(cases, want)):
        a = ours.collate(ex)
        assert a["ids"] == w["ids"]
        for k in S1_COLLATE_KEYS:
            assert digest(a[k]) == w[k], (case, k)


def _reject_y_cases():
    g = torch.Generator().manual_seed(5)
    for seed in range(60):
        B, T = int(torch.randint(1, 6, (1,), generator=g)), int(torch.randint(2, 90, (1,), generator=g))
        y = torch.randint(0, 1025, (B, T), generator=g)
        lens = torch.randint(1, T + 1, (B,), generator=g)
        yield seed, y, lens


def test_make_reject_y_random_seeds():
    want = gold()["reject_y"]
    cases = list(_reject_y_cases())
    assert len(cases) == len(want)
    for (seed, y, lens), (ry, rl, after_ref) in zip(cases, want):
        torch.manual_seed(seed)
        oy, ol = PU.make_reject_y(y, lens)
        after_ours = torch.randint(0, 10 ** 6, (1,)).item()       # the generator ends in the same state
        assert digest(oy) == ry and digest(ol) == rl and after_ref == after_ours, seed


def _sampling_cases():
    g = torch.Generator().manual_seed(6)
    rng = random.Random(6)
    for case in range(60):
        B, V = rng.randint(1, 4), rng.choice([1024, 1025, 300])
        logits = torch.randn(B, V, generator=g) * rng.choice([0.5, 3.0, 10.0])
        prev = torch.randint(0, V, (B, rng.randint(0, 80)), generator=g)
        kw = dict(temperature=rng.choice([1.0, 0.7, 1.4, 1e-7]), top_k=rng.choice([None, 1, 5, 15, 5000]),
                  top_p=rng.choice([None, 1, 0.95, 0.5, 0.05]), repetition_penalty=rng.choice([1.0, 1.35, 0.8]))
        yield logits, prev, kw


def test_sampling_restatement_random_logits():
    """the oracle's logits_to_probs (which the GPU sampling kernel is checked against) vs the reference's"""
    from oracle import s1_step as OS

    want_all = gold()["sampling"]
    cases = list(_sampling_cases())
    assert len(cases) == len(want_all)
    for case, ((logits, prev, kw), want) in enumerate(zip(cases, want_all)):
        got = OS.logits_to_probs(logits, prev, kw["temperature"], kw["top_k"], kw["top_p"], kw["repetition_penalty"])
        assert torch.equal(got > 0, want > 0) and torch.allclose(got, want, rtol=1e-6, atol=1e-9), (case, kw)


def _frame_count_cases():
    rng = random.Random(7)
    return [rng.randint(800, 90000) for _ in range(12)]


def test_frame_count_formula_random_lengths():
    want = gold()["frame_count"]
    cases = _frame_count_cases()
    assert len(cases) == len(want)
    for n, shape in zip(cases, want):
        assert shape == (1, 1025, D.spec_frames(n, 2048, 640)), n


def _dpo_cases():
    g = torch.Generator().manual_seed(8)
    return [(torch.randn(5, generator=g) * 30, torch.randn(5, generator=g) * 30) for _ in range(20)]


def test_dpo_loss_matches_reference_helper():
    want = gold()["dpo"]
    cases = _dpo_cases()
    assert len(cases) == len(want)
    for (a, r), w in zip(cases, want):
        assert torch.allclose(PU.dpo_loss(a, r, 0.2), w, rtol=1e-6, atol=1e-7)


def _commons_cases():
    g = torch.Generator().manual_seed(9)
    for case in range(20):
        B, T, Cn, seg = int(torch.randint(1, 6, (1,), generator=g)), int(torch.randint(40, 200, (1,), generator=g)), 7, 32
        x = torch.randn(B, Cn, T, generator=g)                        # reference layout [B, C, T]
        lens = torch.randint(seg, T + 1, (B,), generator=g)
        yield case, x, lens, T, seg


def test_commons_helpers_random():
    from easevoice_trainer_amd.module import commons as PC

    want = gold()["commons"]
    cases = list(_commons_cases())
    assert len(cases) == len(want)
    for (case, x, lens, T, seg), w in zip(cases, want):
        assert digest(PC.sequence_mask(lens, T)) == w["mask_T"]
        assert digest(PC.sequence_mask(lens)) == w["mask"]
        torch.manual_seed(case)
        got, ids = PC.rand_slice_segments(x.transpose(1, 2).contiguous(), lens, seg)     # ours is channels-last
        assert torch.equal(ids, w["ids"]) and digest(got.transpose(1, 2).contiguous()) == w["slices"]
        assert digest(PC.slice_segments(x.transpose(1, 2).contiguous(), ids, seg).transpose(1, 2).contiguous()) == w["slice"]


class LrOpt:
    def __init__(self):
        self.param_groups = [dict(lr=0.01), dict(lr=0.01)]


LR_ARGS = dict(init_lr=1e-5, peak_lr=1e-2, end_lr=1e-4, warmup_steps=20, total_steps=100)


def test_lr_schedule_trajectory():
    from easevoice_trainer_amd.auto_reg.optim import WarmupCosineLRSchedule as Ours

    want = gold()["lr_schedule"]
    b = LrOpt()
    rb = Ours(b, **LR_ARGS)
    assert len(want["steps"]) == 150
    for step, last, groups in want["steps"]:
        assert rb.step() == step and rb.get_last_lr() == last
        assert [g["lr"] for g in b.param_groups] == groups
    # the state a Lightning checkpoint keeps under "lr_schedulers": same keys and values, loadable either way (the
    # reference's load_state_dict is a plain update of its attributes by these keys)
    sa, sb = want["state_dict"], rb.state_dict()
    assert set(sa) == set(sb) and all(sa[k] == pytest.approx(sb[k]) for k in sa), (sa, sb)
    assert sb["_current_step"] == 150
    c = LrOpt()
    rc = Ours(c, init_lr=1.0, peak_lr=2.0, end_lr=3.0, warmup_steps=1, total_steps=2)
    rc.load_state_dict(sa)
    assert rc._current_step == 150 and rc.warmup_steps == 20 and rc.get_last_lr() == want["steps"][-1][1]


KMEANS_CASES = ((700, 64, 24, 50), (40, 64, 24, 50), (300, 16, 8, 7))


def _kmeans_cases():
    g = torch.Generator().manual_seed(10)
    for n, K, dim, iters in KMEANS_CASES:
        yield n, K, dim, iters, torch.randn(n, dim, generator=g) + 2.0 * torch.randint(0, 4, (n, 1), generator=g)


def test_kmeans_codebook_init_matches_reference():
    """a run without a pretrained generator: the codebook initialised from the first batch, same draws / same centres as
    the reference's EuclideanCodebook, for more and for fewer vectors than codes"""
    from easevoice_trainer_amd.module import models as PM

    want = gold()["kmeans"]
    cases = list(_kmeans_cases())
    assert len(cases) == len(want)
    for (n, K, dim, iters, data), w in zip(cases, want):
        ours = PM._Codebook(dim, K)
        ours.KMEANS_ITERS = iters
        torch.manual_seed(n)
        ours.init_embed_(data)
        after_ours = torch.randint(0, 10 ** 6, (1,)).item()
        assert w["after"] == after_ours
        assert torch.equal(ours.embed, w["embed"]) and torch.equal(ours.embed_avg, w["embed_avg"])
        assert torch.equal(ours.cluster_size, w["cluster_size"]) and float(ours.inited) == w["inited"] == 1.0
        # (the nearest-code look-up on the initialised codebook is the HIP select kernel: tests/test_frontend_gpu.py)


CKPT_HYPER = dict(lr=1e-4, low=4e-5, betas=(0.8, 0.99), eps=1e-9)


def ref_optim_g(net_g, lr, low, betas, eps):
    """the optimiser construction of src/train/sovits.py:285-313 (the trainer module itself needs tensorboard to import)"""
    te_p = list(map(id, net_g.enc_p.text_embedding.parameters()))
    et_p = list(map(id, net_g.enc_p.encoder_text.parameters()))
    mrte_p = list(map(id, net_g.enc_p.mrte.parameters()))
    base = filter(lambda p: id(p) not in te_p + et_p + mrte_p and p.requires_grad, net_g.parameters())
    return torch.optim.AdamW([{"params": base, "lr": lr}, {"params": net_g.enc_p.text_embedding.parameters(), "lr": low},
                              {"params": net_g.enc_p.encoder_text.parameters(), "lr": low},
                              {"params": net_g.enc_p.mrte.parameters(), "lr": low}], lr, betas=betas, eps=eps)


def stepped_generator(model_cls, hps):
    """the generator of the checkpoint test: filled with util_fill (seed 1), one step of the reference's AdamW set-up on
    seeded gradients (ssl_proj gets none, as in the reference), the lr bookkeeping ExponentialLR adds (sovits.py:368-376)"""
    from util_fill import fill_module

    h = CKPT_HYPER
    net = model_cls(1025, 32, n_speakers=300, **hps["model"])
    fill_module(net, 1)
    opt = ref_optim_g(net, h["lr"], h["low"], h["betas"], h["eps"])
    g = torch.Generator().manual_seed(0)
    for n, p in net.named_parameters():
        if not n.startswith("ssl_proj."):
            p.grad = torch.randn(p.shape, generator=g) * 1e-3
    opt.step()
    for grp in opt.param_groups:
        grp["initial_lr"] = grp["lr"]
    return net, opt


def checkpoint_content(path):
    return torch.load(path, map_location="cpu", weights_only=False)


def test_s2_checkpoints_resume_in_both_directions(tmp_path):
    """G_*.pth written by the reference's save_checkpoint resumes here, and ours resumes there: model tensors and every
    parameter's AdamW moments land on the same parameter (the optimiser state is numbered by position, and ssl_proj
    sits in the reference's first group without ever getting state).  The reference's file is rebuilt here from the same
    model and optimiser (its layout: model / iteration / optimizer / learning_rate) and must be identical, tensor for
    tensor, to the one its save_checkpoint wrote; the file written here must be identical to the one the reference
    loaded and resumed from when the fixture was made."""
    import json
    from easevoice_trainer_amd.module import models as PM
    from easevoice_trainer_amd.runtime import FlatAdamW, ParamArena
    from easevoice_trainer_amd.train.s2_engine import S2Engine
    from easevoice_trainer_amd.utils import ckpt as PCK

    want = gold()["checkpoint"]
    h = CKPT_HYPER
    lr, low = h["lr"], h["low"]
    hps = json.load(open(os.path.join(os.path.dirname(HERE), "configs", "s2.json")))
    ref, ropt = stepped_generator(PM.SynthesizerTrn, hps)
    p_ref = str(tmp_path / "G_ref.pth")
    torch.save({"model": ref.state_dict(), "iteration": 3, "optimizer": ropt.state_dict(), "learning_rate": lr}, p_ref)
    assert digest_hex(checkpoint_content(p_ref)) == want["ref_file"]
    ref_state = {n: ropt.state[p] for n, p in ref.named_parameters() if p in ropt.state}
    assert "ssl_proj.weight" not in ref_state and len(ref_state) == len(list(ref.parameters())) - 2

    # ---- reference -> ours ----
    ours = PM.SynthesizerTrn(1025, 32, n_speakers=300, **hps["model"])
    arena = ParamArena(ours, "cpu")
    opt = FlatAdamW(arena, S2Engine.g_param_groups(ours, lr, low), betas=h["betas"], eps=h["eps"])
    _, _, got_lr, it = PCK.load_checkpoint(p_ref, ours, opt)
    assert (got_lr, it) == (lr, 3) and opt.step_count == 1
    named = dict(ours.named_parameters())
    for n, p in ref.named_parameters():
        assert torch.equal(named[n].detach(), p.detach()), n
        b, e = arena.range_of(n, p.numel())
        if n in ref_state:
            assert torch.equal(opt.exp_avg[b:e].view(p.shape), ref_state[n]["exp_avg"]), n
            assert torch.equal(opt.exp_avg_sq[b:e].view(p.shape), ref_state[n]["exp_avg_sq"]), n
        else:
            assert not opt.exp_avg[b:e].any()
    assert [g_["lr"] for g_ in opt.param_groups] == [lr, low, low, low]

    # ---- ours -> reference ----
    p_ours = str(tmp_path / "G_ours.pth")
    PCK.save_checkpoint(ours, opt, lr, 4, p_ours)
    assert digest_hex(checkpoint_content(p_ours)) == want["ours_file"]
    # what the reference made of that file: (lr, iteration) from its load_checkpoint, and its checks of every parameter,
    # moment and group lr, and of a further optimiser step (tests/golden/make_golden_differential.py)
    assert want["ours_loaded_by_reference"] == dict(lr=lr, iteration=4, params_equal=True, moments_equal=True,
                                                    group_lrs=[lr, low, low, low], steps_after_resume=True)


def test_stdout_protocol_lines_equal_reference(capsys):
    """the `<prefix> <json>` lines a trainer process prints are what the reference's own connector prints (and parses)"""
    from easevoice_trainer_amd.utils import connector as PC

    ours = PC.MultiProcessOutputConnector()
    want = gold()["stdout_protocol"]
    ours.write_loss(7, 1.25, other={"loss/g/total": 1.25, "learning_rate": 1e-4})
    ours.write_loss(8, 0.5)
    ours.write_log({"epoch": 3, "msg": "x"})
    ours.write_response(PC.ResponseStatus.SUCCESS, "Training completed", {"model_path": "/p/m"})
    ours.write_response(PC.ResponseStatus.FAILED, "boom")
    got = capsys.readouterr().out
    assert got == want and want.count("\n") == 5


TRAIN_DIR_NAMES = ("voice1", "", None)


def _checkpoint_dir_cases():
    """[(case, file names)]"""
    rng = random.Random(11)
    for case in range(20):
        names = {f"G_{rng.randint(1, 99999)}.pth" for _ in range(rng.randint(1, 6))}
        if rng.random() < 0.4:
            names.add("G_latest.pth")
        names |= {f"D_{rng.randint(1, 99999)}.pth", "notes.txt"}
        yield case, sorted(names)


def test_directory_and_checkpoint_selection_equal_reference(tmp_path):
    from easevoice_trainer_amd.train import helper as PH
    from easevoice_trainer_amd.utils import ckpt as PCK

    want = gold()["directories"]
    for name, (w_sovits, w_gpt) in zip(TRAIN_DIR_NAMES, want["train_dirs"]):
        a = PH.get_sovits_train_dir("/proj", name)
        assert os.path.dirname(a) == os.path.dirname(w_sovits) and (a == w_sovits or not name)
        a = PH.get_gpt_train_dir("/proj", name)
        assert os.path.dirname(a) == os.path.dirname(w_gpt) and (a == w_gpt or not name)
    assert PH.train_logs_path == want["train_logs_path"]
    cases = list(_checkpoint_dir_cases())
    assert len(cases) == len(want["latest"])
    for (case, names), w in zip(cases, want["latest"]):
        d = tmp_path / f"c{case}"
        d.mkdir()
        for n in names:
            (d / n).write_bytes(b"x")
        assert os.path.relpath(PCK.latest_checkpoint_path(str(d), "G_*.pth"), str(d)) == w, names


def test_params_files_and_configs_equal_reference():
    """the `-c params.json` contract: same fields and defaults as the reference's dataclasses; same training configs"""
    import dataclasses
    import json
    import yaml
    from easevoice_trainer_amd.train.gpt import GPTTrainParams
    from easevoice_trainer_amd.train.sovits import SovitsTrainParams

    want = gold()["params_files"]
    for ours, cls in ((SovitsTrainParams, "SovitsTrainParams"), (GPTTrainParams, "GPTTrainParams")):
        got = [(f.name, f.default) for f in dataclasses.fields(ours)]
        # GPTTrainParams.model_path defaults to the reference's stock checkpoint path there; here "" resolves to the
        # same file through helper.default_pretrained (checked below)
        w = [(n, "" if d == ("name", "gpt_pretrained_model_path") else d) for n, d in want[cls]]
        assert got == w, (cls, got, w)
    repo = os.path.dirname(HERE)
    assert json.load(open(os.path.join(repo, "configs", "s2.json"))) == want["s2.json"]
    # stock pretrained fallbacks: same files as src/utils/config/__init__.py:34-35 and sovits.py:149-157
    from easevoice_trainer_amd.train import helper as PH
    assert os.path.join(want["normalize_root"], PH.PRETRAINED_FILES["s1"]) == want["gpt_pretrained_model_path"]
    assert os.path.join(want["normalize_root"], PH.PRETRAINED_FILES["s2G"]) == want["sovits_pretrained_model_path"]
    assert PH.PRETRAINED_FILES["s2D"] == PH.PRETRAINED_FILES["s2G"].replace("s2G", "s2D")
    assert yaml.safe_load(open(os.path.join(repo, "configs", "gpt.yaml"))) == want["gpt.yaml"]


def _scaled_adam_cases():
    """(case, shapes, init, period, clipping_scale, [per step: {name: gradient}])"""
    rng = random.Random(12)
    g = torch.Generator().manual_seed(12)
    for case in range(6):
        shapes = {}
        for i in range(rng.randint(3, 9)):
            kind = rng.choice(["mat", "mat", "vec", "scalar", "dup"])
            shapes[f"p{i}"] = {"mat": (rng.randint(2, 9), rng.randint(2, 17)), "vec": (rng.randint(2, 20),), "scalar": (1,),
                               "dup": (4, 6)}[kind]
        init = {k: torch.randn(v, generator=g) * (0.5 if len(v) > 1 else 0.2) for k, v in shapes.items()}
        period = rng.choice([3, 4, 7])
        cs = rng.choice([2.0, 1.2])
        grads = []
        for step in range(26):
            scale = 8.0 if rng.random() < 0.15 else 1.0           # spikes so that clipping engages
            grads.append({k: torch.randn(shapes[k], generator=g) * 0.1 * scale for k in shapes})
        yield case, shapes, init, period, cs, grads


def scaled_adam_lr(step):
    return 0.002 if step > 2 else 0.01                             # the scheduler pins the lr after its first steps


def test_scaled_adam_random_trajectories():
    """ScaledAdam host logic (batching by shape, scalar branch, size update every 4 steps, gradient clipping from the
    running median with different update periods, lr changes) against the reference's optimiser on random problems"""
    from cpu_emu import cpu_emulation_s1
    from easevoice_trainer_amd.auto_reg.optim import ScaledAdam
    from easevoice_trainer_amd.runtime import ParamArena

    want = gold()["scaled_adam"]
    cases = list(_scaled_adam_cases())
    assert len(cases) == len(want)
    for (case, shapes, init, period, cs, grads), w in zip(cases, want):
        class Holder(torch.nn.Module):
            def __init__(self):
                super().__init__()
                for k, v in init.items():
                    setattr(self, k, torch.nn.Parameter(v.clone()))

        with cpu_emulation_s1():
            h = Holder()
            arena = ParamArena(h, "cpu")
            opt = ScaledAdam(arena, lr=0.01, betas=(0.9, 0.95), clipping_scale=cs, clipping_update_period=period)
            params = dict(h.named_parameters())
            assert all(len(v) == len(grads) for v in w.values()) and set(w) == set(shapes)
            for step, gs in enumerate(grads):
                arena.zero_grad()
                for k in shapes:
                    params[k].grad.copy_(gs[k])
                opt.step()
                opt.param_groups[0]["lr"] = scaled_adam_lr(step)
                for k in shapes:
                    assert torch.allclose(params[k].detach(), w[k][step], rtol=1e-4, atol=3e-6), (case, step, k)


SA_SHAPES = {"emb.w": (7, 6), "a.alpha": (1,), "l0.w": (4, 6), "l0.b": (4,), "b.alpha": (1,), "l1.w": (4, 6), "l1.b": (4,),
             "out.w": (9, 4)}
SA_ORDER = list(SA_SHAPES)                                 # the reference's parameter order
SA_KW = dict(lr=0.01, betas=(0.9, 0.95), clipping_scale=2.0, clipping_update_period=5)


def sa_init():
    g = torch.Generator().manual_seed(3)
    return {k: torch.randn(v, generator=g) * (0.5 if len(v) > 1 else 0.2) for k, v in SA_SHAPES.items()}


def sa_grads(step):
    gg = torch.Generator().manual_seed(100 + step)
    return {k: torch.randn(SA_SHAPES[k], generator=gg) * (0.8 if step % 6 == 5 else 0.1) for k in SA_ORDER}


def sa_ours(values):
    """this repository's ScaledAdam on a module that registers its parameters in ANOTHER order than the reference"""
    from easevoice_trainer_amd.auto_reg.optim import ScaledAdam
    from easevoice_trainer_amd.runtime import ParamArena

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            for k in reversed(SA_ORDER):
                self.register_parameter(k.replace(".", "_"), torch.nn.Parameter(values[k].clone()))

    h = Holder()
    arena = ParamArena(h, "cpu")
    return h, arena, ScaledAdam(arena, **SA_KW)


SA_NAME_OF = {k: k.replace(".", "_") for k in SA_ORDER}


def test_scaled_adam_state_crosses_to_and_from_the_reference_optimizer():
    """src/train/gpt.py:172-177 resumes from a Lightning checkpoint whose "optimizer_states"[0] is the reference
    optimiser's own state_dict (stacked same-shape batches, state under the first parameter of a batch, clipping history in
    the first batch).  ScaledAdam.load_reference_state continues such a run -- same parameters as the reference optimiser
    continuing itself -- and reference_state_dict hands a run back: the reference optimiser loads it and continues like
    ours (the state handed back must be the one the reference loaded when the fixture was made)."""
    from cpu_emu import cpu_emulation_s1

    want = gold()["scaled_adam_cross"]
    with cpu_emulation_s1():
        # ---- reference runs 13 steps, we continue from its state_dict ----
        h, arena, opt = sa_ours(want["after_13"])
        opt.load_reference_state(copy.deepcopy(want["state_13"]), [SA_NAME_OF[k] for k in SA_ORDER])
        assert opt.step_count == 13
        params = dict(h.named_parameters())
        assert len(want["ref_13_25"]) == 12 and len(want["ref_25_36"]) == 11
        for step, ref_p in zip(range(13, 25), want["ref_13_25"]):
            gs = sa_grads(step)
            arena.zero_grad()
            for k in SA_ORDER:
                params[SA_NAME_OF[k]].grad.copy_(gs[k])
            opt.step()
            for k in SA_ORDER:
                assert torch.allclose(params[SA_NAME_OF[k]].detach(), ref_p[k], rtol=1e-4, atol=3e-6), (step, k)
        # ---- and back: our state in the reference's layout, loaded by a fresh reference optimiser ----
        back = opt.reference_state_dict([SA_NAME_OF[k] for k in SA_ORDER])
        assert digest_hex(back) == want["back"]
        assert digest_hex({k: params[SA_NAME_OF[k]].detach() for k in SA_ORDER}) == want["params_25"]
        for step, ref_p in zip(range(25, 36), want["ref_25_36"]):
            gs = sa_grads(step)
            arena.zero_grad()
            for k in SA_ORDER:
                params[SA_NAME_OF[k]].grad.copy_(gs[k])
            opt.step()
            for k in SA_ORDER:
                assert torch.allclose(params[SA_NAME_OF[k]].detach(), ref_p[k], rtol=1e-4, atol=3e-6), (step, k)


def s1_model_config():
    import yaml

    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(HERE), "configs", "gpt.yaml")))
    cfg["model"].update(n_layer=2)                       # two layers show the pattern
    return cfg


def test_s1_parameter_order_equals_reference():
    """the s1 resume file stores the optimiser state by parameter INDEX in named_parameters() order (the reference's
    configure_optimizers, t2s_lightning_module.py:94-108): names, order and shapes of our Text2SemanticDecoder equal the
    reference's, so an index means the same tensor on both sides"""
    from easevoice_trainer_amd.auto_reg.t2s_model import Text2SemanticDecoder as Ours

    want = gold()["s1_parameter_order"]
    ours = Ours(s1_model_config())
    assert [(n, tuple(p.shape)) for n, p in ours.named_parameters()] == want["named_parameters"]
    assert [k for k in ours.state_dict()] == want["state_dict_keys"]

"""hip/linear.LinearBank: the fold reads Np rows of a weight whose output width is padded (N = 1025 -> Np = 1152, the
vocabulary projection).  A parameter whose storage ends behind its own N rows -- a bare model outside an engine's
ParamArena -- must be folded from a zero-padded copy; one that has the room (the arena's reserve) is read in place."""
import pytest
import torch


def _bank(weight, device):
    from easevoice_trainer_amd.hip.linear import LinearBank

    bank = LinearBank([("proj", weight, None)], torch.float32, device)
    bank._tables()
    return bank, bank.slots[0]


def test_padded_width_gets_a_source_copy_only_without_room():
    N, K = 1025, 64
    bare = torch.nn.Parameter(torch.randn(N, K))
    _b, s = _bank(bare, "cpu")
    assert (s.N, s.Np) == (N, 1152) and s.pad is not None and s.pad.shape == (1152, K) and s.pad.dtype == torch.float32
    assert s.layout.d0 == 1152                      # the rows the fold walks
    room = torch.zeros(1152 * K + 7)
    inside = torch.nn.Parameter(room[:N * K].view(N, K))
    _b, s = _bank(inside, "cpu")
    assert s.pad is None
    short = torch.nn.Parameter(torch.zeros(1151 * K)[:N * K].view(N, K))
    _b, s = _bank(short, "cpu")
    assert s.pad is not None
    _b, s = _bank(torch.nn.Parameter(torch.randn(1024, K)), "cpu")
    assert s.Np == 1024 and s.pad is None


@pytest.mark.gpu
def test_bare_weight_is_folded_from_the_padded_copy(gpu):
    """the image of a bare [1025, K] weight equals the image of the same values inside zeroed storage of 1152 rows"""
    N, K = 1025, 512
    w = torch.randn(N, K, generator=torch.Generator().manual_seed(2))
    bare = torch.nn.Parameter(w.to(gpu))
    room = torch.zeros(1152, K, device=gpu)
    room[:N] = w.to(gpu)
    inside = torch.nn.Parameter(room[:N])
    (ba, sa), (bb, sb) = _bank(bare, gpu), _bank(inside, gpu)
    assert sa.pad is not None and sb.pad is None
    ba.prepare()
    bb.prepare()
    torch.cuda.synchronize()
    assert torch.equal(sa.pad[:N], bare.detach()) and not bool(sa.pad[N:].any())
    assert torch.equal(sa.reg, sb.reg) and torch.equal(sa.alt, sb.alt) and bool(sa.reg.any())
    with torch.no_grad():
        bare.mul_(2.0)                              # an in-place write bumps the version: prepare() refreshes the copy
    ba.prepare()
    torch.cuda.synchronize()
    assert torch.equal(sa.pad[:N], bare.detach()) and not torch.equal(sa.reg, sb.reg)

"""CPU: packed_layout (auto_reg/t2s_infer.py), the descriptors of the packed prompt pass, against a brute-force enumeration."""
import pytest

from easevoice_trainer_amd.auto_reg.t2s_infer import PACKED_QUERY_TILE, packed_layout

CASES = {
    "edges16": ([(1, 1), (15, 0), (16, 17), (17, 64)], [[0], [1], [2], [3]]),
    "edges64": ([(63, 1), (64, 65), (65, 130)], [[2], [0], [5]]),
    "candidates": ([(20, 100), (5, 7)], [[4, 1, 3], [0]]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_layout_against_enumeration(name):
    pack, slots = CASES[name]
    xl, yl = [a for a, _b in pack], [b for _a, b in pack]
    tok0, tiles, off, slot = packed_layout(xl, yl, slots)
    # rows follow each other without a gap
    assert tok0 == [sum(a + b for a, b in pack[:s]) for s in range(len(pack))]
    # every packed row belongs to exactly one tile, tiles start on multiples of the tile counted from the sequence's row 0 and
    # never reach into the next sequence
    owner = {}
    for s, q0 in zip(tiles[0::2], tiles[1::2]):
        assert q0 % PACKED_QUERY_TILE == 0 and 0 <= q0 < xl[s] + yl[s]
        for i in range(q0, min(q0 + PACKED_QUERY_TILE, xl[s] + yl[s])):
            assert (s, i) not in owner
            owner[s, i] = q0
    assert sorted(owner) == [(s, i) for s in range(len(pack)) for i in range(xl[s] + yl[s])]
    # the kernel's key bound of a tile (xl for a text tile, its last live query + 1 otherwise) covers what each of its
    # queries may see under the mask: a text query the text, an audio query the keys up to itself
    for (s, i), q0 in owner.items():
        last = min(q0 + PACKED_QUERY_TILE, xl[s] + yl[s]) - 1
        kend = xl[s] if last < xl[s] else last + 1
        assert (xl[s] if i < xl[s] else i + 1) <= kend <= xl[s] + yl[s]
    # the CSR map names every (sequence, slot) pair once
    pairs = [(s, d) for s in range(len(pack)) for d in slot[off[s]:off[s + 1]]]
    assert off[0] == 0 and off[-1] == len(slot) and pairs == [(s, d) for s, sl in enumerate(slots) for d in sl]
    assert len(set(pairs)) == len(pairs)

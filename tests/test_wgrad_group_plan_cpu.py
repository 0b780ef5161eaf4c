"""The split policy of the grouped weight-gradient launches (evt_wgrad_group_plan, include/evt.h): host arithmetic alone,
so it runs without a GPU.  The expectations are written from the rule the header states, not from the library:

  per launch of at most 16 members:  want = ceil(target / tiles of all its members)
  per member:                        split = clamp(want, 1, min(parts, stages // min_stages)),
                                     per = ceil(stages / split),  nsplit = ceil(stages / per)

and a group of one must be what the single launchers compute for a convolution alone (wgrad_pick_split in
csrc/conv_deep.hip, spelled out again below).
"""
import ctypes as C

import pytest

from easevoice_trainer_amd.hip import lib as L

RING_TARGET, RING_MIN = 256, 3       # launch_wgrad_ring: 256 blocks, at least 3 K stages per block


def ceil_div(a, b):
    return -(-a // b)


def pick_split(tiles, stages, target, min_stages, parts):
    """wgrad_pick_split of the single launchers"""
    split = ceil_div(target, tiles)
    split = min(split, stages // min_stages)
    if parts > 0:
        split = min(split, parts)
    split = max(split, 1)
    per = ceil_div(stages, split)
    return ceil_div(stages, per), per


def plan(members, target=RING_TARGET):
    """members: (tiles, stages, min_stages, parts) -> [(launch, nsplit, per)]"""
    arr = (L.WgradPlan * max(len(members), 1))()
    for r, (tiles, stages, min_stages, parts) in zip(arr, members):
        r.tiles, r.stages, r.min_stages, r.parts = tiles, stages, min_stages, parts
        r.launch = r.nsplit = r.per = -7
    assert L.lib().evt_wgrad_group_plan(arr, len(members), C.c_int64(target)) == 0
    return [(r.launch, r.nsplit, r.per) for r in arr[:len(members)]]


WN_IN = (36, 50, RING_MIN, 20)       # a WN in_layer of the s2 step: 36 tiles of wgrad_ring<64, 5x32>, 3200 positions, 20 slabs
TABLES = {
    "one": [WN_IN],
    "sixteen_equal": [WN_IN] * 16,
    "mixed_tiles": [(36, 50, RING_MIN, 20), (18, 50, RING_MIN, 20), (2, 10, RING_MIN, 20), (72, 257, RING_MIN, 7)],
    "parts_1": [(4, 50, RING_MIN, 1), (4, 50, RING_MIN, 20), (1, 50, RING_MIN, 1)],
    "short_reductions": [(2, 2, RING_MIN, 20), (2, 1, 8, 20), (36, 50, RING_MIN, 20)],       # stages < min_stages
    "no_slabs": [(4, 50, RING_MIN, 0), (4, 50, RING_MIN, 0)],                                  # parts 0: fp32 atomics, no bound
}


@pytest.mark.parametrize("name", sorted(TABLES))
def test_plan_follows_the_rule(name):
    members = TABLES[name]
    got = plan(members)
    want = ceil_div(RING_TARGET, sum(m[0] for m in members))
    for (tiles, stages, min_stages, parts), (launch, nsplit, per) in zip(members, got):
        assert launch == 0
        hi = stages // min_stages
        if parts > 0:
            hi = min(hi, parts)
        split = max(1, min(want, hi))
        assert per == ceil_div(stages, split) and nsplit == ceil_div(stages, per), (name, nsplit, per)
        assert 1 <= nsplit <= (parts if parts > 0 else stages), (name, nsplit, parts)
        # no split is empty: the last one starts inside the reduction, and together they cover it
        assert (nsplit - 1) * per < stages <= nsplit * per, (name, nsplit, per, stages)


def test_a_group_of_one_is_the_single_launch():
    for tiles in (1, 2, 3, 18, 36, 72, 255, 256, 257, 600):
        for stages in (1, 2, 3, 8, 10, 50, 51, 257, 640):
            for parts in (0, 1, 2, 7, 20, 128):
                for target, min_stages in ((256, 3), (512, 8), (1024, 8)):
                    got = plan([(tiles, stages, min_stages, parts)], target)
                    assert got == [(0,) + pick_split(tiles, stages, target, min_stages, parts)], \
                        (tiles, stages, parts, target, min_stages, got)


def test_the_wn_stack_needs_no_split():
    """16 in_layers are 576 tiles: the chip is full without a split, every block runs the 50 stages"""
    assert plan([WN_IN] * 16) == [(0, 1, 50)] * 16
    assert plan([WN_IN]) == [(0, 8, 7)]


@pytest.mark.parametrize("name", sorted(TABLES))
def test_plan_is_repeatable(name):
    assert plan(TABLES[name]) == plan(TABLES[name])


def test_seventeen_members_are_two_launches():
    members = [(36 if i % 2 else 18, 50 + i, RING_MIN, 20) for i in range(16)] + [(2, 50, RING_MIN, 20)]
    got = plan(members)
    assert [g[0] for g in got] == [0] * 16 + [1]
    # each launch's plan depends on its own members only
    assert got[:16] == plan(members[:16])
    assert got[16][1:] == plan(members[16:])[0][1:] == pick_split(2, 50, RING_TARGET, RING_MIN, 20)
    changed = plan(members[:16] + [(200, 50, RING_MIN, 20)])
    assert changed[:16] == got[:16]


def test_bad_arguments_are_refused():
    arr = (L.WgradPlan * 1)()
    arr[0].tiles, arr[0].stages, arr[0].min_stages, arr[0].parts = 0, 5, 3, 4
    assert L.lib().evt_wgrad_group_plan(arr, 1, C.c_int64(256)) != 0
    arr[0].tiles = 4
    assert L.lib().evt_wgrad_group_plan(arr, 1, C.c_int64(0)) != 0
    assert L.lib().evt_wgrad_group_plan(arr, 0, C.c_int64(256)) == 0

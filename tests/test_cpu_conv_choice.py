"""The host side of the convolution family -- argument checks, kernel and tile choice, column-sum layout, the batch rules -- is a pure
function of the argument block, and the query entry points run it without a device.  It must stay THE SAME function: for every block of
the sweep in `tests/conv_choice_sweep.py`, the same return code, the same choice, the same partial-row layout, single and batched.

`tests/golden/conv_choice.json` holds, per group of the sweep, the block count, the SHA-256 of the canonical record and the first two
records in full.  It was generated from commit cbf307e, the parent of the change that split `conv_impl` into conv_validate / conv_choose /
conv_launch and moved the tile facts into csrc/conv_tiles.h: that commit's unmodified library, loaded by path
(`python tests/conv_choice_sweep.py --lib <parent's libmtbt_hip.so> --fixture`), two separate processes, identical output.  The digests are
never regenerated from the code under test: a change that is meant to move a choice replaces the fixture from the old library's point of
view, by hand, with the reason.

That the sweep is dense enough was checked on scratch copies of the parent by moving one threshold of `pick_tile` at a time by about 10 %
(300, 512, 1024, 3000, 4096, the 256s of the k x k branch): every move that can change a choice at all changed at least one digest.

On a mismatch: `python tests/conv_choice_sweep.py <group>` prints the group's full record; diff it against the same command with
`--lib` pointing at the other build."""
import json

import pytest

import conv_choice_sweep as S

with open(S.FIXTURE) as f:
    GOLDEN = json.load(f)


@pytest.fixture(scope="module")
def lib():
    return S.load()


def test_fixture_holds_exactly_the_groups():
    assert sorted(GOLDEN) == sorted(S.ALL_GROUPS)
    assert 3000 <= sum(e["blocks"] for e in GOLDEN.values()) <= 9000
    # readable pins: a ragged 1x1 with a tile hint, the legal two-member batch of 3x3 head convs
    assert GOLDEN["hints"]["first"][1]["kc"] == [0, 0, 128, 128, 1] and GOLDEN["hints"]["first"][1]["layout"] == [[0, 2, 136], [0, 2, 272]]
    assert GOLDEN["batch_refusals"]["first"][0]["batch"] == [0, 0, 64, 64, 1]


@pytest.mark.parametrize("group", S.ALL_GROUPS)
def test_choices_are_the_parents_choices(lib, group):
    got = S.group_entry(lib, group)
    assert got["blocks"] == GOLDEN[group]["blocks"]
    assert got["first"] == GOLDEN[group]["first"]
    assert got["sha256"] == GOLDEN[group]["sha256"]

"""CPU: the lean walk form where the analysis kernel's registers decide it (speedy_amd/csrc/spx_mode.h spx_choose_mode), replayed
from profiles/kernel_resources.json like tests/test_mode_table.py.

Since the 16-frame 16 kHz analysis kernel takes 88 registers, two of its waves fit beside two walk waves of 128 registers.  16 kHz
batches with slow-down jobs keep the lean form they have had (the full form beside them is not measured); every other plan whose
numbers look the same -- 8 kHz: walk waves of 128 registers, analysis waves of 88 -- keeps the FULL form it has had, because the
rule is tied to the one kernel that was rebuilt (its default-tile instantiation takes fewer registers than its small-tile one)."""
from test_mode_table import kind, table  # noqa: F401  (the fixture and its helper)


def test_16k_slow_down_batches_keep_the_lean_form(table):
    for kw in (dict(), dict(ahead_req=1)):
        a = table("16000,1,256,0", **kw)
        assert a["launch_lean"] == 1 and a["tile_frames"] == 16, (kw, a)
    assert kind(table("16000,1,256,0")) == "concurrent"


def test_8k_calls_keep_the_full_form(table):
    for kw in (dict(), dict(ahead_req=1)):
        a = table("8000,1,256,1", **kw)
        assert a["launch_lean"] == 0 and a["lean_walk"] == 0 and a["tile_frames"] == 16, (kw, a)
    assert kind(table("8000,1,256,1")) == "concurrent"
    # ... and the lean form by preference only, for overlapped walk kernels, as before
    assert table("8000,1,256,1", ahead_req=1, overlap_req=1)["launch_lean"] == 1


def test_16k_speed_up_calls_are_unchanged(table):
    assert table("16000,1,256,1")["launch_lean"] == 0
    assert table("16000,1,256,1", ahead_req=1)["launch_lean"] == 0
    a = table("16000,1,256,1", ahead_req=1, overlap_req=1)
    assert (a["launch_lean"], a["walk2"], a["tile_frames"]) == (1, 1, 16)

"""The kernel instantiation a batch is served by is chosen in ONE place per kernel family (spx_analysis_select, spx_walk_select,
spx_walk_fast_select): the launch, the register query and the name all come from that pick.  For a table of batch shapes this
checks that the three agree -- the form that ran (spx_debug_last_walk_form), what spx_debug_walk_info reports and the template
values in spx_batch_kernel_names -- and that the names are the ones recorded below.

The expected names were printed by this file's `observe` (python tests/test_gpu_kernel_choice.py) with the library of the
commit before the selectors (bcd76a2) on an MI355X with 256 CUs, with one exception: the 11 025 Hz rows.  Their plan has more
than 64 coarse lags; the launcher of that commit instantiated the wide-coarse kernels (SPEC = 2) for them while its hand-built
name said SPEC = 0 -- the table has what was launched.  The two 16 kHz mono rows of 256 streams are also the keys of
profiles/pmc_traffic.json."""
import ctypes as C
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RATES = (11025, 16000, 22050, 32000, 48000)
CHANNELS = (1, 2)
SECONDS = 0.25


def shapes(cus):
    """(streams, speedup_only, lean); the last: more than two streams per CU (600 on a 256-CU part)"""
    many = 600 if cus == 256 else 2 * cus + 88
    return ((1, 1, 0), (256, 1, 0), (256, 1, 1), (256, 0, 0), (many, 1, 0))


# analysis kernel per rate; (rate, channels) -> the template values of spx_walk_fast_kernel for the five shapes, in the order of shapes()
ANALYSIS = {11025: "spx_analysis_kernel<16, 0>", 16000: "spx_analysis_kernel<16, 240>", 22050: "spx_analysis_kernel<16, 330>",
            32000: "spx_analysis_kernel<16, 480>", 48000: "spx_analysis_kernel<8, 720>"}
WALK = {
    (11025, 1): ("<4, 4, 0, 2, 0>", "<4, 4, 0, 2, 0>", "<4, 0, 0, 2, 0>", "<4, 4, 0, 2, 2>", "<4, 0, 0, 2, 0>"),
    (11025, 2): ("<4, 4, 0, 2, 1>", "<4, 4, 0, 2, 1>", "<4, 0, 0, 2, 1>", "<4, 4, 0, 2, 3>", "<4, 0, 0, 2, 1>"),
    (16000, 1): ("<4, 4, 16000, 1, 0>", "<4, 4, 16000, 1, 0>", "<4, 0, 16000, 0, 0>", "<4, 4, 0, 0, 2>", "<2, 0, 16000, 0, 0>"),
    (16000, 2): ("<4, 4, 16000, 1, 1>", "<4, 4, 16000, 1, 1>", "<4, 0, 16000, 0, 1>", "<4, 4, 0, 0, 3>", "<2, 0, 16000, 0, 1>"),
    (22050, 1): ("<4, 4, 22050, 1, 0>", "<4, 4, 22050, 1, 0>", "<4, 0, 22050, 0, 0>", "<4, 4, 0, 0, 2>", "<2, 0, 22050, 0, 0>"),
    (22050, 2): ("<4, 4, 22050, 1, 1>", "<4, 4, 22050, 1, 1>", "<4, 0, 22050, 0, 1>", "<4, 4, 0, 0, 3>", "<2, 0, 22050, 0, 1>"),
    (32000, 1): ("<8, 4, 0, 0, 0>", "<8, 4, 0, 0, 0>", "<8, 4, 0, 0, 0>", "<8, 4, 0, 0, 2>", "<8, 4, 0, 0, 0>"),
    (32000, 2): ("<8, 4, 0, 0, 1>", "<8, 4, 0, 0, 1>", "<8, 4, 0, 0, 1>", "<8, 4, 0, 0, 3>", "<8, 4, 0, 0, 1>"),
    (48000, 1): ("<8, 4, 0, 0, 0>", "<8, 4, 0, 0, 0>", "<8, 4, 0, 0, 0>", "<8, 4, 0, 0, 2>", "<8, 4, 0, 0, 0>"),
    (48000, 2): ("<8, 4, 0, 0, 1>", "<8, 4, 0, 0, 1>", "<8, 4, 0, 0, 1>", "<8, 4, 0, 0, 3>", "<8, 4, 0, 0, 1>"),
}


# ... and 16 * search waves + output waves of the walk kernel that RAN: the engine launches the lean form by itself where that
# lets the analysis run beside the walk -- only in a call whose kernels run concurrently (spx_debug_last_call_concurrent)
RAN = {
    (11025, 1): (64, 64, 64, 64, 64),
    (11025, 2): (68, 68, 68, 68, 64),
    (16000, 1): (68, 68, 68, 64, 32),
    (16000, 2): (68, 68, 68, 68, 32),
    (22050, 1): (64, 64, 64, 64, 32),
    (22050, 2): (68, 68, 68, 68, 32),
    (32000, 1): (132,) * 5, (32000, 2): (132,) * 5, (48000, 1): (132,) * 5, (48000, 2): (132,) * 5,
}


def expected(rate, ch):
    return [ANALYSIS[rate] + ";spx_tension_kernel;spx_walk_fast_kernel" + w for w in WALK[(rate, ch)]]


def form_of(names):
    """16 * search waves + output waves of the walk part of a names string (0: the general kernel), and its waves"""
    walk = names.split(";")[2]
    m = re.fullmatch(r"spx_walk_fast_kernel<(\d+), (\d+), \d+, \d+, \d+>", walk)
    if m:
        return 16 * int(m.group(1)) + int(m.group(2)), int(m.group(1)) + int(m.group(2))
    m = re.fullmatch(r"spx_walk_kernel<(\d+), \d+>", walk)
    assert m, walk
    return 0, int(m.group(1))


def observe(rate, ch):
    """Runs the shapes' batches; per shape (names, (form of the walk kernel that ran, forms of the names and the lean names,
    whether the call's kernels ran concurrently), spx_debug_walk_info's five values)."""
    import torch
    from speedy_amd.batch import Batch, Plan
    from speedy_amd.synth import speech_like
    plan = Plan(rate, False)
    L = plan.L
    n = int(rate * SECONDS)
    x = speech_like(n, rate, seed=41, channels=ch)
    ran = {}
    rows = []
    for streams, speedup_only, lean in shapes(torch.cuda.get_device_properties(0).multi_processor_count):
        if (streams, speedup_only) not in ran:   # the lean row asks about the batch the row before it ran
            speeds = np.full(streams, 3.5, np.float32)
            if not speedup_only:
                speeds[streams // 2] = 0.8
            b = Batch(plan, [n] * streams, ch, speeds, 1.0, 0.0)
            b.upload([x] * streams)
            b.run()   # raises unless the call succeeds
            torch.cuda.synchronize()
            assert int(b.d_nout.min()) > 0, "a stream overflowed or lost its producer"
            both = [f(plan.h, streams, ch, speedup_only).decode() for f in (L.spx_batch_kernel_names, L.spx_batch_kernel_names_lean)]
            ran[(streams, speedup_only)] = (L.spx_debug_last_walk_form(), [form_of(v)[0] for v in both], L.spx_debug_last_call_concurrent())
        names = (L.spx_batch_kernel_names_lean if lean else L.spx_batch_kernel_names)(plan.h, streams, ch, speedup_only).decode()
        info = (C.c_int * 5)()
        assert L.spx_debug_walk_info(rate, ch, streams, speedup_only, 0, lean, info) == 0
        rows.append((names, ran[(streams, speedup_only)], list(info)))
    return rows


@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("rate", RATES)
def test_launch_registers_and_name_come_from_one_choice(rate, ch):
    import torch
    rows = observe(rate, ch)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for i, ((streams, speedup_only, lean), (names, (ran, named, concurrent), info)) in enumerate(zip(shapes(cus), rows)):
        print(rate, ch, streams, speedup_only, lean, names, ran, named, concurrent, info)
        form, waves = form_of(names)
        assert info[3] == form and info[4] == waves, (names, info)
        assert form == named[lean] and RAN[(rate, ch)][i] in named
        # a call whose kernels ran in sequence (the device's lock is held elsewhere, SPX_SHARED_GPU) never launches the lean form
        assert ran == (RAN[(rate, ch)][i] if concurrent else named[0]), (streams, speedup_only, lean, names, ran, named, concurrent)
    assert [r[0] for r in rows] == expected(rate, ch)


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for rate_ in RATES:
        for ch_ in CHANNELS:
            for row in observe(rate_, ch_):
                print("ROW", rate_, ch_, repr(row[0]), row[1], row[2], flush=True)

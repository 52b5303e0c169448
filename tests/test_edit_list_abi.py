"""CPU-only: the C ABI of the edit list (spx_plan_edit_ops, spx_batch_run_edits, spx_edit_replay; spx_edit_op, spx_edit_track) and the
definition the device is held to (tests/edit_list_ref.py).

The definition is pinned on every directed job of tests/tsm_inputs.py -- linear_jobs(), nonlinear_jobs(), nonlinear_map_jobs(), the
event speeds of the nonlinear ones from the oracle's speed tap as tests/test_oracle_tsm_definition.py takes them:
replay(EditStream's list, the job's own input) is tests/tsm_ref.py's output AND the oracle's, sample for sample; the records are
contiguous from 0; every switch of edit_list_ref (one mistake each) breaks at least one input.  The jobs whose steps fail -- the ones
spx_plan_edit_ops does not promise to cover -- are listed with their true record counts; tests/test_gpu_edit_list.py gives them
explicit capacities and holds spx_plan_edit_ops to every other job (the plan needs a device)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_list_ref as E  # noqa: E402
import tsm_inputs as I  # noqa: E402
import tsm_ref as T  # noqa: E402

NEW = ["spx_plan_edit_ops", "spx_batch_run_edits", "spx_edit_replay"]

FAILED_STEP_JOBS = E.FAILED_STEP_JOBS


def test_the_abi_has_the_edit_list_and_keeps_its_layout(tmp_path):
    """The header declares the three functions and the two structs, the library exports the functions, the binding lists them;
    sizeof(spx_edit_op) == 16 and sizeof(spx_edit_track) == 24 under gcc -std=c99 -pedantic; the ABI version is still 1 and
    spx_stream_job still 48 bytes."""
    import speedy_amd
    from speedy_amd._lib import SYMBOLS, EditTrack
    hdr = open(os.path.join(ROOT, "include", "speedy_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared in include/speedy_hip.h"
        assert name in SYMBOLS, name + " is missing from speedy_amd._lib.SYMBOLS"
    assert re.search(r"typedef\s+struct\s*\{\s*int32_t\s+out_at\s*,\s*a\s*,\s*b\s*,\s*n\s*;\s*\}\s*spx_edit_op\s*;", code)
    assert re.search(r"typedef\s+struct\s*\{\s*int64_t\s+in_off\s*,\s*out_off\s*;\s*int32_t\s+channels\s*,\s*reserved\s*;\s*\}\s*spx_edit_track\s*;", code)
    assert ctypes.sizeof(EditTrack) == 24
    speedy_amd.build()
    raw = ctypes.CDLL(os.path.join(ROOT, "speedy_amd", "lib", "libspeedy_hip.so"))
    assert not [n for n in NEW if not hasattr(raw, n)]
    raw.spx_abi_version.restype = ctypes.c_int
    assert raw.spx_abi_version() == 1
    prog = tmp_path / "size.c"
    prog.write_text('#include <stdio.h>\n#include "speedy_hip.h"\n'
                    'int main(void) { printf("%u %u %u\\n", (unsigned)sizeof(spx_edit_op), (unsigned)sizeof(spx_edit_track),\n'
                    '                        (unsigned)sizeof(spx_stream_job)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(prog), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().split() == ["16", "24", "48"]


def test_the_c_example_builds():
    """tools/batch_edits_example.c builds with gcc -std=c99 -pedantic -Wall -Wextra -Werror (make editsexample)."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "speedy_amd", "csrc"), "editsexample"])
    assert os.path.exists(os.path.join(ROOT, "speedy_amd", "lib", "batch_edits_example"))


def test_batch_refuses_edits_together_with_rate_or_time_map():
    """Batch(edits=True) with rate= or time_map=True is a ValueError, raised before anything of the device is asked."""
    from speedy_amd.batch import Batch
    with pytest.raises(ValueError):
        Batch(None, [1000], 1, 2.0, edits=True, rate=1.25)
    with pytest.raises(ValueError):
        Batch(None, [1000], 1, 2.0, edits=True, time_map=True)


# ------------------------------------------------------------------ the definition, once ------------------------------------------------------------------

@pytest.fixture(scope="module")
def linear():
    """{name: (tsm_ref's stream, EditStream)} of every directed linear job; computed once, left unchanged."""
    out = {}
    with E.shared_pitch_searches():
        for name, rate, ch, x, speed in I.linear_jobs():
            out[name] = (T.linear_job(x, rate, ch, speed), E.linear_job(x, rate, ch, speed))
    return out


@pytest.fixture(scope="module")
def nonlinear(orc):
    """{name: (job, event speeds, tsm_ref's stream, EditStream, the oracle's output)} of every nonlinear job."""
    out = {}
    with E.shared_pitch_searches():
        for job in I.nonlinear_jobs() + I.nonlinear_map_jobs():
            name, rate, ch, x, speed, nl = job
            ref = orc.compress_sound(x, rate, ch, speed, nl, 0.0, False, chunk=1000, taps=True)
            speeds = T.event_speeds(x.size // ch, rate, ref["speed"], speed)
            out[name] = (job, speeds, T.nonlinear_job(x, rate, ch, speeds, speed), E.nonlinear_job(x, rate, ch, speeds, speed), ref["out"])
    return out


def _oracle_linear(orc, x, rate, ch, speed):
    """The oracle's time-scale stage (orc_sonicInt*) on one write of everything and the flush."""
    L = orc.lib()
    h = L.orc_sonicIntCreateStream(rate, ch)
    assert h
    L.orc_sonicIntSetSpeed(h, speed)
    x = np.ascontiguousarray(x, np.int16)
    assert L.orc_sonicIntWriteShortToStream(h, orc.sptr(x), x.size // ch) == 1
    assert L.orc_sonicIntFlushStream(h) == 1
    buf, got = np.zeros((1 << 16) * ch, np.int16), []
    while True:
        k = L.orc_sonicIntReadShortFromStream(h, orc.sptr(buf), 1 << 16)
        if k <= 0:
            break
        got.append(buf[:k * ch].copy())
    L.orc_sonicIntDestroyStream(h)
    return np.concatenate(got).astype(np.int64) if got else np.zeros(0, np.int64)


def _replayed(e, x, ch, switch=None):
    return E.replay(e.ops, x, ch, e.limit, e.out_n, switch)


def test_replaying_a_linear_jobs_list_on_its_own_input_gives_the_jobs_output(orc, linear):
    """... tsm_ref's, sample for sample, and the oracle's; the records are contiguous from 0; L = n_in."""
    assert len(linear) == len(I.linear_jobs()) > 250
    for name, rate, ch, x, speed in I.linear_jobs():
        s, e = linear[name]
        assert e.out_n == s.frames_out and e.limit == x.size // ch == E.limit_of(x.size // ch, rate, False), name
        assert E.contiguous(e.ops), name
        assert _replayed(e, x, ch) == s.out, name
        if not name.startswith("run"):
            assert np.array_equal(np.asarray(s.out, np.int64), _oracle_linear(orc, x, rate, ch, speed)), name


def test_replaying_a_nonlinear_jobs_list_on_its_own_input_gives_the_jobs_output(nonlinear):
    """... and there L = (n_in / B) B: the trailing partial ring buffer is never read."""
    assert len(nonlinear) == 15
    for name, (job, speeds, s, e, ref) in nonlinear.items():
        _, rate, ch, x, speed, nl = job
        n = x.size // ch
        assert e.out_n == s.frames_out and e.limit == E.limit_of(n, rate, True) == n // (rate // 100) * (rate // 100), name
        assert E.contiguous(e.ops), name
        got = _replayed(e, x, ch)
        assert got == s.out, name
        assert np.array_equal(np.asarray(got, np.int64), ref.astype(np.int64)), name


def test_the_lists_have_every_kind_of_record(linear, nonlinear):
    """Copies and cross-fades in one list, records of one frame (speed 200), one record for a whole unity job, a record that the
    flush's cut shortens, cross-fades with an operand behind L."""
    s, e = linear["lengths/22050Hz/1ch/679/1"]
    # (a unity job: the write's copy covers the whole output; the flush's copy of its 2 maxRequired zeros lies behind the cut, and stays)
    assert e.ops == [(0, 0, -1, 679), (679, 679, -1, 1356)] and e.out_n == 679
    s, e = linear["speeds/22050Hz/1ch/7000/200"]
    assert sum(1 for op in e.ops if op[3] == 1 and op[2] >= 0) >= 20
    s, e = linear["channels/22050Hz/2ch/6615/0.7"]
    assert sum(1 for op in e.ops if op[2] < 0) > 10 and sum(1 for op in e.ops if op[2] >= 0) > 10
    cut = sum(1 for _, e in linear.values() if e.ops and e.ops[-1][0] + e.ops[-1][3] > e.out_n)
    assert cut > 100
    behind = 0
    for job, speeds, s, e, ref in nonlinear.values():
        behind += sum(1 for op in e.ops if op[2] >= 0 and op[0] < e.out_n and max(op[1], op[2]) + op[3] > e.limit)
    assert behind >= 5


def test_the_jobs_with_failed_steps_and_their_true_counts(linear, nonlinear):
    """spx_plan_edit_ops covers a job none of whose steps fails; these are the directed jobs that have failed steps, with the number
    of records each really has.  No nonlinear job has one."""
    failed = {name: len(e.ops) for name, (s, e) in linear.items() if e.failed_steps}
    assert failed == FAILED_STEP_JOBS, failed
    for name, (s, e) in linear.items():
        assert e.failed_steps == s.census["failed_steps"], name
    assert not [name for name, v in nonlinear.items() if v[3].failed_steps]


def _caught(linear, nonlinear, switch):
    """The jobs on which the switch changes the records or the replayed output."""
    caught = []
    for name, rate, ch, x, speed in I.linear_jobs():
        if name.startswith("run") and not name.startswith("run/22050Hz/1ch/2981/"):
            continue          # (one length of the run is enough here)
        s, e = linear[name]
        m = E.linear_job(x, rate, ch, speed, switch)
        if m.ops != e.ops or m.limit != e.limit or _replayed(m, x, ch, switch) != s.out:
            caught.append(name)
    for name, (job, speeds, s, e, ref) in nonlinear.items():
        _, rate, ch, x, speed, nl = job
        m = E.nonlinear_job(x, rate, ch, speeds, speed, switch)
        if m.ops != e.ops or _replayed(m, x, ch, switch) != s.out:
            caught.append(name)
    return caught


@pytest.mark.parametrize("switch", E.SWITCHES)
def test_every_switch_breaks_a_job(linear, nonlinear, switch):
    """Teeth: each mistake changes the records or the replayed output of at least one directed job -- and limit_n_in, which only a
    nonlinear job can show, changes the OUTPUT of one (the records stay what they were)."""
    with E.shared_pitch_searches():
        caught = _caught(linear, nonlinear, switch)
    assert caught, switch
    if switch == "limit_n_in":
        assert all(n.startswith(("nonlinear", "map")) for n in caught), caught
    if switch == "floor":
        assert "channels/22050Hz/2ch/6615/2" in caught

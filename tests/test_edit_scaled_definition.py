"""CPU-only: the definition the device is held to for spx_edit_replay_scaled (tests/edit_scaled_ref.py), and the C ABI of the call
(spx_edit_scale, spx_edit_replay_scaled; spx_edit_master).

The definition is pinned on the directed jobs of tests/tsm_inputs.py that tests/test_edit_list_abi.py uses -- linear_jobs(),
nonlinear_jobs(), nonlinear_map_jobs(), the records those of tests/edit_list_ref.py: at p == q it is edit_list_ref.replay; the scaled
extents tile the output at every ratio; a copy-only list at an integer ratio r turns np.repeat(x, r) into np.repeat(out, r); the
float cross-fade is three roundings and a division, worked out by hand; every switch of edit_scaled_ref (one mistake each) breaks at
least one job.  The record-at-a-time form the GPU tests use (replay_scaled_np) is held to the definition value for value."""
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
import edit_scaled_ref as SC  # noqa: E402
import edit_scaled_util as U  # noqa: E402
import tsm_inputs as I  # noqa: E402
import tsm_ref as T  # noqa: E402

NEW = ["spx_edit_scale", "spx_edit_replay_scaled", "spx_debug_last_scaled_grid"]
_F = np.float32


def test_the_abi_has_the_scaled_replay_and_its_layout(tmp_path):
    """The header declares the functions, the struct and the two format constants, the library exports the functions, the binding
    lists them; sizeof(spx_edit_master) == 40 under gcc -std=c99 -pedantic, and the older structs are what they were."""
    import speedy_amd
    from speedy_amd._lib import SYMBOLS, EditMaster
    hdr = open(os.path.join(ROOT, "include", "speedy_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared in include/speedy_hip.h"
        assert name in SYMBOLS, name + " is missing from speedy_amd._lib.SYMBOLS"
    assert re.search(r"#define\s+SPX_SAMPLES_INT16\s+0\b", code) and re.search(r"#define\s+SPX_SAMPLES_FLOAT\s+1\b", code)
    assert re.search(r"typedef\s+struct\s*\{\s*int64_t\s+in_off\s*,\s*out_off\s*,\s*n_in\s*,\s*out_cap\s*;\s*int32_t\s+channels\s*,"
                     r"\s*reserved\s*;\s*\}\s*spx_edit_master\s*;", code)
    assert ctypes.sizeof(EditMaster) == 40
    assert "float tracks" in hdr, "the edit-list section's sentence on float tracks stays where it was"
    speedy_amd.build()
    raw = ctypes.CDLL(os.path.join(ROOT, "speedy_amd", "lib", "libspeedy_hip.so"))
    assert not [n for n in NEW if not hasattr(raw, n)]
    raw.spx_abi_version.restype = ctypes.c_int
    assert raw.spx_abi_version() == 1
    prog = tmp_path / "size.c"
    prog.write_text('#include <stdio.h>\n#include "speedy_hip.h"\n'
                    'int main(void) { printf("%u %u %u %u %d %d\\n", (unsigned)sizeof(spx_edit_master), (unsigned)sizeof(spx_edit_op),\n'
                    '                        (unsigned)sizeof(spx_edit_track), (unsigned)sizeof(spx_stream_job), SPX_SAMPLES_INT16,\n'
                    '                        SPX_SAMPLES_FLOAT); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(prog), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().split() == ["40", "16", "24", "48", "0", "1"]


def test_spx_edit_scale_is_S_and_refuses_what_the_definition_refuses():
    """The host function against edit_scaled_ref.scale: the five ratios and their unreduced forms, the edges of the rule, large x."""
    from speedy_amd import lib
    L = lib()
    xs = [0, 1, 2, 159, 160, 161, 9001, 2 ** 31 - 1, 2 ** 40 + 12345, 2 ** 62]
    ratios = list(SC.RATIOS) + [(48000, 16000), (44100, 16000), (882, 320), (32, 1), (33, 1), (32768, 1025), (32768, 1023), (32769, 32768),
                                (65536, 2), (1, 2), (0, 1), (1, 0), (-3, 1), (3, -1), (2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 1, 2 ** 26)]
    for p, q in ratios:
        for x in xs + [-1]:
            want = SC.scale(x, p, q)
            if want >= 2 ** 63:
                want = -1
            assert L.spx_edit_scale(x, p, q) == want, (x, p, q)
    assert SC.ratio(48000, 16000) == (3, 1) and SC.ratio(44100, 16000) == (441, 160) and SC.ratio(48000, 22050) == (320, 147)
    assert SC.ratio(33, 1) is None and SC.ratio(1, 2) is None and SC.ratio(32769, 32768) is None and SC.ratio(65536, 2) is None
    assert SC.ratio(65536, 2050) == (32768, 1025) and SC.ratio(32768, 1023) is None and SC.ratio(64, 2) == (32, 1)


def test_the_c_example_builds():
    """tools/batch_edit_scaled_example.c builds with gcc -std=c99 -pedantic -Wall -Wextra -Werror (make editscaledexample)."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "speedy_amd", "csrc"), "editscaledexample"])
    assert os.path.exists(os.path.join(ROOT, "speedy_amd", "lib", "batch_edit_scaled_example"))


# ------------------------------------------------------------------ the definition, once ------------------------------------------------------------------

@pytest.fixture(scope="module")
def linear():
    """{name: (job, EditStream)} of every directed linear job; computed once, left unchanged."""
    out = {}
    with E.shared_pitch_searches():
        for job in I.linear_jobs():
            name, rate, ch, x, speed = job
            out[name] = (job, E.linear_job(x, rate, ch, speed))
    return out


@pytest.fixture(scope="module")
def nonlinear(orc):
    """{name: (job, EditStream)} of every directed nonlinear job, the event speeds from the oracle's speed tap."""
    out = {}
    with E.shared_pitch_searches():
        for job in I.nonlinear_jobs() + I.nonlinear_map_jobs():
            name, rate, ch, x, speed, nl = job
            ref = orc.compress_sound(x, rate, ch, speed, nl, 0.0, False, chunk=1000, taps=True)
            out[name] = (job, E.nonlinear_job(x, rate, ch, T.event_speeds(x.size // ch, rate, ref["speed"], speed), speed))
    return out


def _all(linear, nonlinear):
    return list(linear.values()) + list(nonlinear.values())


def _few(linear, nonlinear):
    """A speed-up, a slow-down, two and three channels, a nonlinear job with L < n_in: the jobs the slower checks run on."""
    names = ["speeds/16000Hz/1ch/9001/3.5", "speeds/16000Hz/1ch/9001/0.7", "channels/22050Hz/2ch/6615/2", "rates/16000Hz/2ch/4800/1.3"]
    return [linear[n] for n in names] + [nonlinear["map/16000Hz/3ch/6000/2/1"], nonlinear["nonlinear/16000Hz/1ch/15000/3.5/1"]]


def test_at_one_to_one_the_definition_is_the_edit_lists_replay(linear, nonlinear):
    """p == q, int16: edit_list_ref.replay, value for value, on every directed job (and 2 / 2 is 1 / 1)."""
    assert len(linear) > 250 and len(nonlinear) == 15
    for job, e in _all(linear, nonlinear):
        x, ch = job[3], job[2]
        want = E.replay(e.ops, x, ch, e.limit, e.out_n)
        assert SC.replay_scaled(e.ops, x, ch, e.limit, e.out_n, 1, 1, x.size // ch) == want, job[0]
        assert SC.replay_scaled_np(e.ops, x, ch, e.limit, e.out_n, 1, 1, x.size // ch).tolist() == want, job[0]
    assert SC.ratio(2, 2) == (1, 1) and SC.ratio(44100, 44100) == (1, 1)


def test_the_scaled_extents_tile_the_output_at_every_ratio(linear, nonlinear):
    """n' >= 1 and S(out_at) + n' = S(next out_at), from 0 to at least N', for the five ratios on every list."""
    for p, q in SC.RATIOS:
        assert SC.ratio(p, q) == (p, q)
        for job, e in _all(linear, nonlinear):
            assert SC.tiles(e.ops, p, q, e.out_n), (job[0], p, q)
    # ... and below 1 / 1 they would not: a record of one frame gets none
    assert not SC.tiles([(0, 0, -1, 1), (1, 1, -1, 1), (2, 2, -1, 1)], 1, 2, 3)
    assert [op[3] for op in SC.scaled_ops([(0, 0, -1, 1), (1, 1, -1, 1)], 1, 2)] == [0, 1]


@pytest.mark.parametrize("fmt", ["int16", "float"])
@pytest.mark.parametrize("r", [2, 3])
def test_a_copy_only_list_repeats_what_it_copies(linear, r, fmt):
    """Speed 1 is one copy: at the integer ratio r the track np.repeat(x, r) -- every frame r times -- comes out as np.repeat(out, r)."""
    got_any = 0
    for name in ("lengths/22050Hz/1ch/679/1", "channels/22050Hz/2ch/6615/1"):
        if name not in linear:
            continue
        job, e = linear[name]
        _, rate, ch, x, speed = job
        assert speed == 1 and all(op[2] < 0 for op in e.ops)
        out = np.asarray(E.replay(e.ops, x, ch, e.limit, e.out_n), np.int64).reshape(-1, ch)
        y = np.repeat(x.reshape(-1, ch), r, axis=0).reshape(-1)
        want = np.repeat(out, r, axis=0).reshape(-1)
        if fmt == "float":
            y, want = (y / _F(32768)).astype(_F), (want / _F(32768)).astype(_F)
        got = SC.replay_scaled(e.ops, y, ch, e.limit, e.out_n, r, 1, y.size // ch, fmt)
        assert np.array_equal(U.as_bits(got, fmt), U.as_bits(want, fmt)), name
        got_any += 1
    assert got_any >= 1


def test_the_float_cross_fade_by_hand():
    """One record (0, 0, 1, 1) at 3 / 1: n' = 3, a' = 0, b' = 3.  The three values in np.float32, one operation at a time; the second
    is NOT the correctly rounded exact value (0.1 = 0x3dcccccd): the roundings in between show."""
    y = np.asarray([0.1, -0.3, 0.7, 0.25, 0.9, -0.55], _F)
    assert SC.scaled_ops([(0, 0, 1, 1)], 3, 1) == [(0, 0, 3, 3)]
    want = []
    for t in range(3):
        down = _F(y[t] * _F(3 - t))
        up = _F(y[3 + t] * _F(t))
        total = _F(down + up)
        want.append(_F(total / _F(3)))
    assert [hex(v) for v in SC.bits(want)] == ["0x3dcccccd", "0x3dcccccb", "0xbe088889"]
    got = SC.replay_scaled([(0, 0, 1, 1)], y, 1, 2, 1, 3, 1, 6, "float")
    assert [hex(v) for v in SC.bits(got)] == ["0x3dcccccd", "0x3dcccccb", "0xbe088889"]
    assert np.array_equal(SC.bits(SC.replay_scaled_np([(0, 0, 1, 1)], y, 1, 2, 1, 3, 1, 6, "float")), SC.bits(got))
    # a source frame at or behind L' reads as +0.0f: with L' = 4 the up-ramp has one frame
    got = SC.replay_scaled([(0, 0, 1, 1)], y, 1, 2, 1, 3, 1, 4, "float")
    assert [hex(v) for v in SC.bits(got)] == ["0x3dcccccd", hex(SC.bits([_F(_F(_F(y[1] * _F(2)) + _F(0)) / _F(3))])[0]),
                                              hex(SC.bits([_F(_F(y[2] * _F(1)) / _F(3))])[0])]
    # the sign of a zero survives a copy, and a cross-fade of two negative zeros is a negative zero
    z = np.asarray([-0.0, -0.0, 0.0, -0.0], _F)
    assert [hex(v) for v in SC.bits(SC.replay_scaled([(0, 0, -1, 2)], z, 1, 2, 2, 2, 1, 4, "float"))] == ["0x80000000", "0x80000000", "0x0", "0x80000000"]
    assert hex(SC.bits(SC.replay_scaled([(0, 0, 1, 1)], z, 1, 2, 1, 2, 1, 4, "float"))[1]) == "0x80000000"


@pytest.mark.parametrize("fmt", ["int16", "float"])
def test_the_record_at_a_time_form_is_the_definition(linear, nonlinear, fmt):
    """replay_scaled_np == replay_scaled, bit for bit, at the four ratios above 1 / 1, on tracks of 1 to 3 channels, one of them
    shorter than S(L)."""
    for k, (job, e) in enumerate(_few(linear, nonlinear)):
        p, q = SC.RATIOS[1 + k % 4]
        c = 1 + k % 3
        frames = SC.S(job[3].size // job[2], p, q) - (40 if k == 1 else 0)
        y = U.track(fmt, frames * c + (k % 2), 300 + k)
        a = SC.replay_scaled(e.ops, y, c, e.limit, e.out_n, p, q, frames, fmt)
        assert None not in a
        b = SC.replay_scaled_np(e.ops, y, c, e.limit, e.out_n, p, q, frames, fmt)
        assert np.array_equal(U.as_bits(a, fmt), U.as_bits(b, fmt)), (job[0], p, q, c)


@pytest.mark.parametrize("switch", SC.SWITCHES)
def test_every_switch_breaks_a_job(linear, nonlinear, switch):
    """Teeth: each mistake changes the replayed master of at least one directed job at 441 / 160 -- and at 3 / 1, where every floor is
    exact, neither of the two rounding mistakes shows."""
    caught, caught_int = [], []
    for k, (job, e) in enumerate(_few(linear, nonlinear)):
        for p, q, bucket in ((441, 160, caught), (3, 1, caught_int)):
            full = SC.S(job[3].size // job[2], p, q)
            n_in = full - 500 if switch == "limit_no_min" else full       # (the frames behind n_in are there, and far from zero)
            y = U.full_scale(full, 500 + k)
            if SC.replay_scaled(e.ops, y, 1, e.limit, e.out_n, p, q, n_in, "int16", switch) != SC.replay_scaled(e.ops, y, 1, e.limit, e.out_n, p, q, n_in):
                bucket.append(job[0])
    assert caught, switch
    if switch == "limit_no_min":
        assert caught_int
    else:
        assert not caught_int, (switch, caught_int)

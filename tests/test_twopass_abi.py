"""CPU-only: the C ABI of the two-pass batch call (spx_batch_run_twopass and its queries), its speed formula -- the text the retarget
kernel compiles, built for the host in libspx_mode_table.so -- against the numpy definition (tests/twopass_ref.py) bit for bit, the
C99 example, and what makes the call worth having: the oracle's own two passes land nearer the target than its probe pass."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import twopass_ref as tp  # noqa: E402
from util import read_wav  # noqa: E402

NEW = ["spx_batch_workspace_bytes_twopass", "spx_plan_out_capacity_twopass", "spx_batch_run_twopass", "spx_debug_last_twopass"]


def test_the_abi_has_the_twopass_calls_and_keeps_its_layout():
    """The header declares the four functions, the built library exports them, the Python binding lists them; the ABI version is
    still 1 (the targets travel beside the job table, not in it)."""
    import speedy_amd
    from speedy_amd._lib import SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "speedy_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared in include/speedy_hip.h"
        assert name in SYMBOLS, name + " is missing from speedy_amd._lib.SYMBOLS"
    speedy_amd.build()
    raw = ctypes.CDLL(os.path.join(ROOT, "speedy_amd", "lib", "libspeedy_hip.so"))
    assert not [n for n in NEW if not hasattr(raw, n)]
    src = "".join(open(os.path.join(ROOT, "speedy_amd", "csrc", f)).read()
                  for f in sorted(os.listdir(os.path.join(ROOT, "speedy_amd", "csrc"))) if f.endswith((".hip", ".cpp")))
    m = re.search(r"int\s+spx_abi_version\s*\(\s*(void)?\s*\)\s*\{\s*return\s+(\d+)\s*;", src)
    assert m and int(m.group(2)) == 1


def test_the_kernel_and_the_table_library_compile_one_formula():
    """spx_twopass.h is the one place the formula is written: the device code and the host-only library include it, neither
    restates it."""
    csrc = os.path.join(ROOT, "speedy_amd", "csrc")
    assert '#include "spx_twopass.h"' in open(os.path.join(csrc, "spx_twopass.hip")).read()
    assert '#include "spx_twopass.h"' in open(os.path.join(csrc, "spx_mode_table.cpp")).read()
    assert "#include <hip" not in open(os.path.join(csrc, "spx_twopass.h")).read()
    # the object with the retarget kernel is the last one linked: the hot object's placement stays what it was
    mk = open(os.path.join(csrc, "Makefile")).read()
    src = re.search(r"^SRC \?= (.*)$", mk, flags=re.M).group(1).split()
    assert src[-1] == "spx_twopass.hip" and src[0] == "spx_hot.hip"


@pytest.fixture(scope="module")
def table():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "speedy_amd", "csrc"), "modetable"])
    L = ctypes.CDLL(os.path.join(ROOT, "speedy_amd", "lib", "libspx_mode_table.so"))
    L.spx_mode_table_twopass_speed.restype = ctypes.c_float
    L.spx_mode_table_twopass_speed.argtypes = [ctypes.c_double, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong]
    return L


def _same(table, want, mode, T, n_probe):
    got = np.float32(table.spx_mode_table_twopass_speed(float(want), int(mode), int(T), int(n_probe)))
    ref = tp.second_speed(want, mode, T, n_probe)
    assert tp.bits(got) == tp.bits(ref), (want, mode, T, n_probe, got, ref)


def test_formula_equals_the_numpy_definition_bit_for_bit(table):
    rng = np.random.default_rng(20)
    for _ in range(4000):
        want = float(np.exp(rng.uniform(np.log(0.01), np.log(50.0))))
        T = int(rng.integers(1, 1 << int(rng.integers(1, 31))))
        # counts around T / want, as a probe gives them, and anything else now and then
        n_probe = max(1, int(T / want * rng.uniform(0.5, 2.0))) if rng.random() < 0.8 else int(rng.integers(1, 1 << 40))
        for mode in (0, 1):
            _same(table, want, mode, T, n_probe)
    # want as the call computes it in length mode, with the counts of a probe
    for T in (241, 6000, 16000, 50381, (1 << 30) - 1):
        for rate in (16000, 22050, 44100):
            for sec in (0.1, 1.5, 7.0, 1e-3):
                want = tp.want_of(T, rate, sec, 1.0)
                for n_probe in (int(T / want), int(T / want) + 1, int(T / want * 1.07)):
                    _same(table, want, 1, T, n_probe)
                    _same(table, want, 0, T, n_probe)


def test_formula_edges(table):
    """Nothing to measure (a count of 0 or below: empty, too short, overflow, lost producer) answers (float)want in both modes; a
    count of 1; an empty input (never seen with a positive count by the call itself: defined all the same)."""
    lost = -(1 << 63)
    for want in (0.8, 1.0, 3.5, 1e-3, 123.456, float(np.float32(2.2))):
        for mode in (0, 1):
            for T in (0, 1, 100, 241, 16000):
                for n_probe in (0, -1, -17, lost):
                    _same(table, want, mode, T, n_probe)
                    assert tp.bits(tp.second_speed(want, mode, T, n_probe)) == tp.bits(np.float32(want))
                for n_probe in (1, 2, T, T + 1):
                    if n_probe > 0:
                        _same(table, want, mode, T, n_probe)
    assert tp.second_speed(2.0, 0, 1000, 1) == np.float32(1000.0)
    assert tp.second_speed(2.0, 1, 1000, 500) == np.float32(2.0)
    assert tp.second_speed(2.0, 0, 0, 5) == np.float32(0.0) and np.isinf(tp.second_speed(2.0, 1, 0, 5))


def test_c_example_builds():
    """tools/batch_twopass_example.c builds with gcc -std=c99 -pedantic -Werror over include/speedy_hip.h alone."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "speedy_amd", "csrc"), "twopassexample"])
    assert os.path.exists(os.path.join(ROOT, "speedy_amd", "lib", "batch_twopass_example"))


@pytest.mark.parametrize("seg", tp.SEGMENTS, ids=lambda s: "whole" if s[0] is None else "%d-%d" % s)
@pytest.mark.parametrize("factor", tp.FACTORS)
def test_the_oracles_second_pass_lands_nearer_the_target(orc, seg, factor):
    """The reference's --length driver on the oracle (compress_sound twice, as tests/test_gpu_cli.py does): the final pass's length
    is nearer the requested one than the probe pass's -- the property the batch call exists for.  Feedback 0."""
    x, rate, ch = read_wav("tapestry.wav")
    x = tp.segment(x, seg)
    T = x.size // ch
    seconds = T / rate / factor
    want = float(tp.want_of(T, rate, seconds, 1.0))
    probe = orc.compress_sound(x, rate, ch, want, 1.0, 0.0, False, chunk=1000)["out"].size // ch
    speed = float(tp.second_speed(want, 1, T, probe))
    final = orc.compress_sound(x, rate, ch, speed, 1.0, 0.0, False, chunk=1000)["out"].size // ch
    target = seconds * rate
    print("T %d target %.1f probe %d final %d" % (T, target, probe, final))
    assert abs(final - target) < abs(probe - target)


def test_a_twopass_batch_has_no_cpu_path():
    """Without a GPU a two-pass batch refuses to exist, as Plan does."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from speedy_amd.batch import TwoPassBatch
    with pytest.raises(RuntimeError):
        TwoPassBatch(None, [16000], 1, 3.5, seconds=1.0)

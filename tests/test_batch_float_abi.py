"""CPU-only: the C ABI of the batch call on float samples (spx_batch_run_float) and what makes its expected output well defined --
the oracle FLOAT stream equals the oracle SHORT stream on a numpy definition of the input conversion, divided by 32767."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["spx_batch_workspace_bytes_float", "spx_batch_run_float", "spx_float_to_short", "spx_short_to_float"]


def float_to_short_def(x, nonlinear):
    """The input conversion of a float batch job, defined in numpy: the product in float64 (nonlinear != 0: x * 32768.0) or in
    float32 (x * 32767.0f), truncated toward zero to an integer of which the low 16 bits are kept; a product that is NaN or of
    magnitude >= 2^31 gives 0."""
    x = np.ascontiguousarray(x, np.float32)
    with np.errstate(all="ignore"):
        if nonlinear:
            p = x.astype(np.float64) * np.float64(32768.0)
        else:
            p = (x * np.float32(32767.0)).astype(np.float64)   # (float32 x float32: one rounding, to float32)
        ok = np.abs(p) < 2.0 ** 31   # (False for NaN)
        t = np.trunc(np.where(ok, p, 0.0)).astype(np.int64)
    return (t & 0xffff).astype(np.uint16).view(np.int16)


def _oracle_stream(orc, x, rate_hz, ch, speed, nl, rate, mm, feedback, chunk, as_float):
    L = orc.lib()
    h = L.orc_sonicCreateStream(int(rate_hz), int(ch), int(bool(mm)))
    assert h
    L.orc_sonicSetSpeed(h, float(speed))
    if rate is not None:
        L.orc_sonicSetRate(h, float(rate))
    L.orc_sonicEnableNonlinearSpeedup(h, float(nl))
    L.orc_sonicSetDurationFeedbackStrength(h, float(feedback))
    cap = 1 << 16
    dt = np.float32 if as_float else np.int16
    write, read, ptr = ((L.orc_sonicWriteFloatToStream, L.orc_sonicReadFloatFromStream, orc.fptr) if as_float else
                        (L.orc_sonicWriteShortToStream, L.orc_sonicReadShortFromStream, orc.sptr))
    buf = np.zeros(cap * ch, dt)
    got = []

    def drain():
        while True:
            k = read(h, ptr(buf), cap)
            if k <= 0:
                return
            got.append(buf[:k * ch].copy())

    n = x.size // ch
    for pos in range(0, n, chunk):
        seg = np.ascontiguousarray(x[pos * ch:(pos + chunk) * ch])
        assert write(h, ptr(seg), seg.size // ch) == 1
        drain()
    assert L.orc_sonicFlushStream(h) == 1
    drain()
    L.orc_sonicDestroyStream(h)
    return np.concatenate(got) if got else np.zeros(0, dt)


def oracle_float_stream(orc, x, rate_hz, ch, speed, nl, rate=None, mm=False, feedback=0.0, chunk=1000):
    """The expected output of a float batch job: the oracle stream fed with FLOATS -- create, set speed / rate / nonlinear /
    feedback, orc_sonicWriteFloatToStream in chunks of `chunk` frames each followed by orc_sonicReadFloatFromStream until 0, flush,
    reads until 0.  rate None: sonicSetRate is not called."""
    return _oracle_stream(orc, np.ascontiguousarray(x, np.float32), rate_hz, ch, speed, nl, rate, mm, feedback, chunk, True)


def oracle_short_stream(orc, x, rate_hz, ch, speed, nl, rate=None, mm=False, feedback=0.0, chunk=1000):
    return _oracle_stream(orc, np.ascontiguousarray(x, np.int16), rate_hz, ch, speed, nl, rate, mm, feedback, chunk, False)


def test_the_abi_has_the_float_calls_and_keeps_its_layout(tmp_path):
    """The header declares the four functions, the built library exports them, the Python binding lists them; the ABI version is
    still 1 and spx_stream_job is still 48 bytes (a float job is the same record: only the unit of its offsets' buffers differs)."""
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
    prog = tmp_path / "size.c"
    prog.write_text('#include <stdio.h>\n#include "speedy_hip.h"\n'
                    'int main(void) { printf("%u\\n", (unsigned)sizeof(spx_stream_job)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(prog), "-o", str(exe)])
    assert int(subprocess.check_output([str(exe)]).decode()) == 48


def test_c_float_example_builds():
    """make floatexample: tools/batch_float_example.c under -std=c99 -pedantic -Werror, no HIP headers."""
    mk = open(os.path.join(ROOT, "speedy_amd", "csrc", "Makefile")).read()
    rule = re.search(r"^floatexample:.*\n((?:\t.*\n)+)", mk, flags=re.M)
    assert rule and all(f in rule.group(1) for f in ("-std=c99", "-pedantic", "-Werror", "batch_float_example.c"))
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "speedy_amd", "csrc"), "floatexample"])
    assert os.path.exists(os.path.join(ROOT, "speedy_amd", "lib", "batch_float_example"))


def test_the_definition_on_special_values():
    """float_to_short_def against hand-worked values: full scale wraps on the 32768 scale, not on the 32767 one; truncation is
    toward zero; NaN, infinities and products from 2^31 up give 0; 65536 keeps its low 16 bits (0)."""
    f = np.float32
    x = np.asarray([0.0, -0.0, 1.0, -1.0, 0.99999994, -0.99999994, 1.5, -1.5, 65536.0, -65536.0, 1e10, -1e10,
                    np.inf, -np.inf, np.nan, 1e-45, 0.5 / 32768, -0.5 / 32768, 2.5 / 32768, -2.5 / 32768], f)
    nl = float_to_short_def(x, True)
    assert list(nl) == [0, 0, -32768, -32768, 32767, -32767, -16384, 16384, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, -2]
    lin = float_to_short_def(x, False)
    #                                      0.99999994f * 32767.0f = 32766.998 -> 32766;  1.5 -> 49150.5 -> 49150 - 65536
    assert list(lin[:8]) == [0, 0, 32767, -32767, 32766, -32766, 49150 - 65536, 65536 - 49150]
    assert list(lin[8:16]) == [0, 0, 0, 0, 0, 0, 0, 0]   # 65536 * 32767 = 0x7fff0000: low 16 bits 0
    assert float_to_short_def(f([65537.0 / 32768]), True)[0] == 1 and float_to_short_def(f([40000.0 / 32768]), True)[0] == 40000 - 65536


CASES = [   # the (rate_hz, ch, speed, nl, rate) rows of tests/test_batch_rate_abi.py, plus two with rate 1
    (16000, 1, 3.5, 1.0, 1.25),
    (16000, 2, 2.0, 0.0, 0.5),
    (22050, 1, 1.5, 0.6, 2.0),
    (22050, 2, 0.7, 0.0, 0.8),
    (44100, 1, 3.5, 1.0, 0.8),
    (44100, 2, 1.0, 0.0, 1.25),
    (16000, 1, 0.7, 1.0, 2.0),
    (16000, 1, 3.5, 1.0, 1.0),
    (22050, 2, 2.0, 0.0, 1.0),
]


@pytest.mark.parametrize("rate_hz,ch,speed,nl,rate", CASES)
def test_oracle_float_stream_is_the_short_stream_on_the_defined_conversion(orc, rate_hz, ch, speed, nl, rate):
    """On float32 inputs in (-0.999, 0.999) the oracle float stream (writes of 1000 frames, reads until 0, flush, reads) equals
    bit for bit the oracle short stream on float_to_short_def(x), divided by float32 32767: inside the short range the definition
    IS the reference's cast, both input scales included, so "the oracle float stream" is a well-defined expected output."""
    from speedy_amd.synth import speech_like
    n = 5 * rate_hz
    s = np.stack([speech_like(n, rate_hz, seed=61 + c) for c in range(ch)], axis=1).reshape(-1)
    rng = np.random.default_rng(rate_hz + ch)
    x = (s.astype(np.float32) / np.float32(32768.0) * np.float32(0.97)).astype(np.float32)
    x[::7] = rng.uniform(-0.999, 0.999, x[::7].size).astype(np.float32)   # ... and values no short is the image of, up to the edge
    assert x.dtype == np.float32 and float(np.abs(x).max()) < 0.999
    got = oracle_float_stream(orc, x, rate_hz, ch, speed, nl, rate)
    q = float_to_short_def(x, nl != 0.0)
    assert np.array_equal(q, (x.astype(np.float64) * 32768.0).astype(np.int16) if nl != 0.0
                          else (x * np.float32(32767.0)).astype(np.int16))   # inside the range: the plain cast
    ref = oracle_short_stream(orc, q, rate_hz, ch, speed, nl, rate)
    want = ref.astype(np.float32) / np.float32(32767)
    assert ref.size > 0 and got.size == want.size
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_float_batch_has_no_cpu_path():
    """Without a GPU a float batch refuses to exist, as Plan does."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from speedy_amd.batch import FloatBatch, Plan, compress_batch_float
    with pytest.raises(RuntimeError):
        Plan(16000)
    with pytest.raises(RuntimeError):
        FloatBatch(None, [16000], 1, 3.5)
    with pytest.raises(RuntimeError):
        compress_batch_float([np.zeros(16000, np.float32)], 16000, 1, 3.5)

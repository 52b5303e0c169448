"""CPU-only: the C ABI of the batch call with a playback rate per stream (spx_batch_run_rate) and what makes its expected
output well defined -- the oracle stream with a rate set before the first write does not depend on how the input is chunked."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["spx_batch_run_rate", "spx_batch_workspace_bytes_rate", "spx_plan_out_capacity_rate"]


def oracle_rate_stream(orc, x, rate_hz, ch, speed, nl, rate, mm=False, feedback=0.0, chunk=1000):
    """The expected output of a batch job with a rate: the oracle STREAM -- create, set speed / rate / nonlinear / feedback,
    writes of `chunk` frames each followed by reads until 0, flush, reads until 0."""
    L = orc.lib()
    x = np.ascontiguousarray(x, np.int16)
    h = L.orc_sonicCreateStream(int(rate_hz), int(ch), int(bool(mm)))
    assert h
    L.orc_sonicSetSpeed(h, float(speed))
    L.orc_sonicSetRate(h, float(rate))
    L.orc_sonicEnableNonlinearSpeedup(h, float(nl))
    L.orc_sonicSetDurationFeedbackStrength(h, float(feedback))
    cap = 1 << 16
    buf = np.zeros(cap * ch, np.int16)
    got = []

    def drain():
        while True:
            k = L.orc_sonicReadShortFromStream(h, orc.sptr(buf), cap)
            if k <= 0:
                return
            got.append(buf[:k * ch].copy())

    n = x.size // ch
    for pos in range(0, n, chunk):
        seg = np.ascontiguousarray(x[pos * ch:(pos + chunk) * ch])
        assert L.orc_sonicWriteShortToStream(h, orc.sptr(seg), seg.size // ch) == 1
        drain()
    assert L.orc_sonicFlushStream(h) == 1
    drain()
    L.orc_sonicDestroyStream(h)
    return np.concatenate(got) if got else np.zeros(0, np.int16)


def test_the_abi_has_the_rate_call_and_keeps_its_layout(tmp_path):
    """The header declares the three functions, the built library exports them, the Python binding lists them; the ABI version
    is still 1 and spx_stream_job is still 48 bytes (the rates travel beside the job table, not in it)."""
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


def test_c_rate_example_builds():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "speedy_amd", "csrc"), "rateexample"])
    assert os.path.exists(os.path.join(ROOT, "speedy_amd", "lib", "batch_rate_example"))


@pytest.mark.parametrize("rate_hz,ch,speed,nl,rate", [
    (16000, 1, 3.5, 1.0, 1.25),
    (16000, 2, 2.0, 0.0, 0.5),
    (22050, 1, 1.5, 0.6, 2.0),
    (22050, 2, 0.7, 0.0, 0.8),
    (44100, 1, 3.5, 1.0, 0.8),
    (44100, 2, 1.0, 0.0, 1.25),
    (16000, 1, 0.7, 1.0, 2.0),
])
def test_oracle_rate_stream_does_not_depend_on_the_chunking(orc, rate_hz, ch, speed, nl, rate):
    """With the rate set before the first write the oracle stream gives the same bytes for writes of 160, 777, 1000 frames and
    one single write: "the oracle stream, written in chunks of 1000" is a well-defined expected output for a batch job."""
    from speedy_amd.synth import speech_like
    n = 5 * rate_hz
    x = np.stack([speech_like(n, rate_hz, seed=31 + c) for c in range(ch)], axis=1).reshape(-1)
    ref = oracle_rate_stream(orc, x, rate_hz, ch, speed, nl, rate, chunk=1000)
    assert ref.size > 0
    for chunk in (160, 777, n):
        got = oracle_rate_stream(orc, x, rate_hz, ch, speed, nl, rate, chunk=chunk)
        assert got.size == ref.size and np.array_equal(got, ref), "chunk %d" % chunk


def test_batch_with_rates_has_no_cpu_path():
    """Without a GPU a batch with rates refuses to exist, as Plan does."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from speedy_amd.batch import Batch, Plan, compress_batch
    with pytest.raises(RuntimeError):
        Plan(16000)
    with pytest.raises(RuntimeError):
        Batch(None, [16000], 1, 3.5, rate=1.25)
    with pytest.raises(RuntimeError):
        compress_batch([np.zeros(16000, np.int16)], 16000, 1, 3.5, rate=1.25)

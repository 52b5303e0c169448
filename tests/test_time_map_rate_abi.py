"""CPU-only: the C ABI of the time map on the rate and float batch calls (spx_batch_run_rate_map, spx_batch_run_float_map) and what
makes its expected rows well defined: the oracle stream with sonicSetRate set, observed at every hand-off, shows exactly
F(its rows at rate 1) -- tests/time_map_rate_ref.py, written from the header's text -- whatever the chunking; and the exact
definition of the rate stage as a stream (tests/tsm_ref.py RateStream) gives the same rows."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time_map_rate_ref as tr  # noqa: E402
import time_map_ref as tm  # noqa: E402

NEW = ["spx_batch_run_rate_map", "spx_batch_run_float_map"]
IDS = ["%d-%dch-%gx-nl%g-%d-fb%g" % s for s in tr.SHAPES]


def test_the_abi_has_the_rate_map_calls_and_keeps_its_layout(tmp_path):
    """The header declares both functions, the built library exports them, the Python binding lists them; the ABI version is still
    1 and spx_stream_job is still 48 bytes."""
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


def test_c_rate_map_example_builds():
    """make ratemapexample: tools/batch_rate_map_example.c under -std=c99 -pedantic -Wall -Wextra -Werror, no HIP headers."""
    mk = open(os.path.join(ROOT, "speedy_amd", "csrc", "Makefile")).read()
    rule = re.search(r"^ratemapexample:.*\n((?:\t.*\n)+)", mk, flags=re.M)
    assert rule and all(f in rule.group(1) for f in ("-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "batch_rate_map_example.c"))
    assert "hip/hip_runtime" not in open(os.path.join(ROOT, "tools", "batch_rate_map_example.c")).read()
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "speedy_amd", "csrc"), "ratemapexample"])
    assert os.path.exists(os.path.join(ROOT, "speedy_amd", "lib", "batch_rate_map_example"))


def test_rate_pair_and_F_on_hand_worked_values():
    """16 kHz at 1.25: (int)(12800.0f) = 12800 against 16000, both within 14 bits.  22.05 kHz at 1.3: (int)(16961.54f) = 16961
    against 22050, halved once -- 8480 (a bit dropped) and 11025.  F: nothing before the second frame, then the ceiling."""
    assert tr.rate_pair(16000, 1.25) == (12800, 16000)
    assert tr.rate_pair(22050, 1.3) == (8480, 11025)
    assert tr.rate_pair(22050, 0.5) == (11025, 5512)            # 44100 and 22050 halved twice
    assert tr.rate_pair(16000, 0.5) == (16000, 8000)            # 32000 and 16000 halved once
    assert [tr.F(m, 12800, 16000) for m in (-5, 0, 1, 2, 3, 6, 11)] == [0, 0, 0, 1, 2, 4, 8]
    assert [tr.F(m, 16000, 8000) for m in (1, 2, 3, 100)] == [0, 2, 4, 198]


_ROWS = {}


def _rows(orc, shape, rate, chunk):
    """The oracle's rows of a shape at a playback rate (None: sonicSetRate never called) and a chunking, computed once."""
    key = (shape, rate, chunk)
    if key not in _ROWS:
        rate_hz, ch, speed, nl, n, fb = shape
        _ROWS[key] = tr.oracle_rate_map(orc, tm.signal(rate_hz, ch, n), rate_hz, ch, speed, nl, fb, rate, chunk)
    return _ROWS[key]


@pytest.mark.parametrize("shape", tr.SHAPES, ids=IDS)
def test_the_oracles_rows_at_a_rate_are_F_of_its_rows_at_rate_one(orc, shape):
    """Every rate and every chunking: row k of the rate stream is F(row k of the stream at rate 1), the last row is the stream's
    total; the rows never decrease, the last included; they do not depend on the chunking; rate 1 gives oracle_map's rows."""
    rate_hz, ch, speed, nl, n, fb = shape
    base = _rows(orc, shape, None, None)
    plain = tm.oracle_map(orc, tm.signal(rate_hz, ch, n), rate_hz, ch, speed, nl, False, fb)[0]
    assert np.array_equal(base, plain)
    assert np.array_equal(_rows(orc, shape, 1.0, None), plain), "sonicSetRate(1) changes the rows"
    assert base.size == tm.map_rows(rate_hz // 100, n, nl)
    for rate in tr.RATES:
        M = _rows(orc, shape, rate, None)
        assert M.size == base.size, "the rate stage changes no row count"
        want = tr.convert_rows(base, rate_hz, rate, M[-1])
        assert np.array_equal(M, want), "rate %g: rows %s, F of the rows at rate 1 gives %s" % (rate, M, want)
        assert (np.diff(M) >= 0).all(), "rate %g: the rows decrease" % rate
        for chunk in tr.CHUNKINGS[1:]:
            assert np.array_equal(_rows(orc, shape, rate, chunk), M), "rate %g: the rows depend on the chunking (%s)" % (rate, chunk)


def test_the_shapes_reach_the_edges():
    """The halving that drops a bit, a job of 301 rows, an empty job, one shorter than a ring buffer, a linear one."""
    assert (22050, 2, 1.5, 1.0, 11025, 0.0) in tr.SHAPES and (tr.rate_pair(22050, 1.3)[0] * 2 + 1, tr.rate_pair(22050, 1.3)[1] * 2) == (16961, 22050)
    assert tm.map_rows(160, 48000, 1.0) == 301 and (16000, 1, 0.8, 1.0, 48000, 0.1) in tr.SHAPES
    assert any(s[4] == 0 for s in tr.SHAPES) and any(0 < s[4] < s[0] // 100 for s in tr.SHAPES) and any(s[3] == 0.0 for s in tr.SHAPES)


def _definition_rows(orc, shape, rate):
    """The rows a tsm_ref.RateStream gives: frames_out before each event's write, the final count behind the flush; a linear job is
    one write and the flush.  The event speeds come from the oracle's speed tap (tsm_ref.event_speeds)."""
    import tsm_ref as T
    rate_hz, ch, speed, nl, n, fb = shape
    x = tm.signal(rate_hz, ch, n)
    if nl == 0:
        return [T.rate_job(x, rate_hz, ch, speed, rate).frames_out]
    tap = orc.compress_sound(x, rate_hz, ch, speed, nl, fb, False, chunk=1000, taps=True)["speed"] if n else []
    speeds = T.event_speeds(n, rate_hz, tap, speed)
    B = rate_hz // 100
    s = T.RateStream(rate_hz, ch, rate)
    rows = []
    for k, sp in enumerate(speeds):
        rows.append(s.frames_out)
        s.write(x[k * B * ch:(k + 1) * B * ch], sp)
    s.flush(speeds[-1] if speeds else speed)
    rows.append(s.frames_out)
    return rows


@pytest.mark.parametrize("shape", [s for s in tr.SHAPES if s[4] <= 4000], ids=[i for s, i in zip(tr.SHAPES, IDS) if s[4] <= 4000])
def test_the_definitions_rate_stream_gives_the_oracles_rows(orc, shape):
    """On the shapes of at most 4000 frames (RateStream.write is quadratic) the exact definition's rows equal the oracle's, at every rate."""
    for rate in tr.RATES:
        got = _definition_rows(orc, shape, rate)
        want = _rows(orc, shape, rate, None)
        assert got == want.tolist(), "rate %g: the definition gives %s, the oracle %s" % (rate, got, want)


def test_float_batch_with_a_map_has_no_cpu_path():
    """Without a GPU a float batch with a time map refuses to exist, as Plan does (and a rate batch with a map no longer raises ValueError)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from speedy_amd.batch import Batch, FloatBatch
    with pytest.raises(RuntimeError):
        FloatBatch(None, [16000], 1, 3.5, rate=1.25, time_map=True)
    with pytest.raises(RuntimeError):
        Batch(None, [16000], 1, 3.5, rate=1.25, time_map=True)

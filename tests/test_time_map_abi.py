"""CPU-only: the C ABI of the time map (spx_plan_map_rows, spx_batch_run_map, spx_map_lookup) and what makes its expected values
well defined -- the oracle's rows, observed through the hand-off callback, do not depend on how the input is chunked -- and the
numpy statement of the lookups (tests/time_map_ref.py) checked on those rows."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time_map_ref as tm  # noqa: E402

NEW = ["spx_plan_map_rows", "spx_batch_run_map", "spx_map_lookup"]


def test_the_abi_has_the_map_calls_and_keeps_its_layout(tmp_path):
    """The header declares the three functions, the built library exports them, the Python binding lists them; the ABI version
    is still 1 and spx_stream_job is still 48 bytes (the map travels beside the job table, not in it)."""
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


_MAPS = {}


def _maps(orc, shape):
    """The oracle's rows of a shape under three chunkings (one piece, 97, 1000), computed once."""
    if shape not in _MAPS:
        rate_hz, ch, speed, nl, n = shape
        x = tm.signal(rate_hz, ch, n)
        _MAPS[shape] = [tm.oracle_map(orc, x, rate_hz, ch, speed, nl, chunk=c) for c in (None, 97, 1000)]
    return _MAPS[shape]


@pytest.mark.parametrize("shape", tm.SHAPES, ids=lambda s: "%d-%dch-%gx-nl%g-%d" % s)
def test_oracle_rows(orc, shape):
    """Row count, the callback's times, M[0] = 0, monotone rows, last row = the stream's total, the same rows for every chunking."""
    rate_hz, ch, speed, nl, n = shape
    B = rate_hz // 100
    R = n // B if nl != 0 else 0
    runs = _maps(orc, shape)
    M, times, out = runs[0]
    assert M.size == tm.map_rows(B, n, nl) == R + 1
    assert times == list(range(R)), "the hand-off callback fires once per complete ring buffer, in order"
    if nl == 0:
        assert times == []
    if R >= 1:
        assert M[0] == 0
    assert (np.diff(M) >= 0).all()
    assert M[-1] == out.size // ch
    assert M[-1] > 0 or n < B   # (a nonlinear stream shorter than a ring buffer hands nothing over, flush included)
    for Mc, tc, oc in runs[1:]:
        assert np.array_equal(Mc, M) and tc == times and np.array_equal(oc, out)


def test_the_first_shape_has_flat_runs(orc):
    """The time-scale stage works in whole pitch periods: most hand-offs produce nothing, so consecutive rows repeat."""
    M = _maps(orc, tm.SHAPES[0])[0][0]
    assert M.size == 26 and np.unique(M).size < M.size


@pytest.mark.parametrize("shape", tm.SHAPES, ids=lambda s: "%d-%dch-%gx-nl%g-%d" % s)
def test_numpy_lookups_on_the_oracle_rows(orc, shape):
    rate_hz, ch, speed, nl, n = shape
    B = rate_hz // 100
    M = _maps(orc, shape)[0][0]
    X, Y = tm.nodes(M, B, n, nl)
    # forward hits every node
    assert np.array_equal(tm.forward(M, B, n, nl, X), Y)
    # both directions are non-decreasing over their whole domain and clamp outside it
    t = np.arange(-3, n + 4, dtype=np.int64)
    f = tm.forward(M, B, n, nl, t)
    assert (np.diff(f) >= 0).all() and f[0] == 0 and f[-1] == Y[-1]
    u = np.arange(-3, Y[-1] + 4, dtype=np.int64)
    g = tm.inverse(M, B, n, nl, u)
    assert (np.diff(g) >= 0).all() and g[-1] == n
    # (output frame 0 belongs to the LAST node that still has nothing behind it -- the stage holds input back before its first
    # frame; u >= Y[L-1] answers n_in, so an empty output maps everything to the input's end)
    assert g[0] == (X[np.nonzero(Y == 0)[0][-1]] if Y[-1] > 0 else n)
    # forward(inverse(u)) never overshoots
    uu = np.arange(0, Y[-1] + 1, dtype=np.int64)
    assert (tm.forward(M, B, n, nl, tm.inverse(M, B, n, nl, uu)) <= uu).all()
    # a u that sits on a flat run resolves to the run's LAST node
    flat = [j for j in range(Y.size - 1) if Y[j] == Y[j + 1]]
    for j in flat:
        if Y[j] >= Y[-1]:
            continue
        last = max(k for k in range(Y.size) if Y[k] == Y[j])
        assert tm.inverse(M, B, n, nl, [Y[j]])[0] == X[last]
    if shape == tm.SHAPES[0]:
        assert flat, "the first shape has flat runs to test this on"


def test_empty_job_lookups():
    """n_in = 0: one node pair [0, 0], every query answers 0."""
    for nl in (0.0, 1.0):
        assert tm.forward([0], 160, 0, nl, [-1, 0, 5]).tolist() == [0, 0, 0]
        assert tm.inverse([0], 160, 0, nl, [-1, 0, 5]).tolist() == [0, 0, 0]


def test_batch_with_a_map_has_no_cpu_path():
    """Without a GPU a batch with a time map refuses to exist, as Plan does."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from speedy_amd.batch import Batch
    with pytest.raises(RuntimeError):
        Batch(None, [16000], 1, 3.5, time_map=True)

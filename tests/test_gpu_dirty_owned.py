"""GPU: no result depends on what the memory the LIBRARY allocates for itself held when it was new.

Pipeline slots, the pool's workspace, block cache and record arrays, the state of the drop-in stream API and of the unit-level API
are hipMalloc / hipMallocAsync blocks; a fresh process usually gets zero pages, which is the reference's initial state of almost
everything.  spx_debug_set_alloc_fill(byte) makes every such block hold that byte when it is new (speedy_amd/csrc/spx_internal.h:
spx_dev_alloc).  Every scenario is created AFTER the switch is set -- with bytes 0xFF (NaN, -1) and 0x7F (huge finite values) -- and
held against the oracle call for call, with the helpers of the files that test these APIs on fresh memory.  The switch is reset in a
finally.  (Blocks that the process-wide pool cached before the switch was set keep what they held: the handles made here get new
state records and, as they grow, new blocks.)"""
import contextlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dirty_memory as D  # noqa: E402
import test_gpu_dirty_memory as M  # noqa: E402

pytestmark = pytest.mark.gpu
FILLS = [0xFF, 0x7F]


@contextlib.contextmanager
def alloc_fill(byte):
    from speedy_amd import lib
    L = lib()
    L.spx_debug_set_alloc_fill(int(byte))
    try:
        yield
    finally:
        L.spx_debug_set_alloc_fill(-1)


# ---------------------------------------------------------------- the pipeline object ----------------------------------------------------------------

def _content(table, k):
    """Batch k of three: the table's jobs on other samples of the same lengths."""
    x = M._wav("tapestry.wav")
    return [(x[3000 + 500 * k + 41 * i:3000 + 500 * k + 41 * i + t[0].size].copy(),) + t[1:] for i, t in enumerate(table)]


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("kind", ["int16", "float", "rate", "jobs", "mixed"])
def test_three_batches_through_a_depth_2_pipeline(orc, kind, fill):
    """int16 (device input with a dirty pad behind it; also against the plain call's bytes), SPX_PIPELINE_FLOAT,
    spx_pipeline_create_rate, a job table per batch (shorter streams every batch), the mixed pipeline."""
    import torch
    from speedy_amd.batch import Batch, Pipeline
    from test_batch_float_abi import oracle_float_stream
    from test_batch_rate_abi import oracle_rate_stream
    rate, ch, table = M.table16()
    plans, pidx = M.plan_of(rate), None
    if kind == "mixed":
        t22 = M.table22()[2]
        table = table[:4] + t22 + table[4:]
        plans, pidx = [M.plan_of(rate), M.plan_of(22050)], [0] * 4 + [1] * 3 + [0] * 4
    rates_of = (lambda i: 22050 if pidx and pidx[i] else rate)
    lens = [t[0].size for t in table]
    with alloc_fill(fill):
        pipe = Pipeline(plans, lens, 1, [t[1] for t in table], [t[2] for t in table], [t[3] for t in table], depth=2, plan_index=pidx,
                        float_samples=kind == "float", rate=M.RATES16 if kind == "rate" else None)
        try:
            tickets, batches, keep = [], [], []

            def check(k):
                """Batch k's outputs: fetched while batch k + 1 is in flight (depth 2: its buffers go to batch k + 2)."""
                outs = pipe.results(tickets[k])
                for i, e in enumerate(batches[k]):
                    if kind == "float":
                        want = oracle_float_stream(orc, M.floats(e[0]), rate, 1, e[1], e[2], None, False, e[3])
                    elif kind == "rate":
                        want = oracle_rate_stream(orc, e[0], rate, 1, e[1], e[2], M.RATES16[i], False, e[3])
                    else:
                        want = M.orc_job(orc, rates_of(i), 1, e)["out"]
                    assert outs[i].size == want.size and outs[i].tobytes() == want.tobytes(), \
                        "%s pipeline, fill 0x%02X, batch %d, lane %d: not the oracle's output (%d, %d values)" % (kind, fill, k, i, outs[i].size, want.size)
                if kind == "int16" and k == 0:
                    b = M.make(Batch, plans, 1, batches[k])
                    b.upload([e[0] for e in batches[k]])
                    b.run()
                    for i, o in enumerate(b.results()):
                        assert o.tobytes() == outs[i].tobytes(), "int16 pipeline, fill 0x%02X, lane %d: not the plain call's bytes" % (fill, i)

            for k in range(3):
                tab = _content(table, k) if kind != "mixed" else table
                if kind == "jobs":
                    tab = [(t[0][:max(0, t[0].size - 13 * k * (i % 3))],) + t[1:] for i, t in enumerate(tab)]
                kl = [t[0].size for t in tab]
                if kind == "float":
                    x = pipe.pack([M.floats(t[0]) for t in tab])
                    tickets.append(pipe.submit(x))
                elif kind == "jobs":
                    tickets.append(pipe.submit_jobs(pipe.pack([t[0] for t in tab], kl), kl))
                elif kind == "int16":
                    # a device input: the 64 values behind it are the caller's, and they hold anything
                    d = D.fill(torch.empty(pipe.total_in + 64, dtype=torch.int16, device="cuda"), "random", 20 + k)
                    d[:pipe.total_in].copy_(torch.from_numpy(pipe.pack([t[0] for t in tab])))
                    keep.append(d)
                    tickets.append(pipe.submit(d))
                else:
                    tickets.append(pipe.submit(pipe.pack([t[0] for t in tab])))
                batches.append(tab)
                if k >= 1:
                    check(k - 1)
            check(2)
        finally:
            pipe.close()


# ---------------------------------------------------------------- the drop-in stream API ----------------------------------------------------------------

def _two_lives(x, ch, chunk=1000):
    """write / read in chunks, flush, drain -- and again on the second half: both lives of a handle."""
    n = x.size // ch
    ops = []
    for lo, hi in ((0, n // 2), (n // 2, n)):
        for pos in range(lo, hi, chunk):
            ops += [("w", x[pos * ch:min(hi, pos + chunk) * ch]), ("r", chunk)]
        ops += [("f",), ("r", 400000), ("r", 10)]
    return ops


STREAM_CASES = {"linear": (2.0, 0.0, None), "nonlinear": (3.5, 1.0, None), "rate": (2.0, 0.0, 1.25)}


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("coalesce", [True, False])
@pytest.mark.parametrize("case", list(STREAM_CASES))
def test_the_stream_api_on_int16_samples_through_both_lives(orc, case, coalesce, fill):
    """Against the oracle shim call for call (tests/test_gpu_sonic2.py _drive_both), handle created after the switch is set."""
    from speedy_amd.sonic2 import SonicStream
    from test_gpu_sonic2 import _drive_both
    speed, nl, playback = STREAM_CASES[case]
    rate, ch = 16000, 1
    x = M._wav("tapestry.wav")[:24000]
    L = orc.lib()
    with alloc_fill(fill):
        h = L.orc_sonicCreateStream(rate, ch, 0)
        s = SonicStream(rate, ch, False, coalesce)
        try:
            L.orc_sonicSetSpeed(h, speed); s.set_speed(speed)
            L.orc_sonicEnableNonlinearSpeedup(h, nl); s.enable_nonlinear(nl)
            if playback is not None:
                L.orc_sonicSetRate(h, playback); s.set_rate(playback)
            _drive_both(orc, L, h, s, _two_lives(x, ch), np.zeros(400000 * ch, np.int16))
        finally:
            L.orc_sonicDestroyStream(h)
            s.close()


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("coalesce", [True, False])
@pytest.mark.parametrize("case", list(STREAM_CASES))
def test_the_stream_api_on_float_samples_through_both_lives(orc, case, coalesce, fill):
    """sonicWriteFloatToStream / sonicReadFloatFromStream against the shim's, call for call."""
    from speedy_amd.sonic2 import SonicStream
    speed, nl, playback = STREAM_CASES[case]
    rate, ch = 16000, 1
    xf = M.floats(M._wav("tapestry.wav")[:24000])
    L = orc.lib()
    buf = np.zeros(400000, np.float32)
    with alloc_fill(fill):
        h = L.orc_sonicCreateStream(rate, ch, 0)
        s = SonicStream(rate, ch, False, coalesce)
        try:
            L.orc_sonicSetSpeed(h, speed); s.set_speed(speed)
            L.orc_sonicEnableNonlinearSpeedup(h, nl); s.enable_nonlinear(nl)
            if playback is not None:
                L.orc_sonicSetRate(h, playback); s.set_rate(playback)
            for i, op in enumerate(_two_lives(xf, ch)):
                if op[0] == "w":
                    part = np.ascontiguousarray(op[1])
                    assert L.orc_sonicWriteFloatToStream(h, orc.fptr(part), part.size) == 1
                    assert s.write_float(part) == 1, (i, s.L.speedyHipLastError())
                elif op[0] == "f":
                    L.orc_sonicFlushStream(h)
                    assert s.flush() == 1
                else:
                    n = L.orc_sonicReadFloatFromStream(h, orc.fptr(buf), op[1])
                    got = s.read_float(op[1])
                    assert got.size == n and got.tobytes() == buf[:n].tobytes(), (case, coalesce, fill, i, got.size, n)
        finally:
            L.orc_sonicDestroyStream(h)
            s.close()


# ---------------------------------------------------------------- the pool ----------------------------------------------------------------

@pytest.mark.parametrize("fill", FILLS)
def test_sixteen_interleaved_pooled_handles(orc, fill):
    """tests/test_gpu_pool.py's schedule with 16 handles of its mixed kinds: 1000-frame writes to all of them, then a read from each,
    flush, drain -- counts and bytes per call as the oracle's."""
    from speedy_amd.sonic2 import SonicStream
    from test_gpu_pool import _Ref, _configs
    cfg = _configs(16, 1)
    for c in cfg:
        c["x"] = c["x"][:8000 * c["ch"]]
    with alloc_fill(fill):
        refs = [_Ref(orc, c["rate"], c["ch"], c["speed"], c["nl"], c["fb"], c["mm"]) for c in cfg]
        hs = []
        try:
            for c in cfg:
                s = SonicStream(c["rate"], c["ch"], c["mm"], True)
                s.set_speed(c["speed"]); s.enable_nonlinear(c["nl"]); s.set_feedback(c["fb"])
                hs.append(s)
            for pos in range(0, 8000, 1000):
                for c, ref, s in zip(cfg, refs, hs):
                    seg = c["x"][pos * c["ch"]:(pos + 1000) * c["ch"]]
                    ref.write(seg)
                    assert s.write_short(seg) == 1
                for i, (ref, s) in enumerate(zip(refs, hs)):
                    want, got = ref.read(1000), s.read_short(1000)
                    assert got.size == want.size and np.array_equal(got, want), (fill, i, pos, got.size, want.size)
            for ref, s in zip(refs, hs):
                ref.flush()
                assert s.flush() == 1
            for i, (ref, s) in enumerate(zip(refs, hs)):
                while True:
                    want, got = ref.read(4096), s.read_short(4096)
                    assert np.array_equal(got, want), (fill, i, "drain")
                    if want.size == 0:
                        break
        finally:
            for ref in refs:
                ref.close()
            for s in hs:
                s.close()


# ---------------------------------------------------------------- the unit-level API ----------------------------------------------------------------

@pytest.mark.parametrize("fill", FILLS)
def test_the_unit_apis_known_answers(orc, fill):
    """The reference KATs of tests/test_gpu_speedy_unit.py on streams and filters created after the switch is set: the spectrogram,
    the tension KAT with the spectrogram history (both hysteresis shapes), the hysteresis triangle, the first-order filter, local
    energy and spectral difference on speedyGetSpectrogramAtTime's rows."""
    import test_gpu_speedy_unit as U
    with alloc_fill(fill):
        U.test_spectrogram_known_answers()
        for mm in (True, False):
            U.test_tension_known_answer_and_oracle_equality(orc, mm)
            U.test_hook_hysteresis_triangle(orc, mm)
        U.test_hook_first_order_filter()
        U.test_hook_local_energy(orc)
        U.test_hook_spectral_difference(orc)

"""GPU: ready reads on coalesced handles (include/sonic2.h SPEEDY_HIP_COALESCE_READY, speedy_amd/csrc/sonic2_pool.hip).  A read
returns what the host already holds and never waits for the GPU, except behind a flush; the audio a handle delivers over its
life is the oracle's bit for bit, and what it has delivered never runs ahead of the oracle's readable count.  Driven in the
reference's own call order -- write a chunk, read what is ready, next handle (speedy_wave.cc:199-231, sonic_test.cc:384-400)."""
import os
import subprocess
import threading

import numpy as np
import pytest

from util import GOLDEN, read_wav

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Ref:
    """One oracle-shim stream (orc_sonic2.c, the reference shim restated)."""

    def __init__(self, orc, rate, ch, speed, nl, fb=0.0, mm=False):
        self.orc, self.L, self.ch = orc, orc.lib(), ch
        self.h = self.L.orc_sonicCreateStream(rate, ch, int(mm))
        self.L.orc_sonicSetSpeed(self.h, speed)
        self.L.orc_sonicEnableNonlinearSpeedup(self.h, nl)
        self.L.orc_sonicSetDurationFeedbackStrength(self.h, fb)
        self.buf = np.zeros(16384 * ch, np.int16)
        self.fbuf = np.zeros(16384 * ch, np.float32)

    def write(self, seg):
        seg = np.ascontiguousarray(seg, np.int16)
        assert self.L.orc_sonicWriteShortToStream(self.h, self.orc.sptr(seg), seg.size // self.ch) == 1

    def write_float(self, seg):
        seg = np.ascontiguousarray(seg, np.float32)
        assert self.L.orc_sonicWriteFloatToStream(self.h, self.orc.fptr(seg), seg.size // self.ch) == 1

    def read(self, n):
        k = self.L.orc_sonicReadShortFromStream(self.h, self.orc.sptr(self.buf), n)
        return self.buf[:k * self.ch].copy()

    def read_float(self, n):
        k = self.L.orc_sonicReadFloatFromStream(self.h, self.orc.fptr(self.fbuf), n)
        return self.fbuf[:k * self.ch].copy()

    def set_speed(self, v):
        self.L.orc_sonicSetSpeed(self.h, v)

    def flush(self):
        self.L.orc_sonicFlushStream(self.h)

    def close(self):
        self.L.orc_sonicDestroyStream(self.h)


def _stream(rate, ch, speed, nl, fb=0.0, mm=False, coalesce="ready"):
    from speedy_amd.sonic2 import SonicStream
    s = SonicStream(rate, ch, mm, coalesce)
    s.set_speed(speed)
    s.enable_nonlinear(nl)
    s.set_feedback(fb)
    return s


def _drain(read, n=4096):
    """The reference's drain after a flush: read until a read returns nothing (speedy_wave.cc:223-231)."""
    outs = []
    while True:
        got = read(n)
        if got.size == 0:
            return outs
        outs.append(got)


def _cat(parts, dtype=np.int16):
    return np.concatenate(parts) if parts else np.zeros(0, dtype)


def _configs(n, seed):
    """Handles of mixed kinds: 16 / 22.05 kHz, mono / stereo, linear / nonlinear, feedback, both hysteresis shapes, 0.8 - 2 s."""
    rng = np.random.default_rng(seed)
    from speedy_amd.synth import speech_like
    tap, _, _ = read_wav("tapestry.wav")
    out = []
    for i in range(n):
        rate = 16000 if i % 4 != 3 else 22050
        ch = 2 if i % 8 == 5 else 1
        nl = 0.0 if i % 5 == 4 else 1.0
        speed = float(rng.choice([1.5, 2.0, 3.5, 3.5]))
        fb = 0.1 if i % 7 == 6 else 0.0
        mm = bool(i % 2)
        secs = float(rng.uniform(0.8, 2.0))
        if i % 6 == 0:
            x = np.roll(tap, 997 * i)[: int(secs * rate)]
        else:
            x = speech_like(int(secs * rate), rate, seed=200 + i)
        if ch == 2:
            x = np.stack([x, np.roll(x, 3)], axis=1).reshape(-1)
        out.append(dict(rate=rate, ch=ch, nl=nl, speed=speed, fb=fb, mm=mm, x=np.ascontiguousarray(x, np.int16)))
    return out


class _Pair:
    """A GPU handle and its oracle twin, driven by the same calls; keeps what both delivered."""

    def __init__(self, orc, c, chunk, coalesce="ready"):
        self.c, self.ch, self.chunk = c, c["ch"], chunk
        self.ref = _Ref(orc, c["rate"], c["ch"], c["speed"], c["nl"], c["fb"], c["mm"])
        self.s = _stream(c["rate"], c["ch"], c["speed"], c["nl"], c["fb"], c["mm"], coalesce)
        self.pos = 0
        self.want, self.got = [], []
        self.n_want = self.n_got = 0

    def frames(self):
        return self.c["x"].size // self.ch

    def live(self):
        return self.pos < self.frames()

    def step(self):
        """Write the next chunk to both, read at most `chunk` frames from both; returns (gpu frames, oracle frames)."""
        seg = self.c["x"][self.pos * self.ch:(self.pos + self.chunk) * self.ch]
        self.pos += self.chunk
        self.ref.write(seg)
        assert self.s.write_short(seg) == 1
        w, g = self.ref.read(self.chunk), self.s.read_short(self.chunk)
        self.want.append(w)
        self.got.append(g)
        self.n_want += w.size // self.ch
        self.n_got += g.size // self.ch
        assert self.n_got <= self.n_want, ("ran ahead of the reference", self.n_got, self.n_want)
        return g.size // self.ch, w.size // self.ch

    def flush_and_drain(self):
        self.ref.flush()
        assert self.s.flush() == 1
        self.want += _drain(self.ref.read, self.chunk)
        self.got += _drain(self.s.read_short, self.chunk)
        assert self.s.read_short(self.chunk).size == 0   # the drain's 0 came after the last frame and stays 0

    def check(self, tag):
        want, got = _cat(self.want), _cat(self.got)
        assert want.size > 0 and got.size == want.size and np.array_equal(got, want), (tag, got.size, want.size)

    def close(self):
        self.ref.close()
        self.s.close()


def test_read_that_launches_returns_nothing(orc):
    """The read right after a write on a ready handle launches the staged work and returns 0 (its frames are not on the host yet);
    the same calls on a default coalesced handle return the oracle's count.  Flush and drain then deliver the oracle's audio."""
    x, rate, ch = read_wav("tapestry.wav")
    seg = x[:32000]
    ref = _Ref(orc, rate, ch, 3.5, 1.0)
    ready = _stream(rate, ch, 3.5, 1.0, coalesce="ready")
    blocking = _stream(rate, ch, 3.5, 1.0, coalesce=True)
    ref.write(seg)
    want = ref.read(16384)
    assert ready.write_short(seg) == 1
    got_ready = ready.read_short(16384)
    assert blocking.write_short(seg) == 1   # (after the ready read: the blocking read runs whatever is staged, on any handle)
    got_blocking = blocking.read_short(16384)
    assert want.size > 0 and np.array_equal(got_blocking, want)
    assert got_ready.size == 0
    ref.flush()
    assert ready.flush() == 1
    want_all = _cat([want] + _drain(ref.read))
    got_all = _cat([got_ready] + _drain(ready.read_short))
    assert got_all.size == want_all.size and np.array_equal(got_all, want_all)
    ref.close(); ready.close(); blocking.close()


def test_reference_order_matches_oracle(orc):
    """64 ready handles of mixed kinds in the reference's order (1000- or 128-frame chunks, read with bufferSize = chunk, next
    handle), then flush and drain each: bit-exact audio per handle, never ahead of the oracle after any call."""
    cfg = _configs(64, 11)
    pairs = [_Pair(orc, c, 1000 if i % 2 == 0 else 128) for i, c in enumerate(cfg)]
    zeros = 0
    while any(p.live() for p in pairs):
        for p in pairs:
            if p.live():
                g, w = p.step()
                zeros += (g == 0 and w > 0)
    for i, p in enumerate(pairs):
        p.flush_and_drain()
        p.check(i)
        p.close()
    assert zeros > 0   # (the reads really did not wait)


def test_ready_and_blocking_handles_share_a_pool(orc):
    """16 default and 16 ready handles interleaved on one thread: every read of a default handle still returns the oracle's
    count and bytes, call for call; every ready handle delivers the oracle's audio."""
    cfg = _configs(32, 12)
    pairs = [_Pair(orc, c, 1000, coalesce=True if i % 2 == 0 else "ready") for i, c in enumerate(cfg)]
    while any(p.live() for p in pairs):
        for i, p in enumerate(pairs):
            if p.live():
                g, w = p.step()
                if i % 2 == 0:
                    assert g == w and np.array_equal(p.got[-1], p.want[-1]), (i, p.pos, g, w)
    for p in pairs:   # every flush first, then the drains (a drain's wait runs the other handles' flushes as well)
        p.ref.flush()
        assert p.s.flush() == 1
    for i, p in enumerate(pairs):
        want, got = _drain(p.ref.read, 1000), _drain(p.s.read_short, 1000)
        if i % 2 == 0:
            assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want)), (i, "drain")
        p.want += want
        p.got += got
        p.check(i)
        p.close()


def test_threads(orc):
    """16 threads x 4 ready handles, each thread in the reference's order on its own handles: every handle's audio is the
    oracle's."""
    T, M = 16, 4
    cfg = _configs(T * M, 13)
    errors = []
    start = threading.Barrier(T)

    def worker(t):
        try:
            pairs = [_Pair(orc, c, 1000) for c in cfg[t * M:(t + 1) * M]]
            start.wait()
            while any(p.live() for p in pairs):
                for p in pairs:
                    if p.live():
                        p.step()
            for i, p in enumerate(pairs):
                p.flush_and_drain()
                p.check((t, i))
                p.close()
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e)[:500])
            try:
                start.abort()
            except Exception:  # noqa: BLE001
                pass

    th = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors[:3]


def _loop(p, steps, each=None):
    for k in range(steps):
        if not p.live():
            break
        if each:
            each(k)
        p.step()


def test_life_cycle_edges(orc):
    """Ready handles through the rest of a stream's life, each against the oracle's audio for the same calls."""
    x, rate, ch = read_wav("tapestry.wav")
    base = dict(rate=rate, ch=ch, nl=1.0, speed=3.5, fb=0.0, mm=False, x=x)

    # sonicSetSpeed between writes (a setter completes what the handle has in flight, then the next job runs at the new speed)
    p = _Pair(orc, base, 1000)
    _loop(p, 60, lambda k: (p.ref.set_speed(2.0), p.s.set_speed(2.0)) if k == 17 else None)
    p.flush_and_drain()
    p.check("set_speed")
    p.close()

    # a second utterance after flush and drain: non-blocking again, and the stream goes on as the reference's does
    p = _Pair(orc, dict(base, x=x[:20000]), 1000)
    _loop(p, 100)
    p.flush_and_drain()
    p.c, p.pos = dict(base, x=np.concatenate([x[:20000], x[30000:45000]])), 20000
    _loop(p, 100)
    p.flush_and_drain()
    p.check("second utterance")
    p.close()

    # float write / float read
    xf = (x.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    ref = _Ref(orc, rate, ch, 2.5, 1.0)
    s = _stream(rate, ch, 2.5, 1.0)
    want, got = [], []
    for pos in range(0, xf.size, 1000):
        ref.write_float(xf[pos:pos + 1000])
        assert s.write_float(xf[pos:pos + 1000]) == 1
        want.append(ref.read_float(1000))
        got.append(s.read_float(1000))
    ref.flush()
    assert s.flush() == 1
    want += _drain(ref.read_float)
    got += _drain(s.read_float)
    want, got = _cat(want, np.float32), _cat(got, np.float32)
    assert want.size > 0 and got.size == want.size and np.array_equal(got, want)
    ref.close(); s.close()

    # a tension callback registered mid-stream: the handle leaves the pool and goes on eagerly (blocking reads from then on)
    p = _Pair(orc, base, 1000)
    seen = ([], [])
    keep = []

    def register(k):
        if k == 9:
            cb = orc.TENSION_FN(lambda _s, t, v: seen[0].append((t, np.float32(v))))
            keep.append(cb)
            p.ref.L.orc_sonicTensionCallback(p.ref.h, cb)
            p.s.on_tension(lambda t, v: seen[1].append((t, np.float32(v))))
    _loop(p, 100, register)
    p.flush_and_drain()
    p.check("callback")
    assert len(seen[0]) > 50 and seen[0] == seen[1]
    p.close()

    # sonicSamplesAvailable never promises more than the next read (with a buffer at least that large) returns
    s = _stream(rate, ch, 3.5, 1.0)
    ref = _Ref(orc, rate, ch, 3.5, 1.0)
    got, want = [], []
    for pos in range(0, x.size, 1000):
        ref.write(x[pos:pos + 1000])
        want.append(ref.read(16384))
        assert s.write_short(x[pos:pos + 1000]) == 1
        a = s.available()
        g = s.read_short(16384)
        assert a <= g.size, (pos, a, g.size)
        got.append(g)
    ref.flush()
    want += _drain(ref.read)
    assert s.flush() == 1
    while True:
        a = s.available()
        g = s.read_short(max(a, 1))
        assert a <= g.size, ("drain", a, g.size)
        if g.size == 0:
            break
        got.append(g)
    want, got = _cat(want), _cat(got)
    assert got.size == want.size and np.array_equal(got, want)
    ref.close(); s.close()

    # a handle destroyed right after the read that launched its run: the others are unaffected and the pool goes on
    pairs = [_Pair(orc, dict(base, x=np.roll(x, 1111 * i)), 1000) for i in range(4)]
    for k in range(30):
        for i, p in enumerate(pairs):
            if p is None:
                continue
            p.step()
            if k == 12 and i == 1:
                p.close()
                pairs[1] = None
    for i, p in enumerate(pairs):
        if p is not None:
            while p.live():
                p.step()
            p.flush_and_drain()
            p.check(("neighbour", i))
            p.close()
    p = _Pair(orc, base, 1000)
    _loop(p, 100)
    p.flush_and_drain()
    p.check("after the destroy")
    p.close()


@pytest.mark.parametrize("args", [["--speed", "3.5", "--nonlinear", "1.0"], ["--speed", "2.0", "--nonlinear", "0.0"]])
def test_reference_cli_ready(tmp_path, args):
    """The reference's own speedy_wave.cc (oracle/_ref/speedy_wave_ref, built by build()) unmodified, with ready reads switched on
    from the environment: the WAV it writes is byte for byte the one it writes without (its drain loop collects everything).
    Skipped where the binary was not built."""
    exe = os.path.join(ROOT, "oracle", "_ref", "speedy_wave_ref")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/speedy_wave_ref not built (build() found no reference tree)")
    outs = {}
    for ready in (False, True):
        env = {k: v for k, v in os.environ.items() if k not in ("SPX_NO_POOL", "SPX_POOL_READY")}
        if ready:
            env["SPX_POOL_READY"] = "1"
        out = tmp_path / ("ready.wav" if ready else "blocking.wav")
        r = subprocess.run([exe, "--input", os.path.join(GOLDEN, "tapestry.wav"), "--output", str(out)] + args,
                           capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
        outs[ready] = open(out, "rb").read()
    assert len(outs[False]) > 44 + 2 * 1000 and outs[True] == outs[False]

"""The int16 inputs the feature-definition tests share (CPU oracle and HIP kernels): speech-like streams and one input built to
reach each branch of the chain.  numpy only; each test asserts that its input reached the branch it was built for."""
import numpy as np

def speech(rate, seconds=1.9, seed=3, ch=1):
    from speedy_amd.synth import speech_like
    return speech_like(int(seconds * rate), rate, seed=seed, channels=ch)


def clicks_in_silence(rate, seconds=2.0):
    """Digital silence with a 25 ms noise burst every 170 ms: long low runs, all-zero rows, non-low frames right after them."""
    rng = np.random.default_rng(7)
    x = np.zeros(int(seconds * rate), np.int16)
    n = int(0.025 * rate)
    for start in range(int(0.21 * rate), x.size - n, int(0.17 * rate)):
        x[start:start + n] = rng.integers(-9000, 9000, n)
    return x


def square_wave(rate, seconds=1.0):
    """Full scale after 0.3 s of a faint one: the energy jumps far above its low-pass, f2 > 2."""
    n = int(seconds * rate)
    x = np.where((np.arange(n) // 37) % 2 == 0, 32767, -32768).astype(np.int16)
    x[:int(0.3 * rate)] //= 200
    return x


def white_noise(rate, seconds=1.0):
    return np.random.default_rng(11).integers(-12000, 12000, int(seconds * rate)).astype(np.int16)


def jumping_tone(rate, silence=3.0, seconds=1.5):
    """Digital silence, then a steady harmonic tone that jumps to an unrelated pitch every 0.3 s.  Over the silence the low-pass
    of the weighted difference sinks from its start value 123.837 (low frames feed it zeros, speedy.c:698-699); each jump is then
    many times what the low-pass holds -- f9 beyond 4 * mean, the clamp of speedy.c:727-728."""
    n = int(seconds * rate)
    t = np.arange(n) / rate
    seg = (t // 0.3).astype(int)
    f = np.array([200.0, 317.0, 171.0, 263.0, 229.0])[seg % 5]
    phase = 2 * np.pi * np.cumsum(f) / rate
    sig = sum(np.sin(h * phase) / h for h in range(1, 9))
    tone = np.round(sig / np.abs(sig).max() * 0.5 * 32767).astype(np.int16)
    return np.concatenate([np.zeros(int(silence * rate), np.int16), tone])

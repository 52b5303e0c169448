"""CPU-only: the definition of the sample-exact position lookup over an edit list (tests/edit_lookup_ref.py), and its C ABI
(spx_edit_index, spx_edit_lookup, spx_debug_last_edit_lookup_grid).

The lists are tests/edit_list_ref.py's (EditStream, pinned against tests/tsm_ref.py and the oracle by tests/test_edit_list_abi.py)
of the directed linear jobs of tests/tsm_inputs.py at 16 and 22.05 kHz and of every nonlinear job, the event speeds of the
nonlinear ones from the oracle's speed tap.  The searched form of the lookup -- a running maximum and a closed form per record, what
the device does -- is held to an enumeration of the source of every output frame, for EVERY input position and EVERY output frame;
the properties the header states are asserted; every switch of edit_lookup_ref (one mistake each) changes an answer."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_list_ref as E  # noqa: E402
import edit_lookup_ref as K  # noqa: E402
import tsm_inputs as I  # noqa: E402
import tsm_ref as T  # noqa: E402

NEW = ["spx_edit_index", "spx_edit_lookup", "spx_debug_last_edit_lookup_grid"]


@pytest.fixture(scope="module")
def lists(orc):
    """{name: (rate, n_in, nonlinear, EditStream)}: computed once, left unchanged."""
    out = {}
    with E.shared_pitch_searches():
        for name, rate, ch, x, speed in I.linear_jobs():
            if rate in (16000, 22050):
                out[name] = (rate, x.size // ch, False, E.linear_job(x, rate, ch, speed))
        for name, rate, ch, x, speed, nl in I.nonlinear_jobs() + I.nonlinear_map_jobs():
            tap = orc.compress_sound(x, rate, ch, speed, nl, 0.0, False, chunk=1000, taps=True)["speed"]
            out[name] = (rate, x.size // ch, True, E.nonlinear_job(x, rate, ch, T.event_speeds(x.size // ch, rate, tap, speed), speed))
    return out


def _lookup(v, switch=None):
    rate, n_in, nl, e = v
    return K.Lookup(e.ops, e.out_n, K.limit_of(n_in, rate, nl, switch), switch)


@pytest.fixture(scope="module")
def answers(lists):
    """{name: (Lookup, forward(p) for p = 0 .. L, inverse(o) for o = 0 .. n_out)} by the searched form."""
    out = {}
    for name, v in lists.items():
        m = _lookup(v)
        out[name] = (m, [m.forward(p) for p in range(m.L + 1)], [m.inverse(o) for o in range(m.n_out + 1)])
    return out


def test_the_inputs_are_the_directed_jobs(lists):
    speeds = {round(float(n.rsplit("/", 1)[1]), 6) for n in lists if n.startswith("speeds/")}
    assert speeds >= {0.5, round(I.below(0.5), 6), 0.7, 2.0, 3.5, 200.0, 0.0001}
    assert any(n.endswith("/0.4") for n in lists)
    assert sum(1 for v in lists.values() if v[2]) == 15 and sum(1 for v in lists.values() if not v[2]) > 200
    for name, (rate, n_in, nl, e) in lists.items():
        assert e.limit == K.limit_of(n_in, rate, nl) == E.limit_of(n_in, rate, nl), name


def test_the_searched_form_is_the_enumeration(answers):
    """forward for every p in [0, L], inverse for every o in [0, n_out], answers and records."""
    for name, (m, fw, iv) in answers.items():
        assert fw == m.brute_forward_all(), name
        assert iv == m.brute_inverse_all(), name
        assert len(fw) == m.L + 1 and len(iv) == m.n_out + 1, name


def test_the_running_maximum_is_needed_below_half_speed_only(lists):
    """Records whose own maximum lies below the running maximum: some in the slow-downs below 0.5, none from 0.7 up."""
    low = {}
    for name, v in lists.items():
        if not v[2]:
            m = _lookup(v)
            low[name] = sum(1 for r, g in zip(m.R, m.G) if r < g)
    assert low["rates/16000Hz/2ch/4800/0.4"] > 0 and low["run/22050Hz/1ch/2981/0.4"] > 0
    assert not {name: k for name, k in low.items() if k and float(name.rsplit("/", 1)[1]) >= 0.7}


def test_the_properties(lists, answers):
    decreasing = 0
    for name, (m, fw, iv) in answers.items():
        f, i = [a for a, _ in fw], [a for a, _ in iv]
        assert all(x <= y for x, y in zip(f, f[1:])), name                                    # forward is non-decreasing
        assert all(f[i[o]] <= o for o in range(m.n_out + 1)), name                             # forward(inverse(o)) <= o
        assert all(i[f[p]] >= p for p in range(m.L + 1) if f[p] < m.n_out), name               # inverse(forward(p)) >= p
        assert m.forward(-5) == fw[0] and m.forward(m.L + 9) == fw[m.L], name                  # the clamps
        assert m.inverse(-5) == iv[0] and m.inverse(m.n_out + 9) == (m.L, -1) == iv[m.n_out], name
        assert all((k == -1) == (a == m.n_out) for a, k in fw), name
        decreasing += sum(1 for x, y in zip(i, i[1:m.n_out]) if y < x)
        e = lists[name][3]
        for k, (out_at, a, b, n) in enumerate(e.ops):                                          # a copy: the frame the replay reads
            if b < 0:
                for t in (0, n // 2, n - 1):
                    if out_at + t < m.n_out:
                        assert iv[out_at + t] == (min(a + t, m.L), k), (name, k, t)
    assert decreasing > 100, "no slow-down plays input twice: the inputs show nothing of the running maximum"


def test_a_list_of_copies_is_the_identity_up_to_L(answers):
    unity = [n for n in answers if n.endswith("/1") and not n.startswith(("nonlinear", "map"))]
    assert len(unity) >= 5
    for name in unity:
        m, fw, iv = answers[name]
        assert all(op[2] < 0 for op in m.ops) and m.n_out == m.L, name
        assert [a for a, _ in fw] == list(range(m.L + 1)) and [a for a, _ in iv] == list(range(m.L + 1)), name


def test_a_dead_stream_answers_minus_one():
    assert K.Lookup([(0, 0, -1, 5)], -3, 5).forward(2) == (-1, -1)
    assert K.Lookup([(0, 0, -1, 5)], 5, 5, n_ops=-1).inverse(2) == (-1, -1)


@pytest.mark.parametrize("switch", K.SWITCHES)
def test_every_switch_changes_an_answer(lists, answers, switch):
    caught = []
    for name, v in lists.items():
        m0, fw, iv = answers[name]
        m = _lookup(v, switch)
        if [m.forward(p) for p in range(m0.L + 1)] != fw or [m.inverse(o) for o in range(m0.n_out + 1)] != iv:
            caught.append(name)
    assert caught, switch
    if switch == "limit_n_in":
        assert all(n.startswith(("nonlinear", "map")) for n in caught), caught
    if switch == "no_prefix_max":
        assert all(float(n.rsplit("/", 1)[1]) < 0.5 for n in caught if n.startswith(("speeds", "rates", "run", "channels", "lengths"))), caught


def test_the_abi_has_the_lookup():
    """The header declares the three functions, the binding lists them, the library exports them; the ABI version is still 1; the
    header no longer calls the lookup a follow-up."""
    import speedy_amd
    from speedy_amd._lib import SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "speedy_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared in include/speedy_hip.h"
        assert name in SYMBOLS, name + " is missing from speedy_amd._lib.SYMBOLS"
    assert len(SYMBOLS["spx_edit_index"][1]) == 8 and len(SYMBOLS["spx_edit_lookup"][1]) == 14
    assert "makes the exact answer possible" not in hdr and "POSITION LOOKUP, TO THE SAMPLE" in hdr
    speedy_amd.build()
    raw = ctypes.CDLL(os.path.join(ROOT, "speedy_amd", "lib", "libspeedy_hip.so"))
    assert not [n for n in NEW if not hasattr(raw, n)]
    raw.spx_abi_version.restype = ctypes.c_int
    assert raw.spx_abi_version() == 1


def test_the_c_example_builds():
    """tools/batch_edit_lookup_example.c builds with gcc -std=c99 -pedantic -Wall -Wextra -Werror (make editlookupexample)."""
    import subprocess
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "speedy_amd", "csrc"), "editlookupexample"])
    assert os.path.exists(os.path.join(ROOT, "speedy_amd", "lib", "batch_edit_lookup_example"))

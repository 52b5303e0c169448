"""Which jobs a batch call takes is one pure function (speedy_amd/csrc/spx_jobs.h: spx_check_job) that every entry point asks
before it enqueues anything.  Here it is compiled by plain g++ into speedy_amd/lib/libspx_mode_table.so (spx_mode_table.cpp) and
asked on the CPU: every value tests/test_gpu_parity.py::test_jobs_outside_the_defined_ranges_are_refused lists, the boundaries,
which rule speaks when two are broken, and the texts.  W = 240, B = 160: the 16 kHz plan's window and frame step."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "speedy_amd", "lib", "libspx_mode_table.so")
OK, COUNTS, SPEED, NONLINEAR, FEEDBACK, RATE_TOO_HIGH, TOO_LONG = range(7)   # SpxJobFault, in the order the rules are applied
NAN, INF = float("nan"), float("inf")
GOOD = dict(analysis_fits=1, channels=1, n_in=4000, in_off=0, out_off=0, out_cap=8000, speed=2.0, nonlinear=1.0, feedback=0.0)


@pytest.fixture(scope="module")
def rules():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "speedy_amd", "csrc"), "modetable"])
    L = C.CDLL(LIB)
    L.spx_mode_table_check_job.argtypes = [C.c_int] * 4 + [C.c_longlong] * 4 + [C.c_float] * 3
    L.spx_mode_table_job_fault_text.restype = C.c_char_p
    L.spx_mode_table_job_fault_text.argtypes = [C.c_int]

    def check(**kw):
        j = dict(GOOD, **kw)
        return L.spx_mode_table_check_job(240, 160, j["analysis_fits"], j["channels"], j["n_in"], j["in_off"], j["out_off"], j["out_cap"],
                                          j["speed"], j["nonlinear"], j["feedback"])
    check.text = lambda code: L.spx_mode_table_job_fault_text(code).decode()
    return check


def test_every_refused_value_has_its_fault(rules):
    assert rules() == OK
    for field, value, fault in [("speed", 0.0, SPEED), ("speed", -1.0, SPEED), ("speed", NAN, SPEED), ("speed", INF, SPEED),
                                ("nonlinear", -0.1, NONLINEAR), ("nonlinear", 1.5, NONLINEAR), ("nonlinear", NAN, NONLINEAR),
                                ("feedback", NAN, FEEDBACK), ("feedback", INF, FEEDBACK), ("channels", 0, COUNTS), ("n_in", -1, COUNTS),
                                ("in_off", -8, COUNTS), ("out_off", -8, COUNTS), ("out_cap", -1, COUNTS)]:
        assert rules(**{field: value}) == fault, (field, value)
    assert rules(speed=-INF) == SPEED and rules(feedback=-INF) == FEEDBACK


def test_boundaries(rules):
    assert rules(n_in=(1 << 30) - 1) == OK
    assert rules(n_in=1 << 30) == TOO_LONG
    assert rules(n_in=1 << 30, nonlinear=0.0) == TOO_LONG
    for nl in (0.0, 1.0, -0.0):
        assert rules(nonlinear=nl) == OK, nl
    assert rules(speed=float(np.finfo(np.float32).tiny)) == OK   # FLT_MIN
    assert rules(n_in=0, out_cap=0) == OK
    # a plan whose analysis tile does not fit a CU's LDS serves linear jobs only
    assert rules(analysis_fits=0, nonlinear=0.0) == OK
    assert rules(analysis_fits=0, nonlinear=-0.0) == OK
    assert rules(analysis_fits=0, nonlinear=1.0) == RATE_TOO_HIGH
    assert rules(analysis_fits=0, nonlinear=1e-3) == RATE_TOO_HIGH


def test_the_first_broken_rule_is_reported(rules):
    broken = {COUNTS: dict(channels=0), SPEED: dict(speed=0.0), NONLINEAR: dict(nonlinear=1.5), FEEDBACK: dict(feedback=NAN),
              RATE_TOO_HIGH: dict(analysis_fits=0), TOO_LONG: dict(n_in=1 << 30)}
    for first in range(COUNTS, TOO_LONG + 1):
        for second in range(first + 1, TOO_LONG + 1):   # every pair, the adjacent ones among them
            assert rules(**broken[first], **broken[second]) == first, (first, second)
    assert rules(channels=0, n_in=-1, speed=NAN, nonlinear=NAN, feedback=INF, analysis_fits=0) == COUNTS


def test_fault_texts(rules):
    texts = [rules.text(code) for code in range(COUNTS, TOO_LONG + 1)]
    assert all(texts) and len(set(texts)) == len(texts)
    assert rules.text(OK) == ""
    for code, word in ((COUNTS, "bad job"), (SPEED, "speed must be finite and > 0"), (NONLINEAR, "nonlinear factor outside [0, 1]"),
                       (FEEDBACK, "feedback strength is not finite"), (RATE_TOO_HIGH, "sample rate too high"), (TOO_LONG, "2^30 frames")):
        assert word in rules.text(code), code
    assert not any(t.startswith("spx_") for t in texts)   # the caller puts its own name (and the pipeline its lane) in front


def test_random_valid_jobs_pass(rules):
    rng = np.random.default_rng(20)
    for i in range(64):
        job = dict(channels=int(rng.integers(1, 9)), n_in=int(rng.integers(0, 1 << 30)), in_off=int(rng.integers(0, 1 << 40)),
                   out_off=int(rng.integers(0, 1 << 40)), out_cap=int(rng.integers(0, 1 << 32)), speed=float(rng.uniform(0.1, 8.0)),
                   nonlinear=float(rng.choice([0.0, 1.0, rng.uniform(0.0, 1.0)])), feedback=float(rng.uniform(-1.0, 1.0)))
        assert rules(**job) == OK, (i, job)

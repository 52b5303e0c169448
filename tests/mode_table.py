"""The engine's launch-mode decision (speedy_amd/csrc/spx_mode.h) through the host-only table library
(speedy_amd/csrc/spx_mode_table.cpp -> speedy_amd/lib/libspx_mode_table.so), fed the resource numbers of the shipped kernels
(profiles/kernel_resources.json) -- test infrastructure, no GPU needed.  tests/test_mode_table.py decides on the CPU with it;
tests/test_gpu_time_map.py replays the time-chunk rule with it beside the call that took it."""
import ctypes as C
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "speedy_amd", "lib", "libspx_mode_table.so")


def load(build=True):
    """decide(shape, **kw) -> {answer field: value}.  shape: 'rate,channels,streams,speedup_only' (a key of kernel_resources.json);
    kw: any query field.  decide.lib is the library, decide.res the resource file.  build=False: the library as build() left it
    (nothing is compiled)."""
    if build:
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "speedy_amd", "csrc"), "modetable"])
    L = C.CDLL(LIB)
    L.spx_mode_table_query_fields.restype = C.c_char_p
    L.spx_mode_table_answer_fields.restype = C.c_char_p
    qf = L.spx_mode_table_query_fields().decode().split()
    af = L.spx_mode_table_answer_fields().decode().split()
    res = json.load(open(os.path.join(ROOT, "profiles", "kernel_resources.json")))
    assert res["fields"] == qf[qf.index("cu_count"): qf.index("an_vgprs_small") + 1], "profiles/kernel_resources.json and spx_mode_table.cpp disagree about the fields"

    def decide(shape, **kw):
        q = dict.fromkeys(qf, 0)
        q.update(dict(zip(res["fields"], res["shapes"][shape])))
        rate, ch, n, sp = (int(v) for v in shape.split(","))
        q.update(n=n, max_channels=ch, do_a=1, do_w=1, has_frames=1, force_total_streams=n, concurrent_enabled=1, chunks=1,
                 trial_state_key=-1, trial_choice=-1, trial_key=77, device_ours=1)
        q.update(kw)
        qa = (C.c_longlong * len(qf))(*[int(q[f]) for f in qf])
        aa = (C.c_longlong * len(af))()
        assert L.spx_mode_table_eval(qa, len(qf), aa, len(af)) == 0
        return dict(zip(af, [int(v) for v in aa]))

    decide.lib = L
    decide.res = res
    return decide

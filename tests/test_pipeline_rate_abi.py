"""CPU-only: the C ABI of the rate pipeline (spx_pipeline_create_rate, spx_pipeline_jobs_fit_rate, spx_pipeline_submit_jobs_rate,
spx_pipeline_submit_jobs_rate_float): a playback rate per lane and per batch through the pipeline object."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["spx_pipeline_create_rate", "spx_pipeline_jobs_fit_rate", "spx_pipeline_submit_jobs_rate", "spx_pipeline_submit_jobs_rate_float"]


def test_the_abi_has_the_rate_pipeline_calls_and_keeps_its_layout(tmp_path):
    """The header declares the four functions, the built library exports them, the Python binding lists them; no flag was added
    (SPX_PIPELINE_DEVICE_OUT = 1, SPX_PIPELINE_FLOAT = 2), the ABI version is still 1 and spx_stream_job is still 48 bytes (the
    rates travel beside the job table, not in it)."""
    import speedy_amd
    from speedy_amd._lib import SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "speedy_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared in include/speedy_hip.h"
        assert name in SYMBOLS, name + " is missing from speedy_amd._lib.SYMBOLS"
    assert sorted(re.findall(r"#define\s+(SPX_PIPELINE_\w+)", code)) == ["SPX_PIPELINE_DEVICE_OUT", "SPX_PIPELINE_FLOAT"]
    speedy_amd.build()
    raw = ctypes.CDLL(os.path.join(ROOT, "speedy_amd", "lib", "libspeedy_hip.so"))
    assert not [n for n in NEW if not hasattr(raw, n)]
    src = "".join(open(os.path.join(ROOT, "speedy_amd", "csrc", f)).read()
                  for f in sorted(os.listdir(os.path.join(ROOT, "speedy_amd", "csrc"))) if f.endswith((".hip", ".cpp")))
    m = re.search(r"int\s+spx_abi_version\s*\(\s*(void)?\s*\)\s*\{\s*return\s+(\d+)\s*;", src)
    assert m and int(m.group(2)) == 1
    prog = tmp_path / "size.c"
    prog.write_text('#include <stdio.h>\n#include "speedy_hip.h"\n'
                    'int main(void) { printf("%u %u %u\\n", (unsigned)sizeof(spx_stream_job), (unsigned)SPX_PIPELINE_DEVICE_OUT,\n'
                    '                        (unsigned)SPX_PIPELINE_FLOAT); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(prog), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().split() == ["48", "1", "2"]


def test_the_header_no_longer_calls_pipeline_rates_out_of_scope():
    hdr = open(os.path.join(ROOT, "include", "speedy_hip.h")).read()
    assert "no pipeline object" not in hdr
    assert "playback rates in the pipeline" not in hdr


def test_c_pipeline_rate_example_builds():
    """make piperateexample: tools/pipeline_rate_example.c under -std=c99 -pedantic -Werror, no HIP headers."""
    mk = open(os.path.join(ROOT, "speedy_amd", "csrc", "Makefile")).read()
    rule = re.search(r"^piperateexample:.*\n((?:\t.*\n)+)", mk, flags=re.M)
    assert rule and all(f in rule.group(1) for f in ("-std=c99", "-pedantic", "-Werror", "pipeline_rate_example.c"))
    assert "hip/hip_runtime" not in open(os.path.join(ROOT, "tools", "pipeline_rate_example.c")).read()
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "speedy_amd", "csrc"), "piperateexample"])
    assert os.path.exists(os.path.join(ROOT, "speedy_amd", "lib", "pipeline_rate_example"))


def test_rate_pipeline_has_no_cpu_path():
    """Without a GPU a rate pipeline refuses to exist, as Plan and a Batch with rates do."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from speedy_amd.batch import Pipeline
    with pytest.raises(RuntimeError):
        Pipeline(None, [16000], 1, 3.5, rate=1.25)

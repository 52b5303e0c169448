"""CPU-only: the C ABI of the pipeline object on float samples (SPX_PIPELINE_FLOAT, the four spx_pipeline_*_float calls)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["spx_pipeline_host_input_float", "spx_pipeline_submit_float", "spx_pipeline_submit_jobs_float", "spx_pipeline_wait_float"]


def test_the_abi_has_the_float_pipeline_calls_and_keeps_its_layout(tmp_path):
    """The header declares the four functions and SPX_PIPELINE_FLOAT = 2, the built library exports them, the Python binding lists
    them; the ABI version is still 1 and spx_stream_job is still 48 bytes."""
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
    prog = tmp_path / "flag.c"
    prog.write_text('#include <stdio.h>\n#include "speedy_hip.h"\n'
                    'int main(void) { printf("%u %u %u\\n", (unsigned)sizeof(spx_stream_job), (unsigned)SPX_PIPELINE_FLOAT,\n'
                    '                        (unsigned)(SPX_PIPELINE_FLOAT | SPX_PIPELINE_DEVICE_OUT)); return 0; }\n')
    exe = tmp_path / "flag"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(prog), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().split() == ["48", "2", "3"]


def test_c_pipeline_float_example_builds():
    """make pipefloatexample: tools/pipeline_float_example.c under -std=c99 -pedantic -Werror, no HIP headers."""
    mk = open(os.path.join(ROOT, "speedy_amd", "csrc", "Makefile")).read()
    rule = re.search(r"^pipefloatexample:.*\n((?:\t.*\n)+)", mk, flags=re.M)
    assert rule and all(f in rule.group(1) for f in ("-std=c99", "-pedantic", "-Werror", "pipeline_float_example.c"))
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "speedy_amd", "csrc"), "pipefloatexample"])
    assert os.path.exists(os.path.join(ROOT, "speedy_amd", "lib", "pipeline_float_example"))


def test_float_pipeline_has_no_cpu_path():
    """Without a GPU a float pipeline refuses to exist, as Plan and FloatBatch do."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from speedy_amd.batch import Pipeline
    with pytest.raises(RuntimeError):
        Pipeline(None, [16000], 1, 3.5, float_samples=True)

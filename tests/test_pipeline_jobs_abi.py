"""CPU-only: the C ABI of the pipeline object's per-batch job table (spx_pipeline_submit_jobs, spx_pipeline_jobs_fit) -- declared,
exported, bound with the right signatures, usable from plain C99 -- and the layout the table travels in."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["spx_pipeline_submit_jobs", "spx_pipeline_jobs_fit"]


def _declarations():
    hdr = open(os.path.join(ROOT, "include", "speedy_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_the_header_declares_both_functions():
    code = _declarations()
    m = re.search(r"\bint64_t\s+spx_pipeline_submit_jobs\s*\(([^)]*)\)\s*;", code)
    assert m, "int64_t spx_pipeline_submit_jobs(...) is not declared in include/speedy_hip.h"
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    assert [re.sub(r"\s*\w+$", "", a) for a in args] == ["spx_pipeline_t", "const spx_stream_job*", "const int16_t*", "int"], args
    m = re.search(r"\bint\s+spx_pipeline_jobs_fit\s*\(([^)]*)\)\s*;", code)
    assert m, "int spx_pipeline_jobs_fit(...) is not declared in include/speedy_hip.h"
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    assert [re.sub(r"\s*\w+$", "", a) for a in args] == ["spx_pipeline_t", "const spx_stream_job*"], args
    # the fixed-shape call stays as it was
    assert re.search(r"\bint64_t\s+spx_pipeline_submit\s*\(\s*spx_pipeline_t\s+\w+\s*,\s*const\s+int16_t\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", code)


def test_the_library_exports_them_and_the_abi_version_stays():
    import speedy_amd
    speedy_amd.build()
    raw = ctypes.CDLL(os.path.join(ROOT, "speedy_amd", "lib", "libspeedy_hip.so"))
    assert not [n for n in NEW if not hasattr(raw, n)]
    assert hasattr(raw, "spx_pipeline_submit")
    src = "".join(open(os.path.join(ROOT, "speedy_amd", "csrc", f)).read()
                  for f in sorted(os.listdir(os.path.join(ROOT, "speedy_amd", "csrc"))) if f.endswith((".hip", ".cpp")))
    m = re.search(r"int\s+spx_abi_version\s*\(\s*(void)?\s*\)\s*\{\s*return\s+(\d+)\s*;", src)
    assert m and int(m.group(2)) == 1          # symbols are only added


def test_the_python_binding_lists_them_with_the_headers_signatures():
    import ctypes as C
    from speedy_amd._lib import SYMBOLS, StreamJob
    assert SYMBOLS["spx_pipeline_submit_jobs"] == (C.c_int64, [C.c_void_p, C.POINTER(StreamJob), C.c_void_p, C.c_int])
    assert SYMBOLS["spx_pipeline_jobs_fit"] == (C.c_int, [C.c_void_p, C.POINTER(StreamJob)])
    assert SYMBOLS["spx_pipeline_submit"] == (C.c_int64, [C.c_void_p, C.c_void_p, C.c_int])
    assert C.sizeof(StreamJob) == 48
    from speedy_amd.batch import Pipeline
    for name in ("submit_jobs", "fits", "pack", "submit", "results", "wait"):
        assert callable(getattr(Pipeline, name, None)), name
    assert "ONE shape" not in Pipeline.__doc__


def test_the_job_table_is_still_48_bytes(tmp_path):
    prog = tmp_path / "size.c"
    prog.write_text('#include <stdio.h>\n#include "speedy_hip.h"\n'
                    'int main(void) { printf("%u\\n", (unsigned)sizeof(spx_stream_job)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(prog), "-o", str(exe)])
    assert int(subprocess.check_output([str(exe)]).decode()) == 48


def test_c_example_compiles_against_the_header(tmp_path):
    """tools/pipeline_jobs_example.c is C99 over include/ alone: no HIP headers, no warnings."""
    src = os.path.join(ROOT, "tools", "pipeline_jobs_example.c")
    assert os.path.exists(src)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", src, "-o", str(tmp_path / "pipeline_jobs_example.o")])
    text = open(src).read()
    assert "hip_runtime" not in text and "spx_pipeline_submit_jobs" in text and "spx_pipeline_jobs_fit" in text


def test_c_example_links_with_the_library():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "speedy_amd", "csrc"), "pipejobsexample"])
    assert os.path.exists(os.path.join(ROOT, "speedy_amd", "lib", "pipeline_jobs_example"))

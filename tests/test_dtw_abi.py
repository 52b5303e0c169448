"""CPU-only: the C side of spx_batch_dtw -- the example program builds as strict C99, and the two structs have the sizes the
header, the Python binding and the kernels agree on."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dtw_example_builds():
    """tools/batch_dtw_example.c builds with gcc -std=c99 -pedantic -Werror (make dtwexample)."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "speedy_amd", "csrc"), "dtwexample"])
    assert os.path.exists(os.path.join(ROOT, "speedy_amd", "lib", "batch_dtw_example"))


def test_struct_sizes(tmp_path):
    """spx_dtw_job is 32 bytes, spx_dtw_result 24 -- for the C compiler and for the Python mirror."""
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "speedy_hip.h"\n'
                   'int main(void) { printf("%d %d %d %d %d\\n", (int)sizeof(spx_dtw_job), (int)sizeof(spx_dtw_result),\n'
                   '  (int)offsetof(spx_dtw_job, path_off), (int)offsetof(spx_dtw_job, n_a), (int)offsetof(spx_dtw_result, n_path));\n'
                   '  return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [32, 24, 16, 24, 16]
    from speedy_amd._lib import DtwJob
    from speedy_amd.dtw import RESULT_DTYPE
    assert ctypes.sizeof(DtwJob) == 32 and DtwJob.path_off.offset == 16 and DtwJob.n_a.offset == 24
    assert RESULT_DTYPE.itemsize == 24 and RESULT_DTYPE.fields["n_path"][1] == 16


def test_source_order_keeps_the_dtw_object_in_front_of_the_replay_object():
    """spx_dtw.hip is a code object of its own, linked in front of spx_edits.hip (spx_twopass.hip stays the last, spx_hot.hip the
    first: tests/test_twopass_abi.py)."""
    mk = open(os.path.join(ROOT, "speedy_amd", "csrc", "Makefile")).read()
    src = [l for l in mk.splitlines() if l.startswith("SRC ?=")][0].split()[2:]
    assert src.index("spx_dtw.hip") + 1 == src.index("spx_edits.hip")
    assert src[0] == "spx_hot.hip" and src[-1] == "spx_twopass.hip"

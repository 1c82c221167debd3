"""The host side of the summed-product entries (SumOperand, phantom-fhe_amd/csrc/pha_sum_operand.h), no GPU:
tests/cpp/test_sum_operand.cpp compiles the header alone into a program of its own, with the address and the undefined-behaviour
sanitizer, and sweeps the view: the output-overlap test against a brute-force intersection (empty batches and no terms included),
the strict-mode runs (every distinct polynomial once, no run above its cap, the former loops' run lists at the real cap), the
advanced view, and every layout refusal with its exception class and text."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sum_operand_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_sum_operand")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_sum_operand.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "SumOperand OK (480 layouts)" in out.stdout, out.stdout + out.stderr

"""The host side of the baby-step / giant-step hoisted rotations (BsgsPlan and BsgsScratch, phantom-fhe_amd/csrc/pha_hoist_plan.h), no
GPU: tests/cpp/test_hoist_plan.cpp compiles the header alone into a program of its own, with the address and the undefined-behaviour
sanitizer, and sweeps the scratch layout (regions in order, without a gap, ending at words(), equal to the sums the entries of
pha_hoist.hip used to write out by hand) and the plan (counts, orderings, every refusal with its exception class and message)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bsgs_plan_and_scratch_layout_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_hoist_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_hoist_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "BsgsScratch layout OK (1296 cases), BsgsPlan OK" in out.stdout, out.stdout + out.stderr

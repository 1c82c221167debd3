"""The host side of the secret-key layer (phantom-fhe_amd/csrc/pha_layout.h), no GPU: tests/cpp/test_layout.cpp compiles the header
alone into a program of its own, with the address and the undefined-behaviour sanitizer, and checks the overlap decision against a
brute-force intersection, every refusal the header decides with its exception class and text, the ORDER of the refusals of the decrypt,
noise, encrypt and sampler entries (rule i and every later rule broken at once: message i), and the chunk size and work-buffer words
of the phase front end against the formulas the entries used to write out."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_layout")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_layout.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "layout OK (304 layouts, 48 chunk cases)" in out.stdout, out.stdout + out.stderr

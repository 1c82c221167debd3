"""The scratch layout of the hybrid key switch (KsScratch, phantom-fhe_amd/csrc/pha_internal.h) on the host, no GPU: the size and the
three region pointers equal the expressions the entries of pha_rns.hip used to write out by hand, so every entry asks its stream's
arena for exactly the words it asked for before (captured graphs depend on stable arenas).  tests/cpp/test_ks_scratch.cpp holds the
cases: the three shapes of the key-switch tests and the most digit polynomials a batched entry admits."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ks_scratch_layout(tmp_path):
    exe = str(tmp_path / "test_ks_scratch")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "test_ks_scratch.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "KsScratch layout OK (4 cases)" in out.stdout, out.stdout + out.stderr

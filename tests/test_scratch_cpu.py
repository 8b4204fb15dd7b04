"""iv_slam_amd/csrc/ivf_scratch.h -- the one routine through which the batched tracker handle allocates and grows its device scratch --
on the host, against the counting fake device of tests/scratch/scratch_host.cpp: first use, growth, a refused allocation at every
position, a failing wait, destroy after each, for sets of 1, 2 and 9 buffers.  The header includes no HIP header, so the program is
plain C++17; it is built with AddressSanitizer (whose leak check makes "every buffer freed exactly once" part of exit 0) and UBSan and
run as a child process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scratch_replacement_on_a_counting_fake_device(tmp_path):
    exe = str(tmp_path / "scratch_host")
    # -static-libasan: the sanitizer's runtime is part of the program, which then starts whatever else the environment loads into it
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-I", os.path.join(ROOT, "iv_slam_amd", "csrc"), os.path.join(ROOT, "tests", "scratch", "scratch_host.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "scratch_host: ok" in run.stdout, run.stdout

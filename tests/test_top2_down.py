"""k_top2_fp4q2 runs the FP4 MFMA without block scales and holds every key 2^-12 times as large (MX_DOWN,
csrc/top2_key.h).  tests/host/top2_down.cpp checks on the CPU, under ASan + UBSan, that every accumulator value then
has the block-scaled form's bit pattern minus MX_DOWN_BITS: C with and without the pad, every partial sum, the start
key.  The kernel's outputs against the oracle are tests/test_top2_gpu.py and its neighbours."""
import os
import shutil
import subprocess


def test_scaled_down_keys_keep_their_bit_patterns(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "top2_down")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I" + os.path.join(root, "orb_slam3_comments_ghr_amd", "csrc"),
                        os.path.join(root, "tests", "host", "top2_down.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr and r.stdout.strip() == "ok", (r.stdout[-3000:], r.stderr[-3000:])

"""The chunk ring of k_top2_fp4q2 (csrc/top2_ring.h): tests/host/top2_ring.cpp walks its schedule by barrier epoch
for every nt in 1..8192 (no write before the slot's last reader has passed a barrier, no read before its write
has, the same barrier count for waves with two query tiles, one or none; a two-slot ring must fail), built with
g++ under ASan + UBSan and run as a stand-alone program."""
import os
import shutil
import subprocess


def test_ring_schedule_clean_under_host_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "top2_ring")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I" + os.path.join(root, "orb_slam3_comments_ghr_amd", "csrc"),
                        os.path.join(root, "tests", "host", "top2_ring.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr and r.stdout.strip() == "ok", (r.stdout[-3000:], r.stderr[-3000:])

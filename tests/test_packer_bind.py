"""CPU: osg_packer's pointer binding (csrc/match_common.h) against a pack made with plain add / add_rows / reserve,
under AddressSanitizer and UBSan (tests/host/packer_bind.cpp: host code only, run directly)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bindings_clean_under_host_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "packer_bind")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                        "-I" + os.path.join(ROOT, "orb_slam3_comments_ghr_amd", "csrc"),
                        os.path.join(ROOT, "tests", "host", "packer_bind.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr and r.stdout.strip() == "ok", (r.stdout[-3000:], r.stderr[-3000:])

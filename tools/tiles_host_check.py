"""The host launchers of csrc/ce_tiles.hip under AddressSanitizer and UBSan: builds tools/tiles_host_check.cpp together with ce_tiles.hip as
a stand-alone program (hipcc, the sanitizers on the host side only) and runs it - every rejection the header declares for the three entry
points.  Every such call returns before any HIP call, so nothing is launched; the child is also started with no device visible
(HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES emptied), so it cannot touch one.  The valid path needs a device: tests/test_exact_tiles_gpu.py.
Run after a change to the launchers' argument checks:
    python tools/tiles_host_check.py"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "check")
        subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "chronoedit_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "chronoedit_amd", "csrc", "ce_tiles.hip"), os.path.join(ROOT, "tools", "tiles_host_check.cpp"), "-o", exe],
                       check=True)
        return subprocess.run([exe], env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")).returncode


if __name__ == "__main__":
    sys.exit(main())

"""csrc/ce_gemm_plan.h - the split-K plan of the last round and the encoding of K-segmented operands, the host arithmetic every large-tile
GEMM launcher shares - against brute force, under AddressSanitizer and UBSan: builds tools/gemm_plan_host_check.cpp as a stand-alone program
(no GPU, no HIP) and runs it.  Run before a change to the plan, a bound or a tile geometry goes to a device:
    python tools/gemm_plan_host_check.py"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "check")
        cxx = os.environ.get("CXX", "g++")
        subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                        os.path.join(ROOT, "chronoedit_amd", "csrc"), os.path.join(ROOT, "tools", "gemm_plan_host_check.cpp"), "-o", exe], check=True)
        return subprocess.run([exe]).returncode


if __name__ == "__main__":
    sys.exit(main())

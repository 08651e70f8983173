"""chronoedit_amd.hiplib.header_signatures() - the argtypes every ctypes call goes through, parsed from the headers - against the C++
compiler's reading of the same headers, type by type for every entry point: builds tools/abi_host_check.cpp as a stand-alone program
(no GPU, no HIP, nothing linked or loaded) and compares its output.  Run after a change to a header or to the parser:
    python tools/abi_host_check.py"""
import ctypes
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from chronoedit_amd import hiplib  # noqa: E402

CODES = {ctypes.c_int: "i", ctypes.c_float: "f", ctypes.c_longlong: "q", ctypes.c_size_t: "z", ctypes.c_char_p: "s",
         ctypes.POINTER(ctypes.c_void_p): "A", ctypes.c_void_p: "P"}


def main():
    names = hiplib.header_symbols() + hiplib.header_symbols(diag=True)
    sigs = dict(hiplib.header_signatures(), **hiplib.header_signatures(diag=True))
    want = [" ".join([n] + [CODES.get(t, "?") for t in sigs[n]]) for n in names]
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "abi_names.inc"), "w") as f:
            f.write("".join(f"X({n})\n" for n in names))
        exe = os.path.join(tmp, "check")
        subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", tmp,
                        os.path.join(ROOT, "tools", "abi_host_check.cpp"), "-o", exe], check=True)
        got = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    bad = [f"compiler: {g!r}  parser: {w!r}" for g, w in zip(got, want) if g != w or "?" in g]
    n = len(hiplib.SIGNATURES) + len(hiplib.DIAG_SIGNATURES)
    if bad or not len(got) == len(want) == n:
        print("\n".join(bad + [f"{len(got)} entry points compiled, {len(want)} parsed, {n} bound: MISMATCH"]))
        return 1
    print(f"{n} entry points: OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())

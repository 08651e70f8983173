"""The lane functions of csrc/ce_components_core.h on the host, under AddressSanitizer and UBSan, against `components.reference`: builds
tools/components_host_check.cpp as a stand-alone program (no GPU, no HIP), feeds it the adversarial planes of tests/components_shapes.py at
sizes around the tile and compares the labels bit for bit.  Run before a change to the labelling goes to a device:
    python tools/components_host_check.py"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import components_shapes as S  # noqa: E402

from chronoedit_amd import components  # noqa: E402


def planes():
    th, tw = components.TILE
    sizes = [(1, 1), (1, 70), (70, 1), (th - 1, tw - 1), (th, tw), (th + 1, tw + 1), (2 * th, 2 * tw), (2 * th + 5, 2 * tw + 7), (3 * th + 1, 3 * tw + 13),
             (37, 201)]
    for H, W in sizes:
        for name, p in S.adversarial(H, W).items():
            yield f"{name} {H}x{W}", p
        yield f"last tile {H}x{W}", S.root_in_last_tile(H, W, th, tw)
    yield "noise 300x500", S.noise(300, 500, 0.4, 3)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        exe, fin, fout = (os.path.join(tmp, n) for n in ("check", "in.bin", "out.bin"))
        cxx = os.environ.get("CXX", "g++")
        subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                        os.path.join(ROOT, "chronoedit_amd", "csrc"), os.path.join(ROOT, "tools", "components_host_check.cpp"), "-o", exe], check=True)
        cases = list(planes())
        with open(fin, "wb") as f:
            for _, p in cases:
                f.write(np.array(p.shape, np.int32).tobytes() + p.tobytes())
        subprocess.run([exe, fin, fout], check=True)
        got = np.fromfile(fout, np.int32)
    at, bad = 0, 0
    for name, p in cases:
        want = components.roots(torch.from_numpy(p)).numpy()
        g = got[at:at + p.size].reshape(p.shape)
        at += p.size
        if not np.array_equal(g, want):
            bad += 1
            print("MISMATCH", name, int((g != want).sum()), "labels")
    assert at == got.size
    print(f"{len(cases)} planes, {bad} mismatches")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

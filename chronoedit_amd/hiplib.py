"""Build + load libchronoedit_hip.so (the C-ABI HIP library) through ctypes.

The library is built in-tree (``chronoedit_amd/lib/``) with ``hipcc --offload-arch=gfx950`` so that
it travels with the source tree; nothing is JIT-compiled at run time.  Loading fails loudly when
the library is missing or its exported entry points are not exactly those of include/chronoedit_hip.h.
"""
from __future__ import annotations

import ctypes
import os
import re
import subprocess
from typing import Dict, List

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)
CSRC = os.path.join(PKG_DIR, "csrc")
LIB_DIR = os.path.join(PKG_DIR, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libchronoedit_hip.so")            # the product library: exports exactly include/chronoedit_hip.h
DIAG_LIB_PATH = os.path.join(LIB_DIR, "libchronoedit_hip_diag.so")  # same sources + -DCE_DIAGNOSTICS: also exports chronoedit_hip_diag.h
OBJ_DIR = os.path.join(LIB_DIR, "obj")
HEADER = os.path.join(ROOT, "include", "chronoedit_hip.h")
DIAG_HEADER = os.path.join(ROOT, "include", "chronoedit_hip_diag.h")

# translation units that hold a kernel-body selector (csrc/ce_common.h CE_KNOB): the only ones compiled twice
DIAG_SOURCES = ["ce_gemm.hip", "ce_gemm256.hip", "ce_attn.hip", "ce_attn_fp8.hip", "ce_gemm_fp8.hip", "ce_gemm_fp8w4.hip"]
# measured-and-closed experiments kept as opt-in bodies: in the diagnostic library only
DIAG_ONLY_SOURCES = ["ce_attn16.hip"]
SOURCES = ["ce_rowops.hip", "ce_gemm.hip", "ce_gemm256.hip", "ce_gemm256w4.hip", "ce_gemm384.hip", "ce_attn.hip", "ce_attn16.hip", "ce_attn_fp8.hip", "ce_sched.hip", "ce_conv.hip", "ce_enc.hip", "ce_gemm_fp8.hip", "ce_gemm_fp8w4.hip", "ce_comm.hip", "ce_lora.hip", "ce_tea.hip", "ce_image.hip", "ce_region.hip", "ce_sparse.hip", "ce_region_auto.hip", "ce_focus.hip", "ce_autofocus.hip", "ce_preview.hip", "ce_lift.hip", "ce_sketch.hip", "ce_components.hip", "ce_clusters.hip", "ce_layers.hip", "ce_boxlift.hip", "ce_rimlift.hip", "ce_tiles.hip"]

_c = ctypes
# scalar parameter types of the C ABI; every pointer is passed as an address (see _ctype)
_SCALARS = {"int": _c.c_int, "float": _c.c_float, "long long": _c.c_longlong, "size_t": _c.c_size_t, "hipStream_t": _c.c_void_p}


def _header_text(diag: bool, text: str = None) -> str:
    return open(DIAG_HEADER if diag else HEADER).read() if text is None else text


def header_symbols(diag: bool = False, text: str = None) -> List[str]:
    """Every function declared in include/chronoedit_hip.h (diag: in include/chronoedit_hip_diag.h; text: in that header text instead)."""
    return re.findall(r"^int (ce_\w+)\(", _header_text(diag, text), flags=re.M)


def _ctype(sym: str, param: str):
    """The ctypes type of one parameter declaration: the text up to the parameter's name, looked up - never guessed."""
    m = re.fullmatch(r"(.*?)\w+", param.strip(), flags=re.S)
    ctype = re.sub(r"\s*\*\s*", "*", " ".join(m.group(1).split())) if m else ""
    if ctype in _SCALARS:
        return _SCALARS[ctype]
    if ctype == "const char*":
        return _c.c_char_p
    if ctype == "void**":                     # a handle the callee writes (ce_comm_init)
        return _c.POINTER(_c.c_void_p)
    if ctype.endswith("*"):                   # device pointers and host arrays of them: an address
        return _c.c_void_p
    raise ValueError(f"{sym}: no ctypes type for parameter {param.strip()!r}")


def header_signatures(diag: bool = False, text: str = None) -> Dict[str, List]:
    """symbol -> argtypes (restype is always int) of every prototype of the header, in header order: the one signature table, parsed from the
    ABI's own definition.  Raises on a parameter type it does not know and on a declaration header_symbols() sees whose prototype it cannot
    read (a parameter list that holds a `)`, say) - a wrong argtype does not fail at the call, it shifts the arguments the kernel reads."""
    txt = _header_text(diag, text)
    code = re.sub(r"/\*.*?\*/|//[^\n]*", " ", txt, flags=re.S)
    protos = re.findall(r"^int (ce_\w+)\(([^)]*)\);", code, flags=re.M | re.S)
    declared = header_symbols(diag, txt)
    if [sym for sym, _ in protos] != declared:
        unread = [re.search(r"^int %s\([^;]*" % s, txt, flags=re.M).group(0) for s in declared if s not in dict(protos)]
        raise ValueError(f"{len(protos)} prototypes read where {len(declared)} are declared; not read: {unread}")
    return {sym: [_ctype(sym, p) for p in ([] if params.strip() in ("", "void") else params.split(","))] for sym, params in protos}


SIGNATURES: Dict[str, List] = header_signatures()
# the selectors only libchronoedit_hip_diag.so exports (include/chronoedit_hip_diag.h)
DIAG_SIGNATURES: Dict[str, List] = header_signatures(diag=True)


def bind(lib: ctypes.CDLL, diag: bool = False) -> ctypes.CDLL:
    """Set argtypes / restype on every declared entry point `lib` has (diag: the selectors too) and return `lib`.  An entry point the library
    lacks - an A/B build from before it existed - is skipped.  Only correct for a build of THIS header: nothing here can tell that an
    older build takes other arguments under the same name, and such a build is then called with shifted arguments."""
    for name, argtypes in dict(SIGNATURES, **(DIAG_SIGNATURES if diag else {})).items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.argtypes = argtypes
            fn.restype = _c.c_int
    return lib


def exported_symbols(path: str) -> List[str]:
    """The dynamic symbols a built library defines (`nm -D --defined-only`): tests compare them with the headers."""
    nm = "/opt/rocm/lib/llvm/bin/llvm-nm" if os.path.exists("/opt/rocm/lib/llvm/bin/llvm-nm") else "nm"
    out = subprocess.run([nm, "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-2] in ("T", "t", "W", "D", "B"))


HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden"]


def build(force: bool = False, verbose: bool = False, jobs: int = 0) -> str:
    """hipcc --offload-arch=gfx950 every csrc/*.hip into lib/libchronoedit_hip.so and - the translation units that hold a kernel-body
    selector compiled a second time with -DCE_DIAGNOSTICS - lib/libchronoedit_hip_diag.so (cross-compiles without a GPU).  One object
    per translation unit under lib/obj/, compiled in parallel, rebuilt when its source or any header is newer.  Always writes the in-tree
    paths (CE_HIPLIB_PATH only redirects load())."""
    import glob
    from concurrent.futures import ThreadPoolExecutor
    srcs = [s for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]
    hdrs = sorted(glob.glob(os.path.join(CSRC, "*.h"))) + [HEADER, DIAG_HEADER]
    hdr_m = max(os.path.getmtime(d) for d in hdrs)
    os.makedirs(OBJ_DIR, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    todo, objs, diag_objs = [], [], []
    for s_ in srcs:
        src, stem = os.path.join(CSRC, s_), s_[:-4]
        variants = [("", [])] + ([(".diag", ["-DCE_DIAGNOSTICS"])] if s_ in DIAG_SOURCES else [])
        for tag, defs in variants:
            obj = os.path.join(OBJ_DIR, stem + tag + ".o")
            if force or not os.path.exists(obj) or os.path.getmtime(obj) < max(os.path.getmtime(src), hdr_m):
                todo.append([hipcc, *HIPCC_FLAGS, *defs, "-I", CSRC, "-c", src, "-o", obj])
            if tag or s_ in DIAG_ONLY_SOURCES:
                diag_objs.append(obj)
            else:
                objs.append(obj)
        if s_ not in DIAG_SOURCES and s_ not in DIAG_ONLY_SOURCES:
            diag_objs.append(os.path.join(OBJ_DIR, stem + ".o"))

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)

    if todo:
        with ThreadPoolExecutor(max_workers=jobs or min(8, os.cpu_count() or 4)) as ex:
            list(ex.map(run, todo))
    # the dynamic symbol table is the header, nothing else: a linker version script generated FROM the header(s) keeps the toolchain's own
    # globals (__hip_cuid_*, kernel host stubs) out of it (tests/test_host_cpu.py compares `nm -D` with the headers)
    for path, group, diag in ((LIB_PATH, objs, False), (DIAG_LIB_PATH, diag_objs, True)):
        if force or todo or not os.path.exists(path) or os.path.getmtime(path) < max([hdr_m] + [os.path.getmtime(o) for o in group]):
            vs = os.path.join(OBJ_DIR, "exports_diag.map" if diag else "exports.map")
            names = header_symbols() + (header_symbols(diag=True) if diag else [])
            with open(vs, "w") as f:
                f.write("{\n  global:\n" + "".join(f"    {n};\n" for n in names) + "  local: *;\n};\n")
            run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *group, "-ldl", f"-Wl,--version-script={vs}", "-o", path])
    return LIB_PATH


_LIB = None
_DIAG = None


def _open(path: str, diag: bool) -> ctypes.CDLL:
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: the HIP extension is the only compute path of chronoedit_amd "
            "(no CPU/eager fallback). Build it with `python -c 'import __graft_entry__ as g; g.build()'`."
        )
    # ONE HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 and must be the first to load it - our library's
    # DT_NEEDED then resolves to that copy.  Loaded the other way round (this library before `import torch`) the process holds
    # two runtimes, and a kernel launched through one on a stream of the other fails with hipErrorNoDevice (100).
    import torch  # noqa: F401
    # exactly the header's entry points: a build of another ABI (e.g. a stale one loaded through CE_HIPLIB_PATH) may export the same names
    # with other argument lists, and would be called with shifted arguments.  (The selectors of a diagnostic build are no other ABI: load()
    # refuses that build as the product unless asked for it.)
    declared, selectors = set(header_symbols()), set(header_symbols(diag=True))
    if diag:
        declared |= selectors
    exported = {s for s in exported_symbols(path) if s.startswith("ce_")}
    missing, unknown = declared - exported, exported - declared - selectors
    if missing or unknown:
        raise RuntimeError(f"{path} does not match include/chronoedit_hip{'_diag' if diag else ''}.h: missing {sorted(missing)}, "
                           f"not declared {sorted(unknown)}")
    return bind(ctypes.CDLL(path), diag)


def load() -> ctypes.CDLL:
    """The product library.  CE_HIPLIB_PATH (A/B tooling: tools/sessions_r05/gpu_r5_l.sh runs the same bench against two BUILDS) redirects the
    load - with a warning - and never the build; a build whose ce_build_info() says F8_ABLATE != 0 (results are garbage) or that is the
    diagnostic build is refused unless CE_HIPLIB_ALLOW_DIAGNOSTIC_BUILD=1 says the caller knows."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = LIB_PATH
    override = os.environ.get("CE_HIPLIB_PATH")
    if override:
        import warnings
        warnings.warn(f"CE_HIPLIB_PATH is set: loading {override} instead of the in-tree build {LIB_PATH}", RuntimeWarning, stacklevel=2)
        path = override
    lib = _open(path, diag=False)
    info = lib.ce_build_info()
    if (info & 1 or (info >> 8) & 255) and os.environ.get("CE_HIPLIB_ALLOW_DIAGNOSTIC_BUILD") != "1":
        raise RuntimeError(f"{path}: ce_build_info() = {info:#x} - " + ("a timing-only F8_ABLATE build whose results are garbage" if (info >> 8) & 255
                           else "the diagnostic build") + "; refusing to use it as the product library (CE_HIPLIB_ALLOW_DIAGNOSTIC_BUILD=1 overrides)")
    _LIB = lib
    return lib


def load_diagnostics() -> ctypes.CDLL:
    """libchronoedit_hip_diag.so: the product ABI plus the kernel-body selectors (tools/, body-equivalence tests; never the product path)."""
    global _DIAG
    if _DIAG is None:
        _DIAG = _open(DIAG_LIB_PATH, diag=True)
        if not _DIAG.ce_build_info() & 1:
            raise RuntimeError(f"{DIAG_LIB_PATH} was not compiled with -DCE_DIAGNOSTICS")
    return _DIAG

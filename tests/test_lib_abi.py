"""CPU-side checks of the drop-in boundary: the C-ABI library builds for gfx950, loads, and exports
every symbol include/etch_hip.h declares.  No compute call is made (no GPU here)."""
import os

from etch_amd import _lib
from etch_amd import build as B


def test_library_builds_and_exports_header_symbols():
    lib_path = B.build()
    assert os.path.exists(lib_path)
    names = _lib.declared_symbols()
    assert len(names) >= 5 and "etch_ball_query" in names
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib, n), n


def test_product_has_no_cpu_fallback():
    import pytest
    import torch

    from etch_amd import ops

    with pytest.raises(_lib.EtchHipError):
        ops.ball_query(torch.zeros(1, 3, 4), torch.zeros(1, 3, 8), 0.1, 4)


def test_product_never_imports_oracle():
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "etch_amd")
    for dp, _, fs in os.walk(root):
        for f in fs:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dp, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt, os.path.join(dp, f)


def _norm(proto):
    import re
    proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
    return re.sub(r"\s+", " ", proto.replace("*", " * ")).replace(" ;", ";").strip()


REFERENCE_LAUNCHERS = {
    # external/pointops/src/knnquery/knnquery_cuda_kernel.h:14
    "knnquery_cuda_launcher": "void knnquery_cuda_launcher(int m, int nsample, const float *xyz, const float *new_xyz, const int *offset, "
                              "const int *new_offset, int *idx, float *dist2);",
    # external/pointops/src/sampling/sampling_cuda_kernel.h:14
    "furthestsampling_cuda_launcher": "void furthestsampling_cuda_launcher(int b, int n, const float *xyz, const int *offset, "
                                      "const int *new_offset, float *tmp, int *idx);",
}


def test_reference_launcher_symbols_and_prototypes():
    """The reference's own extern "C" launchers are exported under their names with their exact prototypes (so knnquery_cuda.cpp /
    sampling_cuda.cpp link against libetch_hip.so unchanged).  The reference headers' prototypes are stored above (REFERENCE_LAUNCHERS,
    with the header lines they come from)."""
    import re
    B.build()
    names = _lib.declared_launchers()
    assert set(REFERENCE_LAUNCHERS) <= set(names) and len(names) == 6, names
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib, n), n
    hdr = open(_lib.HEADER).read()
    for name, proto in REFERENCE_LAUNCHERS.items():
        mine = re.search(r"void\s+" + name + r"\s*\([^)]*\)\s*;", hdr).group(0)
        assert _norm(mine) == _norm(proto), (mine, proto)
    assert "etch_knnquery_dev" in _lib.declared_symbols()


# ---- the header is the one description of the C ABI: parse, symbol sets, includes, the call helper ----------------------------------------
NAME_PATTERNS = (r"\bint\s+etch_\w+\(", r"\bvoid\s+\w+_launcher\(",
                 r"\blong\s+etch_\w+\(")           # the one size that does not fit an int: etch_smpl_lm_split_workspace_bytes


def test_parse_finds_every_prototype_and_maps_every_type():
    import ctypes
    import re

    import pytest
    protos = _lib.prototypes()
    txt = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    assert len(protos) == sum(len(re.findall(p, txt)) for p in NAME_PATTERNS)
    assert len(re.findall(NAME_PATTERNS[2], txt)) == 1
    known = set(_lib.CTYPES.values())
    for name, (ret, params) in protos.items():
        assert ret in (None, ctypes.c_int, ctypes.c_long), name
        assert (ret is None) == name.endswith("_launcher"), name
        for ctype, pname in params:
            assert ctype in known and ctype is not None and pname.isidentifier(), (name, pname)
    assert sorted(n for n in protos if n.startswith("etch_")) == _lib.declared_symbols()
    assert sorted(n for n in protos if n.endswith("_launcher")) == _lib.declared_launchers()
    assert len(protos) >= 150
    ret, params = _lib.prototypes()["etch_linear"]
    assert ret is ctypes.c_int and len(params) == 21 and params[4] == (ctypes.c_long, "ldx") and params[-1] == (ctypes.c_void_p, "stream")
    assert _lib.prototypes()["etch_smpl_lm_split_workspace_bytes"][0] is ctypes.c_long
    assert _lib.prototypes()["etch_pt_attention"][1][9] == (ctypes.c_void_p, "params")          # const float* const*
    with pytest.raises(_lib.EtchHipError, match="`x` of etch_f.*`short`"):
        _lib.prototypes(text="int etch_f(int a, short x, void* stream);")


def _exported(path):
    """The etch_* / *_launcher functions `path` exports, by llvm-nm of the toolchain hipcc comes from, else nm -D."""
    import re
    import shutil
    import subprocess
    cc = shutil.which(B.hipcc()) or B.hipcc()
    root = os.path.dirname(os.path.dirname(os.path.realpath(cc)))
    tools = [os.path.join(root, *d, "llvm-nm") for d in (("lib", "llvm", "bin"), ("llvm", "bin"), ("bin",))] + [shutil.which("llvm-nm"), shutil.which("nm")]
    nm = next(t for t in tools if t and os.path.exists(t))
    out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {m.group(1) for m in re.finditer(r"\sT\s+(etch_\w+|\w+_launcher)\s*$", out, flags=re.M)}


def test_header_and_libraries_agree_on_the_symbol_set():
    path = B.build()
    assert _exported(path) == set(_lib.prototypes()), path


def test_every_kernel_source_includes_the_header():
    import re
    names = set(_lib.prototypes())
    csrc = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
    exporting = 0
    for f in sorted(os.listdir(csrc)):
        if not f.endswith(".hip"):
            continue
        txt = open(os.path.join(csrc, f)).read()
        if any(n in names for n in re.findall(r"\b(?:int|long|void)\s+(\w+)\s*\([^;{}]*\)\s*\{", txt)):
            exporting += 1
            assert re.search(r'^#include "etch_hip.h"', txt, flags=re.M), f
    assert exporting >= 20


def test_every_called_name_is_declared_in_the_header():
    """Every literal name the package passes to _lib.call() is a function the library has (declared in include/etch_hip.h): no call of a
    retired symbol survives on a path no GPU test reaches."""
    import re
    root = os.path.dirname(os.path.abspath(_lib.__file__))
    declared = set(_lib.prototypes())
    called = {}
    for dp, _, fs in os.walk(root):
        for f in fs:
            if f.endswith(".py"):
                for n in re.findall(r"\bcall\(\s*\"(etch_\w+)\"", open(os.path.join(dp, f)).read()):
                    called.setdefault(n, os.path.join(dp, f))
    assert len(called) >= 100, len(called)                 # the pattern still finds the package's calls
    assert {n for n in called if n not in declared} == set()


def test_no_hand_written_prototypes_or_pointer_helpers_in_the_package():
    import re
    root = os.path.dirname(os.path.abspath(_lib.__file__))
    for dp, _, fs in os.walk(root):
        for f in fs:
            if not f.endswith(".py"):
                continue
            txt = open(os.path.join(dp, f)).read()
            if f != "_lib.py":
                assert not re.search(r"\.(restype|argtypes)\b", txt), f
            assert not re.search(r"(?<!def )\b(_ptr|_optptr|_c_float|_c_long)\(|\bdef _check\(status", txt), f     # (ops._ptr stays for direct callers only)


class _Entered(Exception):
    pass


def test_call_helper_rejects_bad_calls_before_the_c_function():
    import pytest
    B.build()
    name = "etch_fps_split_workspace_bytes"
    assert _lib.call(name, 3, 4) == 1600                      # index_ops.hip: 64 + nseg * 2 * G * 64
    lib = _lib.lib()
    entered = []

    def hook(sym, args, fn):
        entered.append((sym, args))
        return fn(*args)

    lib.profiler = hook
    try:
        for bad in ((3,), (3, 4, 5)):
            with pytest.raises(_lib.EtchHipError, match=name + " takes 2 arguments"):
                _lib.call(name, *bad)
        assert entered == []                                  # a wrong count never reaches the hook, let alone the C function
        with pytest.raises(_lib.EtchHipError, match=name + ".*argument 1"):
            _lib.call(name, 3.0, 4)                           # ctypes converts every argument before it enters the function
        assert entered == [(name, (3.0, 4))]
    finally:
        lib.profiler = None
    with pytest.raises(_lib.EtchHipError, match=name + ".*argument 1"):
        _lib.call(name, 3.0, 4)
    with pytest.raises(_lib.EtchHipError, match="not declared"):
        _lib.call("etch_no_such_function", 1)
    with pytest.raises(_lib.EtchHipError, match="etch_smpl_lm_split_workspace_bytes failed: unsupported size") as e:
        _lib.call("etch_smpl_lm_split_workspace_bytes", 1, 3, 3, 2)      # no such body model: a host-only function's negative value is its error
    assert e.value.status == -2


def test_profiler_hook_sees_the_call():
    B.build()
    lib = _lib.lib()
    seen = []

    def hook(sym, args, fn):
        seen.append((sym, args, fn))
        return fn(*args)

    lib.profiler = hook
    try:
        assert _lib.call("etch_fps_split_workspace_bytes", 3, 4) == 1600
    finally:
        lib.profiler = None
    (sym, args, fn), = seen
    assert (sym, args) == ("etch_fps_split_workspace_bytes", (3, 4)) and fn(*args) == 1600
    assert lib.etch_fps_split_workspace_bytes(3, 4) == 1600                  # plain attribute access stays

"""ctypes loader of libetch_hip.so.  The product path has NO fallback: if the HIP library is
missing or a symbol is absent this raises, loudly.

include/etch_hip.h is the one description of the C ABI: prototypes() parses it, _load() types every exported function from the parse, and
call() is the one way the package calls the library.

The library writes through raw pointers, which torch cannot see, and every cache of the package is keyed on (data_ptr, _version): a wrapper that
lets the library write into a tensor it did not allocate itself calls wrote() on that tensor, after the launch or, where that is simpler, ahead of it."""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ETCH_HIP_LIB") or os.path.join(_HERE, "lib", "libetch_hip.so")   # override: kernel-variant experiments only
HEADER = os.path.join(os.path.dirname(_HERE), "include", "etch_hip.h")
_lib = None


class EtchHipError(RuntimeError):
    status = None             # the C function's return value, when that is what raised


# Every spelling of a return or parameter type in include/etch_hip.h.  Pointers of any kind travel as addresses.
_POINTERS = ("void*", "const void*", "char*", "const char*", "unsigned char*", "int*", "const int*", "unsigned*", "long long*", "const long long*",
             "const unsigned long long*", "float*", "const float*", "double*", "const double*", "const void* const*", "const float* const*", "float* const*")
CTYPES = {"void": None, "int": ctypes.c_int, "long": ctypes.c_long, "long long": ctypes.c_longlong, "unsigned": ctypes.c_uint, "float": ctypes.c_float,
          "double": ctypes.c_double, **{p: ctypes.c_void_p for p in _POINTERS}}

_PROTOTYPE = re.compile(r"\b(void|int|long)\s+(etch_\w+|\w+_launcher)\s*\(([^()]*)\)\s*;")


def _ctype(spelling, where):
    spelling = re.sub(r"\s*\*", "*", " ".join(spelling.split())).replace("*const", "* const")
    if spelling not in CTYPES:
        raise EtchHipError(f"{HEADER}: {where} has the type `{spelling}`, which etch_amd._lib.CTYPES does not map")
    return CTYPES[spelling]


def prototypes(text=None):
    """{name: (return ctype, [(ctype, parameter name), ...])} of every function declared in include/etch_hip.h, in header order."""
    txt = open(HEADER).read() if text is None else text
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for ret, name, params in _PROTOTYPE.findall(txt):
        plist = []
        for p in params.split(","):
            if p.strip() in ("", "void"):
                continue
            spelling, pname = re.fullmatch(r"\s*(.*?)(\w+)\s*", p, flags=re.S).groups()
            plist.append((_ctype(spelling, f"parameter `{pname}` of {name}"), pname))
        out[name] = (_ctype(ret, f"the return value of {name}"), plist)
    return out


def declared_symbols():
    """Every etch_* function declared in include/etch_hip.h."""
    return sorted(n for n in prototypes() if n.startswith("etch_"))


def declared_launchers():
    """The reference's own launcher symbols re-exported with their exact signatures (`void <name>_launcher(...)`)."""
    return sorted(n for n in prototypes() if n.endswith("_launcher"))


class _Proxy:
    """Attribute access -> typed C function.  When a profiler callback is installed (bench.py) every call is
    bracketed by HIP events on the current stream; otherwise the raw ctypes function is returned."""

    def __init__(self, cdll, sigs):
        self._cdll = cdll
        self._sigs = sigs         # name -> (ctypes function, number of parameters, positions of the pointer parameters, last one is `void* stream`)
        self.profiler = None      # callable(name, args, fn) -> status

    def __getattr__(self, name):
        fn = getattr(self._cdll, name)
        if self.profiler is None:
            return fn
        prof = self.profiler
        return lambda *a: prof(name, a, fn)


def _load(path, how):
    if not os.path.exists(path):
        raise EtchHipError(f"{path} is missing: build it with {how} (hipcc, gfx950). etch_amd has no CPU fallback.")
    cdll = ctypes.CDLL(path)
    sigs = {}
    for name, (ret, params) in prototypes().items():
        fn = getattr(cdll, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = ret
        fn.argtypes = [t for t, _ in params]
        pointers = tuple(i for i, (t, _) in enumerate(params) if t is ctypes.c_void_p)
        sigs[name] = (fn, len(params), pointers, bool(params) and params[-1] == (ctypes.c_void_p, "stream"))
    return _Proxy(cdll, sigs)


def lib():
    global _lib
    if _lib is None:
        _lib = _load(LIB_PATH, "`python -m etch_amd.build`")
    return _lib


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream():
    """The current HIP stream's handle.  Asked ~300 times per step: torch.cuda.current_stream() builds a Stream object (10 us each, 3 ms of the host's
    8.5 ms per step); the raw accessor returns the integer."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


_Tensor = torch.Tensor


def call(name, *args):
    """Call the function `name` of include/etch_hip.h with `args` in header order.  At a pointer parameter a tensor stands for its data pointer and None
    for NULL; a prototype that ends in `void* stream` gets the current stream unless the caller passes one.  The tensors stay referenced until the C call
    has returned, so a temporary (`x.contiguous()`) is passed as it is.  Raises EtchHipError before the call on a wrong number of arguments and after it
    on a failed status; a host-only function (no stream) returns its count or size (negative: the same error)."""
    L = lib()
    try:
        fn, nparams, pointers, streamed = L._sigs[name]
    except KeyError:
        raise EtchHipError(f"{name} is not declared in include/etch_hip.h") from None
    raw = list(args)
    if streamed and len(raw) == nparams - 1:
        raw.append(stream())
    if len(raw) != nparams:
        raise EtchHipError(f"{name} takes {nparams} arguments{' (the last one, the stream, optional)' if streamed else ''}, got {len(args)}")
    for i in pointers:
        a = raw[i]
        if a is not None and isinstance(a, _Tensor):
            raw[i] = a.data_ptr()
    prof = L.profiler
    try:
        status = fn(*raw) if prof is None else prof(name, tuple(raw), fn)
    except ctypes.ArgumentError as e:
        raise EtchHipError(f"{name}: {e}") from None
    if status and (streamed or status < 0):
        check(status, name)
    return status


def wrote(*tensors):
    """Announce a write through raw pointers: bumps `_version` of every tensor given (None is skipped), as an in-place torch op would have."""
    torch.autograd.graph.increment_version([t for t in tensors if t is not None])


def check(status, what):
    """The one status check: call() applies it; direct callers of a typed function (tests, profiles/scripts) apply it to what that returned."""
    if status != 0:
        kind = {-1: "invalid argument", -2: "unsupported size"}.get(status, f"hipError {status}")
        err = EtchHipError(f"{what} failed: {kind}")
        err.status = status
        raise err

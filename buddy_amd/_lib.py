"""ctypes binding of ``libbuddy_hip.so`` (C-ABI in ``include/buddy_hip.h``).

There is NO CPU fallback: importing works anywhere (so configs/host logic can be tested on CPU), but any
compute call raises ``BuddyHipError`` if the shared library is missing or no GPU is visible.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbuddy_hip.so")


class BuddyHipError(RuntimeError):
    pass


_HEADER = os.path.join(os.path.dirname(_HERE), "include", "buddy_hip.h")
_SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "float": C.c_float, "double": C.c_double, "long long": C.c_longlong,
            "unsigned long long": C.c_ulonglong}
_PROTO = re.compile(r"([\w\s*]+?)\b(buddy_\w+)\s*\(([^()]*)\)")


def _ctype(decl, is_param, stmt):
    """one parameter or return type: ``const char*`` is c_char_p, any other pointer or array parameter c_void_p (a raw device / host
    address), a scalar its C type; anything else is refused"""
    if re.fullmatch(r"const\s+char\s*\*\s*\w*", decl):
        return C.c_char_p
    if is_param and ("*" in decl or "[" in decl):
        return C.c_void_p
    if is_param and decl not in _SCALARS:
        decl = re.sub(r"\s+\w+$", "", decl)                # drop the parameter's name
    if decl not in _SCALARS:
        raise BuddyHipError(f"C header: cannot bind `{stmt}`: no ctypes type for `{decl}`")
    return _SCALARS[decl]


def parse_header(text):
    """C header text -> {name: (restype, [argtypes])}.  Strict: once comments, preprocessor lines and the extern "C" braces are gone, EVERY
    statement has to be a prototype ``ret buddy_name(params);`` of types ``_ctype`` knows.  Nothing is skipped and nothing is guessed, so no
    ``buddy_name(`` of the header can be left without an entry."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{|\}', " ", text)
    *stmts, rest = (" ".join(s.split()) for s in text.split(";"))
    if rest:
        raise BuddyHipError(f"C header: cannot bind `{rest[:200]}`: no `;` after it")
    sigs = {}
    for stmt in stmts:
        m = _PROTO.fullmatch(stmt)
        if not m or m.group(2) in sigs:
            raise BuddyHipError(f"C header: cannot bind `{stmt[:200]}`: not one `ret buddy_name(params);` prototype, or declared twice")
        ret, name, params = (g.strip() for g in m.groups())
        sigs[name] = (_ctype(ret, False, stmt), [] if params == "void" else [_ctype(p.strip(), True, stmt) for p in params.split(",")])
    return sigs


try:                                       # once per process: the header is the only place a signature is written down
    with open(_HEADER) as _f:
        _SIGS = parse_header(_f.read())
except OSError as e:
    raise BuddyHipError(f"{_HEADER} not readable ({e.strerror}): the ctypes signatures are derived from it") from None
EXPORTED = sorted(_SIGS)
_lib = None


def load():
    """Load the shared library (no GPU needed for loading / symbol checks)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BuddyHipError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                                "(buddy_amd/csrc/build.sh); there is no CPU fallback")
        import torch  # noqa: F401  -- FIRST: torch ships its own libamdhip64 (same SONAME); loading ours before it would put two
        #                       HIP runtimes in the process ("no ROCm-capable device is detected" from the second one)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
        rc = lib.buddy_options_check()     # a misspelt BUDDY_* switch fails here, loudly, not somewhere inside a launcher
        if rc != 0:
            msg = lib.buddy_last_error().decode()
            _lib = None
            raise BuddyHipError(f"libbuddy_hip: {msg}")
    return _lib


def check(rc):
    if rc != 0:
        raise BuddyHipError(f"libbuddy_hip error {rc}: {load().buddy_last_error().decode()}")


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise BuddyHipError("no HIP device visible: the MI355X path has no CPU fallback")
    return load()


def ptr(t):
    """device pointer of a contiguous float32 CUDA tensor (or None)."""
    if t is None:
        return None
    import torch
    assert t.is_cuda and t.is_contiguous(), "expected a contiguous device tensor"
    assert t.dtype in (torch.float32, torch.float64)
    return t.data_ptr()


def stream_ptr():
    import torch
    return torch.cuda.current_stream().cuda_stream

"""Host: the C ABI is written down once, in include/buddy_hip.h.  The header's prototypes, the ctypes signatures that buddy_amd/_lib.py derives from
it and the symbols libbuddy_hip.so exports are the same set of names; every derived signature is checked against the header by this file's own
regular expressions (not by _lib's parser, which would be circular); and the parser reads the awkward forms and refuses what it cannot classify."""
import ctypes
import os
import re
import subprocess

import pytest

from buddy_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALAR = {"int": "c_int", "unsigned": "c_uint", "float": "c_float", "double": "c_double", "long long": "c_longlong",
          "unsigned long long": "c_ulonglong"}


@pytest.fixture(scope="module")
def header():
    text = open(os.path.join(ROOT, "include", "buddy_hip.h")).read()
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def test_header_signatures_and_exports_are_one_set(header):
    declared = re.findall(r"\b(buddy_[A-Za-z0-9_]+)\s*\(", header)
    assert len(declared) == len(set(declared)) >= 228, sorted(n for n in set(declared) if declared.count(n) > 1)
    assert set(declared) == set(_lib.EXPORTED) == set(_lib._SIGS), set(declared) ^ set(_lib.EXPORTED)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    exported = {s for s in exported if s.startswith("buddy_")}
    assert exported == set(declared), exported ^ set(declared)
    lib = _lib.load()
    for name, (res, args) in _lib._SIGS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def kind(decl):
    """the ctypes type a parameter or return type of the header travels as: pointers and arrays as c_void_p, scalars by their C type"""
    if re.fullmatch(r"const\s+char\s*\*\s*\w*", decl):
        return ctypes.c_char_p
    if "*" in decl or "[" in decl:
        return ctypes.c_void_p
    return getattr(ctypes, SCALAR[decl if decl in SCALAR else re.sub(r"\s+\w+$", "", decl).strip()])


def test_every_signature_matches_its_prototype(header):
    protos = {m.group(2): m for m in re.finditer(r"([\w ]+?[\s*]+)(buddy_\w+)\s*\(([^)]*)\)\s*;", header)}
    assert set(protos) == set(_lib._SIGS)
    for s, (res, args) in _lib._SIGS.items():
        assert res is kind(protos[s].group(1).strip()), s
        params = [" ".join(p.split()) for p in protos[s].group(3).split(",")]
        params = [] if params == ["void"] else params
        assert len(params) == len(args), s
        for p, a in zip(params, args):
            assert a is kind(p), (s, p, a)
    # a few by hand, so that a mistake shared by both sets of expressions shows
    i, ll, d, f, u, p = ctypes.c_int, ctypes.c_longlong, ctypes.c_double, ctypes.c_float, ctypes.c_uint, ctypes.c_void_p
    assert _lib._SIGS["buddy_last_error"] == (ctypes.c_char_p, [])
    assert _lib._SIGS["buddy_optim_sqnorm_chunk"] == (ll, [])
    assert _lib._SIGS["buddy_optim_ema"] == (i, [p, p, ll, d, p])
    assert _lib._SIGS["buddy_perturb_philox"] == (i, [p, p, u, f, p, i, i, p])
    assert _lib._SIGS["buddy_ncsnpp_set_option"] == (i, [p, ctypes.c_char_p, i])
    assert _lib._SIGS["buddy_ncsnpp_tap"] == (i, [p, i, p, p])
    assert _lib._SIGS["buddy_prof_collect"] == (i, [p] * 5)


def test_parser_reads_the_awkward_forms():
    sigs = _lib.parse_header("""
        /* a comment that names buddy_ghost( and int buddy_other(int x); */
        #ifndef H
        #define H
        #ifdef __cplusplus
        extern "C" {
        #endif
        const char* buddy_text(void);   // buddy_line_comment(
        int buddy_collect(double* ms /*[2]*/, long long* launches /*[2]*/,
                          double* executed /*[2]: = flops except, for (some) launches; (4/9)*/);
        int buddy_dims(void* handle, int module_idx, const float** ptr, int dims[4]);
        long long buddy_bytes(int B, long long T, unsigned seed, unsigned long long key, float a, double b, const signed char* e);
        int buddy_key(void* handle, const char* key, int* value);
        #ifdef __cplusplus
        }
        #endif
        #endif
    """)
    i, p = ctypes.c_int, ctypes.c_void_p
    assert sigs == {"buddy_text": (ctypes.c_char_p, []), "buddy_collect": (i, [p, p, p]), "buddy_dims": (i, [p, i, p, p]),
                    "buddy_bytes": (ctypes.c_longlong, [i, ctypes.c_longlong, ctypes.c_uint, ctypes.c_ulonglong, ctypes.c_float, ctypes.c_double, p]),
                    "buddy_key": (i, [p, ctypes.c_char_p, p])}
    assert list(sigs) == ["buddy_text", "buddy_collect", "buddy_dims", "buddy_bytes", "buddy_key"]
    assert _lib.parse_header("") == {}


@pytest.mark.parametrize("text,names", [
    ("int buddy_a(size_t n);", "size_t"),                                          # an unknown scalar type
    ("size_t buddy_a(int n);", "size_t"),
    ("int buddy_a(struct BuddyCfg cfg);", "struct BuddyCfg"),                      # a struct by value
    ("int buddy_a(int n)\nint buddy_b(void);", "buddy_a"),                         # a missing semicolon
    ("int buddy_b(void);\nint buddy_a(int n)\n", "buddy_a"),                       # ... on the last prototype
    ("int buddy_a(int n;\nint buddy_b(void);", "buddy_a"),                         # unbalanced parentheses
    ("int buddy_a(int (*cb)(int), void* ctx);", "buddy_a"),                        # a function pointer
    ("int buddy_a(int n);\nint buddy_a(int n);", "buddy_a"),                       # declared twice
    ("int buddy_a();", "buddy_a"),                                                 # no parameter list
    ("float* buddy_a(int n);", "buddy_a"),                                         # a pointer return other than const char*
    ("typedef int buddy_int;\nint buddy_a(buddy_int n);", "buddy_int"),            # anything that is not a prototype
    ("int other_a(int n);", "other_a"),
])
def test_parser_refuses_what_it_cannot_classify(text, names):
    with pytest.raises(_lib.BuddyHipError) as e:
        _lib.parse_header(text)
    assert names in str(e.value)


def test_missing_header_is_an_error_that_names_the_path(tmp_path):
    """the module's own source, run as if the package lay in a tree without include/"""
    elsewhere = {"__name__": "lib_without_header", "__file__": str(tmp_path / "pkg" / "_lib.py")}
    with pytest.raises(RuntimeError) as e:
        exec(compile(open(_lib.__file__).read(), elsewhere["__file__"], "exec"), elsewhere)
    assert type(e.value).__name__ == "BuddyHipError" and str(tmp_path / "include" / "buddy_hip.h") in str(e.value)

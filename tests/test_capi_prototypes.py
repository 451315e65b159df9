"""CPU suite: the binding takes every prototype from include/mi_slam.h at load (capi._parse_header, capi.lib).  Checked here: every
function is typed before any wrapper has run; the host compiler agrees with the parser's split and with the ctypes type of every argument
and return value of every entry point; the prototypes that exercise the parser's corners equal ones written out by hand; the compiler
agrees with the size and every field offset of every ctypes Structure; a type outside the vocabulary is refused by name."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
V, I, F = C.c_void_p, C.c_int, C.c_float

# written by hand from the header, not from the parser: (restype, argtypes)
PINNED = {
    "mi_pack_key": (C.c_ulonglong, [F, I]),
    "mi_unpack_key": (None, [C.c_ulonglong, V, V]),
    "mi_icp_auto_batch": (I, [C.c_longlong, C.c_longlong, I, I, I]),
    "mi_profile_select": (I, [V, C.c_uint]),
    "mi_nn_kernel_name": (C.c_char_p, [V, I, I, I]),
    "mi_last_error": (C.c_char_p, []),
    "mi_ctx_create_exchange": (I, [I, I, I, "EXCHANGE_FN", V, V]),
    "mi_cluster_dbscan": (I, [V, V, I, V, V, V, V, I, V, V, V]),
    "mi_ndt_system": (I, [V, V, I, V, V, V, I, F, V, V, I, F, V, V, V, V]),
    "mi_ransac_hypotheses": (I, [V, V, I, V, I, V, V, I, I, V, V, V, V]),
    "mi_estimate_covariances": (I, [V, V, I, I, I, F, I, F, V, V]),
    "mi_icp_result": (I, [V, V, V, V, V]),
    "mi_voxel_index": (I, [V, V, F, V]),
    "mi_selftest_cpd_last": (I, [V, I, I] + [V] * 13),
}


def _compile(tmp_path, name, text):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / (name + ".cpp")
    src.write_text(text)
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", INCLUDE, "-fsyntax-only", str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-6000:]


def test_every_function_is_typed_before_first_use():
    """A fresh process: import, lib(), and nothing else -- then every header name carries the header's argument count and return type."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import __graft_entry__ as g\n"
            "capi = g.load_package().capi\n"
            "lib = capi.lib()\n"
            "assert len(capi.EXPORTS) >= 100 and len(set(capi.EXPORTS)) == len(capi.EXPORTS)\n"
            "for name, ret, args, restype, argtypes in capi._PROTOTYPES:\n"
            "    f = lib.__dict__[name]                   # already an attribute: lib() made it, not this lookup\n"
            "    assert f.argtypes is not None and list(f.argtypes) == argtypes and len(argtypes) == len(args), name\n"
            "    assert f.restype is restype, name\n"
            "print('typed', len(capi._PROTOTYPES))\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "typed" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_the_compiler_agrees_with_every_parsed_prototype(capi, tmp_path):
    """One C++ file from the parsed table: &mi_x converts to a pointer type written from the parsed texts, and the type the HEADER declares for
    every slot has the size, pointer-ness, floating-point-ness and signedness of the slot's ctypes type."""
    out = ['#include <cstddef>', '#include <tuple>', '#include <type_traits>', '#include "mi_slam.h"',
           'template <class T> struct sig;',
           'template <class R, class... A> struct sig<R (*)(A...)> {',
           '    using ret = R; static constexpr std::size_t n = sizeof...(A);',
           '    template <std::size_t i> using arg = std::tuple_element_t<i, std::tuple<A...>>; };',
           'template <class T> constexpr bool is_signed_int = std::is_integral<T>::value && std::is_signed<T>::value;',
           'template <class T> constexpr bool is_unsigned_int = std::is_integral<T>::value && std::is_unsigned<T>::value;']
    assert len(capi._PROTOTYPES) == len(capi.EXPORTS) >= 100

    def slot(name, what, T, ct):
        if ct is None:
            return ['static_assert(std::is_void<%s>::value, "%s %s");' % (T, name, what)]
        pointer = ct in (C.c_void_p, C.c_char_p, capi.EXCHANGE_FN)
        integer = ct in (C.c_int, C.c_uint, C.c_longlong, C.c_ulonglong)
        assert pointer or integer or ct is C.c_float, (name, what, ct)
        signed = ct in (C.c_int, C.c_longlong)
        return ['static_assert(sizeof(%s) == %d, "%s %s: size");' % (T, C.sizeof(ct), name, what),
                'static_assert(std::is_pointer<%s>::value == %s, "%s %s: pointer");' % (T, str(pointer).lower(), name, what),
                'static_assert(std::is_floating_point<%s>::value == %s, "%s %s: float");' % (T, str(ct is C.c_float).lower(), name, what),
                'static_assert(is_signed_int<%s> == %s, "%s %s: signed");' % (T, str(integer and signed).lower(), name, what),
                'static_assert(is_unsigned_int<%s> == %s, "%s %s: unsigned");' % (T, str(integer and not signed).lower(), name, what)]

    for name, ret, args, restype, argtypes in capi._PROTOTYPES:
        S = "sig<decltype(&%s)>" % name
        out.append('%s (*p_%s)(%s) = &%s;' % (ret, name, ", ".join(args) or "void", name))
        out.append('static_assert(%s::n == %d, "%s: argument count");' % (S, len(argtypes), name))
        out += slot(name, "return", "%s::ret" % S, restype)
        for i, ct in enumerate(argtypes):
            out += slot(name, "argument %d" % i, "%s::arg<%d>" % (S, i), ct)
    out.append("int main() { return 0; }")
    _compile(tmp_path, "prototypes", "\n".join(out) + "\n")


def test_corner_prototypes_equal_the_hand_written_ones(capi):
    lib = capi.lib()
    for name, (restype, argtypes) in PINNED.items():
        f = getattr(lib, name)
        assert f.restype is restype, name
        assert list(f.argtypes) == [capi.EXCHANGE_FN if a == "EXCHANGE_FN" else a for a in argtypes], name


def test_the_compiler_agrees_with_every_structure_layout(capi, tmp_path):
    classes = [v for v in vars(capi).values() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure]
    assert len(classes) == 13 and set(classes) == set(capi._C_TYPES)           # each class names its C type once
    assert len(set(capi._C_TYPES.values())) == 13
    out = ['#include <cstddef>', '#include "mi_slam.h"']
    for cls, ctype in capi._C_TYPES.items():
        out.append('static_assert(sizeof(%s) == %d, "%s: size");' % (ctype, C.sizeof(cls), ctype))
        assert cls._fields_
        for field, ftype in cls._fields_:
            out.append('static_assert(offsetof(%s, %s) == %d, "%s.%s: offset");' % (ctype, field, getattr(cls, field).offset, ctype, field))
            out.append('static_assert(sizeof(%s::%s) == %d, "%s.%s: size");' % (ctype, field, C.sizeof(ftype), ctype, field))
    out.append("int main() { return 0; }")
    _compile(tmp_path, "layouts", "\n".join(out) + "\n")


def test_a_type_outside_the_vocabulary_is_refused_by_name(capi):
    text = open(os.path.join(INCLUDE, "mi_slam.h")).read()
    assert [p[0] for p in capi._parse_header(text)] == capi.EXPORTS
    for old, new in (("unsigned long long mi_pack_key(float d2, int global_index);", "unsigned long long mi_pack_key(double d2, int global_index);"),
                     ("unsigned long long mi_pack_key(float d2, int global_index);", "double mi_pack_key(float d2, int global_index);"),
                     ("int mi_abi_version(void);", "int mi_abi_version(int (*callback)(void));")):
        assert text.count(old) == 1
        with pytest.raises(capi.MiSlamError, match=new.split("(")[0].split()[-1]):
            capi._parse_header(text.replace(old, new))

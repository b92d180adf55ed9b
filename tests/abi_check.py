"""The ctypes binding (dagnn_amd/_lib.py) against include/dagnn_hip.h, checked by the compiler: `source()` writes one C++17 file
of static_asserts - sizeof / offsetof / type of every struct field (nested members and arrays of structs walked), decltype(&dagnn_x)
of every entry point, DAGNN_X of every constant - and `check()` has hipcc parse it host-only (-fsyntax-only: no device pass, no GPU,
nothing left in the tree).  Each message names the struct and field, the symbol and argument, or the constant."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

from dagnn_amd import _lib
from dagnn_amd import build as _build

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dagnn_hip.h")
# ctypes' type codes -> the C type they bind (c_int32 is c_int, c_int64 is c_long and c_size_t is c_ulong here, as in <stdint.h>)
SCALARS = {"i": "int", "I": "unsigned int", "l": "long", "L": "unsigned long", "f": "float", "d": "double", "z": "const char*"}
PRELUDE = """#include <cstddef>
#include <type_traits>
#include <utility>
#include "%s"
template <class T> using pointee = std::remove_cv_t<std::remove_pointer_t<T>>;
template <class T> constexpr bool object_pointer = std::is_pointer_v<T> && !std::is_function_v<std::remove_pointer_t<T>>;
template <size_t i, class... A> struct nth { using type = struct missing_argument; };
template <class H, class... T> struct nth<0, H, T...> { using type = H; };
template <size_t i, class H, class... T> struct nth<i, H, T...> : nth<i - 1, T...> {};
template <class F> struct sig;
template <class R, class... A> struct sig<R (*)(A...)> {
    using ret = R;
    static constexpr size_t arity = sizeof...(A);
    template <size_t i> using arg = typename nth<i, A...>::type;
};
#define MEMBER(T, path) std::remove_cv_t<std::remove_reference_t<decltype(std::declval<T&>().path)>>
""" % HEADER


def mirrors():
    """Every ctypes.Structure subclass _lib defines."""
    return [c for _, c in inspect.getmembers(_lib, inspect.isclass) if issubclass(c, C.Structure) and c.__module__ == _lib.__name__]


def header_structs():
    """The name of every struct typedef of the header (closed on a line of its own, or written on one line)."""
    return re.findall(r"^(?:typedef struct\b.*)?\}\s*(dagnn_\w+)\s*;", open(HEADER).read(), flags=re.M)


def fields_of(cls):
    return [f for k in reversed(cls.__mro__) for f in k.__dict__.get("_fields_", [])]   # inherited ones first


def constants():
    return {k: v for k, v in vars(_lib).items() if k.isupper() and type(v) is int}


def _is(kind, ctype):
    return isinstance(ctype, type) and issubclass(ctype, kind)


def _name(ctype):
    return "POINTER(%s)" % _name(ctype._type_) if _is(C._Pointer, ctype) else ctype.__name__


def _binds(ctype, T):
    """C++ condition: C type T is what `ctype` (an argtype, a restype, a scalar field's type) binds."""
    if _is(C._Pointer, ctype):
        return "std::is_pointer_v<%s> && %s" % (T, _binds(ctype._type_, "pointee<%s>" % T))
    if _is(C.Structure, ctype):
        return "std::is_same_v<%s, %s>" % (T, _lib.C_TYPES[ctype])
    return "object_pointer<%s>" % T if ctype._type_ == "P" else "std::is_same_v<%s, %s>" % (T, SCALARS[ctype._type_])


def _member(out, name, T, ctype, path, offset):
    """Assertions on member `path` of C type T - ctypes has it as `ctype` at `offset` - and on everything inside it."""
    what, M = "%s.%s" % (name, path), "MEMBER(%s, %s)" % (T, path)
    out.append('static_assert(offsetof(%s, %s) == %d, "%s: offset %d");' % (T, path, offset, what, offset))
    out.append('static_assert(sizeof(%s) == %d, "%s: size %d");' % (M, C.sizeof(ctype), what, C.sizeof(ctype)))
    if _is(C.Array, ctype):
        out.append('static_assert(std::extent_v<%s> == %d, "%s: array of %d");' % (M, ctype._length_, what, ctype._length_))
        elem = ctype._type_
        walked = ctype._length_ if _is(C.Array, elem) or _is(C.Structure, elem) else 1   # scalars: the first stands for all
        for i in range(walked):
            _member(out, name, T, elem, "%s[%d]" % (path, i), offset + i * C.sizeof(elem))
    elif _is(C.Structure, ctype):
        for fname, ftype in fields_of(ctype):
            _member(out, name, T, ftype, "%s.%s" % (path, _lib.C_FIELD_NAMES.get((ctype, fname), fname)), offset + getattr(ctype, fname).offset)
    else:
        out.append('static_assert(%s, "%s: %s");' % (_binds(ctype, M), what, _name(ctype)))


def struct_asserts(cls, c_type, earlier=False):
    """Mirror `cls` against `c_type`: same size, as many members, every member in place.  `earlier` (a struct generation the library
    still serves; fields are only ever appended): every member in place, and no longer than the header's struct."""
    name, T, fields, size = cls.__name__, "T_" + cls.__name__, fields_of(cls), C.sizeof(cls)
    out = ["using %s = %s;" % (T, c_type),
           'static_assert(sizeof(%s) %s %d, "%s: sizeof %d");' % (T, ">=" if earlier else "==", size, name, size)]
    if not earlier:   # a member the mirror lacks can hide in padding; a structured binding takes exactly one name per member
        out.append("inline void members_of_%s(%s& s) { auto& [%s] = s; }   // %s: %d fields" % (
            name, T, ", ".join("m%d" % i for i in range(len(fields))), name, len(fields)))
    for fname, ftype in fields:
        _member(out, name, T, ftype, _lib.C_FIELD_NAMES.get((cls, fname), fname), getattr(cls, fname).offset)
    return out


def symbol_asserts(symbol, restype, argtypes):
    S = "sig<decltype(&%s)>" % symbol
    return ['static_assert(%s::arity == %d, "%s: %d arguments");' % (S, len(argtypes), symbol, len(argtypes)),
            'static_assert(%s, "%s: returns %s");' % (_binds(restype, S + "::ret"), symbol, _name(restype))] + \
           ['static_assert(%s, "%s: argument %d is %s");' % (_binds(a, "%s::arg<%d>" % (S, i)), symbol, i, _name(a)) for i, a in enumerate(argtypes)]


def source(structs=None, symbols=None, consts=None):
    """The translation unit; by default all of _lib.  `structs`: (mirror, C type, earlier generation?) each."""
    if structs is None:
        structs = [(cls, _lib.C_TYPES[cls], cls in _lib.C_EARLIER) for cls in mirrors()]
    lines = [PRELUDE] + [line for s in structs for line in struct_asserts(*s)]
    for symbol, (restype, argtypes) in (_lib.SYMBOLS if symbols is None else symbols).items():
        lines += symbol_asserts(symbol, restype, argtypes)
    for name, value in (constants() if consts is None else consts).items():   # DAGNN_OK is matched as itself
        lines.append('static_assert(%s == %d, "%s: %d");' % (name if name.startswith("DAGNN_") else "DAGNN_" + name, value, name, value))
    return "\n".join(lines) + "\n"


def check(structs=None, symbols=None, consts=None):
    """'' when the compiler accepts the assertions, else its messages."""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "abi_check.cpp")
        with open(path, "w") as fh:
            fh.write(source(structs, symbols, consts))
        run = subprocess.run([_build.hipcc_path(), "-x", "c++", "-std=c++17", "-fsyntax-only", "-ferror-limit=100", path],
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return "" if run.returncode == 0 else (run.stdout or "hipcc exited with %d" % run.returncode)

"""The whole ctypes binding against include/dagnn_hip.h, by the compiler (tests/abi_check.py): every mirror struct, every entry of
SYMBOLS, every constant.  Then the same check on mutated copies of mirrors, built in memory: each must fail, and the compiler's
message must name what was mutated."""
import ctypes as C

import pytest

from dagnn_amd import _lib
from tests import abi_check as A


def test_the_binding_matches_the_header():
    assert A.check() == ""


def test_every_header_struct_has_a_whole_mirror_and_every_mirror_a_c_type():
    declared = A.header_structs()
    # the three forms a typedef takes in the header: over several lines, on one line, of an unnamed struct
    assert {"dagnn_plan", "dagnn_gather_job", "dagnn_opt_tensor"} <= set(declared) and len(set(declared)) == len(declared)
    whole = {c_type for cls, c_type in _lib.C_TYPES.items() if cls not in _lib.C_EARLIER}
    assert set(declared) <= whole, set(declared) - whole
    assert set(A.mirrors()) == set(_lib.C_TYPES) >= _lib.C_EARLIER, set(A.mirrors()) ^ set(_lib.C_TYPES)
    assert {"DAGNN_OK", "EINVAL", "ENOSPC", "MAX_STACKED", "DVAE_SET_MAX_ROWS", "AGG_GIVEN", "POOL_MEAN"} <= set(A.constants())
    for cls in _lib.C_EARLIER:   # checked whole, an earlier generation is not the header's struct
        assert "%s: sizeof" % cls.__name__ in A.check([(cls, _lib.C_TYPES[cls], False)], {}, {})


def _at(fields, name):
    return [f[0] for f in fields].index(name)


def _swap(fields, name):
    i = _at(fields, name)
    assert C.sizeof(fields[i][1]) != C.sizeof(fields[i + 1][1])
    fields[i], fields[i + 1] = fields[i + 1], fields[i]


def _retype(fields, name, new_name, ctype):
    fields[_at(fields, name)] = (new_name, ctype)


def _restack(fields):   # another MAX_STACKED
    _retype(fields, "cell", "cell", (fields[_at(fields, "cell")][1]._type_._type_ * (_lib.MAX_STACKED - 1)) * _lib.MAX_DIRS)


CELL_ARRAYS = [cls for cls in A.mirrors() if getattr(dict(A.fields_of(cls)).get("cell"), "_length_", 0) == _lib.MAX_DIRS]   # cell[MAX_DIRS][MAX_STACKED]
STRUCTS = [   # (mirror, the change, what the messages must name, what they must not)
    (_lib.VariantBwdCell, lambda f: _swap(f, "w_node2"), ["VariantBwdCell.w_ld: offset", "VariantBwdCell.w_node2: offset"], "VariantBwdCell.esum"),
    # stat_rows goes into the tail padding: no size, no offset changes
    (_lib.DataflowArgs, lambda f: f.pop(), ["DataflowArgs: %d fields" % (len(_lib.DataflowArgs._fields_) - 1)], "DataflowArgs: sizeof"),
    (_lib.Plan, lambda f: _retype(f, "flags", "flag", C.c_int), ["no member named 'flag' in 'dagnn_plan'", "Plan.flag: offset"], "Plan.B"),
    # the pointer fills the int's own padding: nothing else moves
    (_lib.LayerArgs, lambda f: _retype(f, "static_score", "static_score", C.c_void_p),
     ["LayerArgs.static_score: size 8", "LayerArgs.static_score: c_void_p"], "LayerArgs.debug_timing"),
] + [(cls, _restack, ["%s.cell[0]: array of %d" % (cls.__name__, _lib.MAX_STACKED - 1), "%s.cell[1]: offset" % cls.__name__,
                      "%s: sizeof" % cls.__name__], "%s.cell: offset" % cls.__name__) for cls in CELL_ARRAYS]


def test_every_args_struct_with_a_cell_array_is_mutated():
    assert {c.__name__ for c in CELL_ARRAYS} == {"FrontierArgs", "DataflowArgs", "TilesArgs", "BackwardArgs", "BwdDataflowArgs",
                                                 "VariantArgs", "VariantBwdArgs"}


@pytest.mark.parametrize("cls,change,named,spared", STRUCTS, ids=["%s-%d" % (s[0].__name__, i) for i, s in enumerate(STRUCTS)])
def test_a_mutated_struct_fails_and_is_named(cls, change, named, spared):
    fields = list(A.fields_of(cls))
    change(fields)
    errors = A.check([(type(cls.__name__, (C.Structure,), {"_fields_": fields}), _lib.C_TYPES[cls], False)], {}, {})
    assert all(n in errors for n in named) and spared not in errors, errors


def _drop(args):
    args.pop(len(args) // 2)


def _replace(args, i, old, new):
    assert args[i] is old
    args[i] = new


SYMBOLS = [   # (symbol, the change, what the message must name, what it must not)
    ("dagnn_seq_ce_step", _drop, "dagnn_seq_ce_step: %d arguments" % (len(_lib.SYMBOLS["dagnn_seq_ce_step"][1]) - 1), "returns"),
    ("dagnn_heads_score", lambda a: _replace(a, 1, C.c_int64, C.c_int), "dagnn_heads_score: argument 1 is c_int", "arguments"),
    ("dagnn_dataflow_run", lambda a: _replace(a, 0, C.POINTER(_lib.Plan), C.POINTER(_lib.DvaeSet)),
     "dagnn_dataflow_run: argument 0 is POINTER(DvaeSet)", "argument 1"),
    ("dagnn_frontier_run", lambda a: _replace(a, 2, C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.c_int32)),
     "dagnn_frontier_run: argument 2 is POINTER(c_int)", "argument 3"),
]


@pytest.mark.parametrize("symbol,change,named,spared", SYMBOLS, ids=[s[0] for s in SYMBOLS])
def test_a_mutated_entry_point_fails_and_is_named(symbol, change, named, spared):
    restype, argtypes = _lib.SYMBOLS[symbol]
    argtypes = list(argtypes)
    change(argtypes)
    errors = A.check([], {symbol: (restype, argtypes)}, {})
    assert named in errors and spared not in errors, errors


def test_a_constant_off_by_one_and_one_the_header_lacks_are_named():
    errors = A.check([], {}, {"PULL_ROW": _lib.PULL_ROW + 1, "MAX_DIRS": _lib.MAX_DIRS})
    assert "PULL_ROW: %d" % (_lib.PULL_ROW + 1) in errors and "MAX_DIRS" not in errors
    assert "DAGNN_NO_SUCH_LIMIT" in A.check([], {}, {"NO_SUCH_LIMIT": 1})

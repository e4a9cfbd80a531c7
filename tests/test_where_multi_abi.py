"""CPU: libsjhip.so and the Python mirror export sjhip_where_paths and sjhip_count_where_paths with the argument counts of the
header; the limits and the program bytes are one number in the header, in csrc/sj_where.h and in the mirror; and the program check
and the bit-stack evaluator of csrc/sj_where.h (replayed by the compiled selftest, sj_selftest_where_program) are the checker's
(tests/where_multi_walk.py check_program, evaluate): every program of up to 5 bytes over 2 predicates with every truth mask, a
chain that fills the 32 bits of the stack, and every family of invalid programs."""
import ctypes as C
import itertools
import os
import re

import __graft_entry__ as G
import where_multi_walk as MW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sjhip.h")).read(), flags=re.S)
AND, OR, NEG = MW.WHERE_AND, MW.WHERE_OR, MW.WHERE_NEG
# the header's declarations: ctx, keys, key_lens, path_lens, ops, values, value_lens, n_preds, program, program_len = 10, then
# records and rows / count
N_ARGS = {"sjhip_where_paths": 12, "sjhip_count_where_paths": 11}


def selftest():
    lib = C.CDLL(G.build_selftest())
    lib.sj_selftest_where_program.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32]
    lib.sj_selftest_where_program.restype = C.c_int
    return lib


def replay(lib, program, n_preds, masks):
    """the compiled check and evaluator against the checker's, for every truth mask given"""
    program = bytes(program)
    why, pos = MW.check_program(program, n_preds)
    for mask in masks:
        got = lib.sj_selftest_where_program(program, len(program), n_preds, mask)
        if why:
            assert got == -(256 * why + pos), (program.hex(), n_preds, mask, got, why, pos)
        else:
            assert got == int(MW.evaluate(program, [(mask >> p) & 1 for p in range(n_preds)])), (program.hex(), n_preds, mask, got)
    return why, pos


def test_library_exports_the_calls():
    L = C.CDLL(G.build_lib())
    import sjhip
    for name, n_args in N_ARGS.items():
        assert hasattr(L, name) and hasattr(sjhip.lib(), name)
        res, args = sjhip._lib.SYMBOLS[name]
        assert res is C.c_int and len(args) == n_args
        decl = re.search(r"\bint %s\((.*?)\);" % name, HDR, flags=re.S).group(1)
        assert len(decl.split(",")) == n_args, decl
    assert hasattr(sjhip.Context, "where_paths") and hasattr(sjhip.Context, "count_where_paths")


def test_the_limits_and_the_program_bytes_are_one_number():
    import sjhip
    out = (C.c_int * 5)()
    selftest().sj_selftest_where_limits(out)
    in_header = [int(re.search(r"#define SJHIP_WHERE_MAX_PREDS (\d+)\b", HDR).group(1)),
                 int(re.search(r"#define SJHIP_WHERE_MAX_PROGRAM (\d+)\b", HDR).group(1))]
    in_header += [int(re.search(r"\bSJHIP_WHERE_%s = (0x[0-9a-fA-F]+)" % name, HDR).group(1), 16) for name in ("AND", "OR", "NEG")]
    ctx = sjhip.Context
    assert in_header == [16, 64, 0x80, 0x81, 0x82] == list(out)
    assert in_header == [ctx.WHERE_MAX_PREDS, ctx.WHERE_MAX_PROGRAM, ctx.WHERE_AND, ctx.WHERE_OR, ctx.WHERE_NEG]
    assert in_header == [MW.WHERE_MAX_PREDS, MW.WHERE_MAX_PROGRAM, MW.WHERE_AND, MW.WHERE_OR, MW.WHERE_NEG]
    assert in_header[0] == int(re.search(r"#define SJHIP_TABLE_MAX_COLS (\d+)\b", HDR).group(1)) == ctx.TABLE_MAX_COLS  # one plan


def test_every_short_program_over_two_predicates():
    lib = selftest()
    valid = 0
    for n in range(1, 6):
        for program in itertools.product((0, 1, AND, OR, NEG), repeat=n):
            valid += replay(lib, program, 2, range(4))[0] == MW.PROG_OK
    assert valid > 50  # (0 1 AND, 0 1 OR, their negations and operand orders, 0 0 AND 1 OR, ...)


def test_a_chain_that_fills_the_stack():
    lib = selftest()
    # 32 pushes, then 31 operators: a right-leaning chain, the stack 32 deep before the first operator
    for ops in ([AND] * 31, [OR] * 31, [AND, OR] * 15 + [AND], [OR, OR, AND] * 10 + [OR]):
        program = bytes([p % 16 for p in range(32)] + ops)
        assert len(program) == 63
        masks = [0, 0xffff, 1, 0x8000, 0xfffe, 0x7fff, 0x5555, 0xaaaa, 0x00ff, 0x0100, 0x1234, 0xedcb]
        assert replay(lib, program, 16, masks) == (MW.PROG_OK, 0)
    assert replay(lib, bytes([p % 16 for p in range(32)] + [AND] * 31 + [NEG]), 16, [0, 0xffff, 0x8000]) == (MW.PROG_OK, 0)  # 64 bytes


def test_every_invalid_family():
    lib = selftest()
    for program, n_preds, want in [
            ([AND], 2, (MW.PROG_UNDERFLOW, 0)), ([NEG, 0], 1, (MW.PROG_UNDERFLOW, 0)), ([OR, 0, 1], 2, (MW.PROG_UNDERFLOW, 0)),
            ([0, 1, AND, OR, 0], 2, (MW.PROG_UNDERFLOW, 3)), ([0, AND, 1], 2, (MW.PROG_UNDERFLOW, 1)),
            ([0, 1], 2, (MW.PROG_LEFT, 2)), ([0, 1, 0, AND], 2, (MW.PROG_LEFT, 4)),
            ([0, 0, OR], 2, (MW.PROG_UNUSED, 1)), ([1, NEG], 3, (MW.PROG_UNUSED, 0)),
            ([0, 2, OR], 2, (MW.PROG_PREDICATE, 1)), ([1], 1, (MW.PROG_PREDICATE, 0)), ([0, 15, AND], 15, (MW.PROG_PREDICATE, 1)),
            ([0, 0x83], 1, (MW.PROG_BYTE, 1)), ([0x7f], 1, (MW.PROG_BYTE, 0)), ([0, 16, OR], 16, (MW.PROG_BYTE, 1)), ([0, 0xff], 1, (MW.PROG_BYTE, 1)),
            ([], 1, (MW.PROG_LENGTH, 0)), ([0] + [NEG] * 64, 1, (MW.PROG_LENGTH, 0))]:
        assert replay(lib, program, n_preds, [0, 1, 3]) == want, (program, n_preds)
    assert len(bytes([0] + [NEG] * 64)) == 65 and replay(lib, [0] + [NEG] * 63, 1, [0, 1]) == (MW.PROG_OK, 0)

// sj_where.h -- the plan of a row predicate over SEVERAL tests (sjhip_where_paths): up to 16 predicates, each a path, an operator
// and a value, resolved in ONE walk per row and combined by a postfix program of AND / OR / NEG.
// Plain C++ (no HIP): host_selftest.cpp exports the checker and the evaluator (sj_selftest_where_program,
// tests/test_where_multi_abi.py).
//
// The predicates with a path are the columns of a table plan (sj_table.h): the walk of sj_tablewalk.h hands every column the tape
// index of its element, or SJHIP_PATH_NOT_*, and the sink sets the predicate's bit in a truth mask.  A predicate with an empty path
// tests the row's own value and is no column.  The program then runs over the mask.  A valid program of at most 64 bytes holds at
// most 32 pushes (every push but one needs an AND or an OR behind it), so its stack never holds more than 32 values: the stack is
// the bits of one u32, its top in bit 0.  A push is a shift; AND and OR fold the two low bits; NEG flips bit 0.  The program is a
// kernel argument -- the same bytes for every lane -- so the loop over it does not diverge.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "sj_chunk.h"
#include "sj_table.h"

namespace sj {

static constexpr int WHERE_MAX_PREDS = 16;          // SJHIP_WHERE_MAX_PREDS (= TABLE_MAX_COLS: one plan)
static constexpr int WHERE_MAX_PROGRAM = 64;        // SJHIP_WHERE_MAX_PROGRAM
static constexpr int WHERE_MAX_VALUE_BYTES = 1024;  // bytes of all values together (QMAX: they travel in QView::val)
static constexpr uint8_t WHERE_AND = 0x80, WHERE_OR = 0x81, WHERE_NEG = 0x82;  // SJHIP_WHERE_AND / _OR / _NEG
static_assert(WHERE_MAX_PREDS == TABLE_MAX_COLS, "the predicates with a path are the columns of one table plan");

struct WherePlan {
    TablePlan pl;                        // the predicates with a path, in the order the caller named them (no column: n_cols 0)
    uint64_t want[WHERE_MAX_PREDS];      // per predicate: the wanted bits of a number or a bool
    uint16_t val_b[WHERE_MAX_PREDS];     // ... and its string value: val[val_b .. val_b + val_n)
    uint16_t val_n[WHERE_MAX_PREDS];
    uint8_t op[WHERE_MAX_PREDS];         // SJHIP_OP_*
    uint8_t pred_of_col[TABLE_MAX_COLS]; // column c of pl is predicate pred_of_col[c]
    uint16_t empty;                      // bit p: predicate p has an empty path -- it tests the row's own value
    uint8_t n_preds, program_len;
    uint8_t program[WHERE_MAX_PROGRAM];
};

// why a program was refused (the text for sjhip_last_error: where_program_error)
enum WhereProgramError {
    WHERE_PROG_OK = 0,
    WHERE_PROG_LENGTH,     // program_len outside 1 .. 64
    WHERE_PROG_BYTE,       // a byte that is no predicate and no operator     (*pos: where it stands)
    WHERE_PROG_PREDICATE,  // a predicate >= n_preds                          (*pos: where it stands)
    WHERE_PROG_UNDERFLOW,  // an operator without its operands                (*pos: where it stands)
    WHERE_PROG_LEFT,       // more than one value on the stack at the end     (*pos: program_len)
    WHERE_PROG_UNUSED      // a predicate the program never names             (*pos: the predicate)
};
inline const char *where_program_error(int e) {
    switch (e) {
    case WHERE_PROG_LENGTH: return "a program holds 1 to 64 bytes";
    case WHERE_PROG_BYTE: return "a byte that is neither a predicate (0 .. 15) nor SJHIP_WHERE_AND / _OR / _NEG";
    case WHERE_PROG_PREDICATE: return "a predicate the call does not hold";
    case WHERE_PROG_UNDERFLOW: return "an operator without its operands on the stack";
    case WHERE_PROG_LEFT: return "more than one value is left on the stack at the end";
    case WHERE_PROG_UNUSED: return "a predicate that the program never names";
    }
    return "";
}

// -> WHERE_PROG_OK, or what is wrong with *pos: the position in the program it was found at (WHERE_PROG_UNUSED: the predicate)
inline int where_program_check(const uint8_t *program, uint32_t len, uint32_t n_preds, uint32_t *pos) {
    *pos = 0;
    if (len < 1 || len > (uint32_t)WHERE_MAX_PROGRAM) return WHERE_PROG_LENGTH;
    uint32_t depth = 0, used = 0;
    for (uint32_t i = 0; i < len; i++) {
        const uint8_t b = program[i];
        *pos = i;
        if (b < (uint8_t)WHERE_MAX_PREDS) {
            if (b >= n_preds) return WHERE_PROG_PREDICATE;
            used |= 1u << b;
            depth++;
        } else if (b == WHERE_AND || b == WHERE_OR) {
            if (depth < 2) return WHERE_PROG_UNDERFLOW;
            depth--;
        } else if (b == WHERE_NEG) {
            if (depth < 1) return WHERE_PROG_UNDERFLOW;
        } else {
            return WHERE_PROG_BYTE;
        }
    }
    *pos = len;
    if (depth != 1) return WHERE_PROG_LEFT;
    for (uint32_t p = 0; p < n_preds; p++)
        if (!((used >> p) & 1u)) {
            *pos = p;
            return WHERE_PROG_UNUSED;
        }
    *pos = 0;
    return WHERE_PROG_OK;
}

// the value of a VALID program for the truth of its predicates (bit p of truth: predicate p holds)
SJ_HD bool where_program_eval(const uint8_t *program, u32 len, u32 truth) {
    u32 st = 0;  // the stack: its top in bit 0
    for (u32 i = 0; i < len; i++) {
        const u32 b = program[i];
        const u32 below = st >> 1;  // the stack without its top
        if (b < (u32)WHERE_MAX_PREDS) st = (st << 1) | ((truth >> b) & 1u);
        else if (b == WHERE_AND) st = below & (st | ~1u);
        else if (b == WHERE_OR) st = below | (st & 1u);
        else st ^= 1u;
    }
    return (st & 1u) != 0;
}

}  // namespace sj

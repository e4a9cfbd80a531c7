"""A row predicate over several tests, restated on (Tape, Strings.B, Message) arrays -- the checker of the device calls
sjhip_where_paths / sjhip_count_where_paths (test infrastructure, on where_walk.satisfies and rows_walk.RowWalk.find_path).

  truth          one predicate (path, op, want) on the row whose value lies at tape index v0: the element at the path exists and
                 satisfies the operator (an empty path: the row's own value) -- where_walk.where's test without negate
  check_program  the validity of a postfix program over n_preds predicates -> (reason, position): PROG_OK, or the first thing that
                 is wrong and where: the position in the program (PROG_UNUSED: the predicate; PROG_LEFT: the length)
  evaluate       the value of a valid program for the truths of its predicates -- a Python list as the stack
  where_multi    one call: the rows of the selection (None: the records, one row each) for which the program is true; every record
                 keeps the matching ones among the rows it owned -> (row_offsets, row_index, statuses), where_walk.where's shape

Pinned by tests/test_where_multi_walk.py."""
import query_walk as Q
import rows_walk as RW
import where_walk as WW

WHERE_AND, WHERE_OR, WHERE_NEG = 0x80, 0x81, 0x82
WHERE_MAX_PREDS = 16
WHERE_MAX_PROGRAM = 64
PROG_OK, PROG_LENGTH, PROG_BYTE, PROG_PREDICATE, PROG_UNDERFLOW, PROG_LEFT, PROG_UNUSED = range(7)


def truth(w, v0, predicate, rw=None):
    path, op, want = predicate
    if not len(path):
        return bool(WW.satisfies(w, v0, op, want))
    rw = rw if rw is not None else RW.RowWalk(w, [v0])
    v = rw.find_path(v0 - 1, list(path))
    return bool(v < Q.NOT_OBJECT and WW.satisfies(w, v, op, want))


def check_program(program, n_preds):
    program = bytes(program)
    if not 1 <= len(program) <= WHERE_MAX_PROGRAM:
        return PROG_LENGTH, 0
    depth, used = 0, set()
    for i, b in enumerate(program):
        if b < WHERE_MAX_PREDS:
            if b >= n_preds:
                return PROG_PREDICATE, i
            used.add(b)
            depth += 1
        elif b in (WHERE_AND, WHERE_OR):
            if depth < 2:
                return PROG_UNDERFLOW, i
            depth -= 1
        elif b == WHERE_NEG:
            if depth < 1:
                return PROG_UNDERFLOW, i
        else:
            return PROG_BYTE, i
    if depth != 1:
        return PROG_LEFT, len(program)
    for p in range(n_preds):
        if p not in used:
            return PROG_UNUSED, p
    return PROG_OK, 0


def evaluate(program, truths):
    stack = []
    for b in bytes(program):
        if b < WHERE_MAX_PREDS:
            stack.append(bool(truths[b]))
        elif b == WHERE_NEG:
            stack.append(not stack.pop())
        else:
            y, x = stack.pop(), stack.pop()
            stack.append((x and y) if b == WHERE_AND else (x or y))
    assert len(stack) == 1
    return stack[0]


def where_multi(w, sel, predicates, program):
    assert 1 <= len(predicates) <= WHERE_MAX_PREDS and check_program(program, len(predicates)) == (PROG_OK, 0)
    offs, index, sts = WW.records_selection(w) if sel is None else sel
    rw = RW.RowWalk(w, index)
    before, new_index = [0], []  # before[i]: the kept rows in front of row i
    for v0 in rw.rows:
        if evaluate(program, [truth(w, v0, p, rw) for p in predicates]):
            new_index.append(v0)
        before.append(len(new_index))
    return [before[o] for o in offs], new_index, list(sts)

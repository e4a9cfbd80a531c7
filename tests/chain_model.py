"""A host model of the query layer's call chains: one row selection, seven products, three tenants of the shared arenas -- and a
seeded generator of chains over them (test infrastructure: plain Python, no GPU; pinned by tests/test_chain_model.py, used by
tests/test_gpu_chains.py and tests/test_debug_bounds_chains.py).

THE LIFETIME TABLE.  Taken from the comments of csrc/sj_result.h and include/sjhip.h, not from running the device.  Per call: what
it does to the selection, which product it replaces, which tenant of d_q / d_qtape / d_qstrings it leaves.

  call                         selection                         product replaced    tenant
  select_rows(path)            replaced (from the RECORDS)       rows                -
  select_records()             dropped: the rows' begin()        rows (gone)         -
  where_path / where_paths     narrowed; created without one     rows                -
  unnest_rows(path)            replaced (from the ROWS)          rows, parents       -
  unnest_members(path)         replaced (from the ROWS),         rows, parents       -
                               `members` set
  where_row_names(op, value)   narrowed; needs `members`         rows                -
  order_path[_strings|s]       narrowed to rank < limit          rows, order         -
  extract_path_strings         read                              column              -
  extract_row_names            read; needs `members`             column              -
  extract_path_list[_strings]  read                              list                -
  extract_table                read                              table               -
  group_path / group_paths     read                              groups              -
  aggregate_path               read                              -                   -
  aggregate_path_records       read                              -                   -
  count_where_paths            read                              -                   -
  filter_rows                  read (needs one; copied strings)  -                   filtered
  marshal_rows                 read (needs one)                  -                   marshaled (by rows)
  marshal_rows_paths           read (needs one)                  -                   marshaled (by rows)
  marshal_json                 ignored                           -                   marshaled (no row offsets)
  serialize                    ignored (copied strings)          -                   serialized

  * A product lives from its publish to the next call of its own kind (or a parse, trim, deserialize, stage-1-only call: none of
    them occurs inside a chain).  It is materialised data: every later change or drop of the selection, every other product and
    every tenant leave it bit for bit as it was -- its row numbers are those of the selection its call left.
  * At most one tenant is resident: a call that claims the shared arenas ends the previous tenant.  sjhip_fetch_marshaled_rows
    after marshal_json is refused (that text has no rows); sjhip_fetch_marshaled delivers either text.
  * A call that fails its argument checks (SJHIP_ERR_ARG) touches nothing: not the selection, not the product of its own kind, not
    the tenant.  That holds for filter_rows / marshal_rows without a selection as well.  (serialize and marshal_json give up THEIR
    OWN tenant before their checks; no chain makes them fail.)
  * A fetch of what does not exist is SJHIP_ERR_ARG and changes nothing.
  * `members` (sjhip.h, "Member rows"): the selection in force is one of object members -- "the one sjhip_unnest_members left, or
    what sjhip_where_*, sjhip_where_row_names and the limit of sjhip_order_* narrowed it to".  Every narrowing hands it on;
    select_rows, unnest_rows and select_records clear it.  Nothing is stored per row: the name of a row is the string two tape
    words in front of its value, and the model reads it from there (members_walk.names_of) after every narrowing, as the device
    must.  Without it the two name calls are SJHIP_ERR_ARG ("... not object members ...") and touch nothing.
  * extract_row_names publishes the string column, the product of extract_path_strings: a late fetch of `column` delivers whichever
    of the two ran last.  marshal_rows_paths publishes the marshaled tenant with row offsets; "the selection, the string column,
    the list column and the table stay as they are".

A step is a tuple (do, name, args): do = "call" (args: the positional arguments of the Context method, then a dict of keywords),
"fetch" (name: a product or tenant), "refused" (a fetch the model says must fail) or "invalid" (name: the call, args: the family).
"""
import functools
import random

import numpy as np

import aggregate_walk as AW
import column_walk as CW
import filter_rows_walk as FW
import fixtures
import group_multi_walk as GMW
import group_walk as GW
import marshal_rows_walk as MRW
import members_walk as MBW
import oracle_lib as O
import order_multi_walk as OMW
import order_strings_walk as OSW
import order_walk as OW
import project_rows_walk as PRW
import query_walk as Q
import rows_walk as RW
import unnest_walk as UW
import where_multi_walk as MW
import where_walk as WW

F, I, U, B, S, SC = CW.COL_FLOAT, CW.COL_INT, CW.COL_UINT, CW.COL_BOOL, GW.COL_STRING, 5
ERR_ARG = 5
U64 = (1 << 64) - 1
AND, OR, NEG = MW.WHERE_AND, MW.WHERE_OR, MW.WHERE_NEG

SELECTION_CALLS = ("select_rows", "select_records", "where_path", "where_paths", "unnest_rows", "order_path", "order_path_strings",
                   "order_paths")
NARROWINGS = ("where_path", "where_paths", "order_path", "order_path_strings", "order_paths")
BUILDS = ("extract_path_strings", "extract_path_list", "extract_path_list_strings", "extract_table", "group_path", "group_paths",
          "aggregate_path", "filter_rows", "marshal_rows", "marshal_json", "serialize")
# the calls the first model did not know (the tuples above stay those of CHAINS' conditions; the *_M ones are what the driver uses)
NEW_CALLS = ("unnest_members", "where_row_names", "extract_row_names", "marshal_rows_paths", "aggregate_path_records", "count_where_paths")
SELECTION_CALLS_M = SELECTION_CALLS + ("unnest_members", "where_row_names")
NARROWINGS_M = NARROWINGS + ("where_row_names",)
CLEARS_MEMBERS = ("select_rows", "unnest_rows", "select_records")
BUILDS_M = BUILDS + ("extract_row_names", "marshal_rows_paths", "aggregate_path_records", "count_where_paths")
PRODUCTS = ("column", "list", "table", "rows", "groups", "order", "parents")
TENANTS = ("filtered", "serialized", "marshaled")
FETCHES = PRODUCTS + TENANTS + ("marshaled_rows",)
# the product or tenant a call publishes
PUBLISHES = {"extract_path_strings": "column", "extract_path_list": "list", "extract_path_list_strings": "list", "extract_table": "table",
             "group_path": "groups", "group_paths": "groups", "order_path": "order", "order_path_strings": "order", "order_paths": "order",
             "unnest_rows": "parents", "filter_rows": "filtered", "marshal_rows": "marshaled", "marshal_json": "marshaled",
             "serialize": "serialized", "unnest_members": "parents", "extract_row_names": "column", "marshal_rows_paths": "marshaled"}
INVALID_FAMILIES = ("kind", "path17", "program")
INVALID_FAMILIES_M = ("not_members", "name_op", "project")
PROJECT_FORMS = ("cols17", "empty_unnamed", "flag", "no_selection")
NOT_MEMBERS = "not object members"
# the malformed programs: one of every family of tests/test_where_multi_abi.py test_every_invalid_family (over two predicates)
BAD_PROGRAMS = [bytes([AND]), bytes([0, 1]), bytes([0, 0, OR]), bytes([0, 2, OR]), bytes([0, 1, 0x83]), b"", bytes([0, 1, AND] + [NEG] * 64)]
SIZES = (63, 65, 255, 257, 1023, 1025, 1100)


# ---- the model ------------------------------------------------------------------------------------------------------------------------
class Expect:
    """what a step must give: ret (the call's return values, None for a fetch), content (what a fetch returns, in the canonical
    form of device_fetch; None when nothing is fetched), error (the code the step must fail with, or 0)"""

    def __init__(self, ret=None, content=None, error=0):
        self.ret, self.content, self.error = ret, content, error


class Model:
    def __init__(self, w, ref=None, exact_floats=()):
        self.w, self.ref = w, ref
        self.exact_floats = set(exact_floats)  # the FLOAT paths on which every partial sum is exact
        self.sel = None      # (row offsets, row index, record statuses)
        self.live = {}       # product -> content
        self.tenant = None   # (tenant, content, by rows)
        self.members = False  # the selection in force is one of object members
        self.origin = {}     # product or tenant -> the call that published it
        self.n_records = len(w.records())

    def rw(self):
        return self.w if self.sel is None else RW.RowWalk(self.w, self.sel[1])

    def rows(self):
        return self.n_records if self.sel is None else len(self.sel[1])

    def _select(self, sel):
        self.sel = tuple(list(map(int, a)) for a in sel)
        self.live["rows"] = self.sel

    def _bound(self, path, vals, sts):
        """None: compared as bits; else the bound of tests/test_gpu_aggregate.py float_bound"""
        if tuple(path) in self.exact_floats:
            return None
        from test_gpu_aggregate import float_bound
        return float_bound(vals, sts)

    def exists(self, what):
        if what in PRODUCTS:
            return what in self.live
        if what == "marshaled_rows":
            return self.tenant is not None and self.tenant[0] == "marshaled" and self.tenant[2]
        return self.tenant is not None and self.tenant[0] == what

    def content(self, what):
        if what in PRODUCTS:
            return self.live[what]
        if what == "marshaled":
            return self.tenant[1][1] if self.tenant[2] else self.tenant[1]
        if what == "marshaled_rows":
            return self.tenant[1][1:]
        return self.tenant[1]

    def apply(self, step):
        do, name, args = step
        if do == "fetch":
            assert self.exists(name), step
            return Expect(content=self.content(name))
        if do == "refused":
            assert not self.exists(name), step
            return Expect(error=ERR_ARG)
        if do == "invalid":
            fam = args[0] if isinstance(args, tuple) else args
            assert fam != "not_members" or not self.members, step   # (what makes the call invalid must hold in the model)
            assert fam != "name_op" or (self.members and args[1] not in (Q.OP_EQ_STRING, WW.OP_PREFIX_STRING)), step
            assert fam != "project" or (self.sel is None) == (args[1] == "no_selection"), step
            return Expect(error=ERR_ARG)  # (nothing is touched)
        has_kw = bool(args) and isinstance(args[-1], dict)
        kw, pos = (args[-1], args[:-1]) if has_kw else ({}, args)
        fetch = kw.get("fetch", True)
        e = getattr(self, "_" + name)(*pos, **{k: v for k, v in kw.items() if k != "fetch"})
        if name in PUBLISHES:
            self.origin[PUBLISHES[name]] = name
        if not fetch:
            e.content = None
        return e

    # ---- the selection ----
    def _select_rows(self, path):
        self._select(RW.select_rows(self.w, path))
        self.members = False
        return Expect((self.n_records, len(self.sel[1])))

    def _select_records(self):
        self.sel = None
        self.members = False
        self.live.pop("rows", None)
        return Expect(None)

    def _where_path(self, path, op, value=None, negate=False):
        self._select(WW.where(self.w, self.sel, path, op, value, negate))
        return Expect((self.n_records, len(self.sel[1])))

    def _where_paths(self, predicates, program):
        self._select(MW.where_multi(self.w, self.sel, [(tuple(p), op, v) for p, op, v in predicates], program))
        return Expect((self.n_records, len(self.sel[1])))

    def _unnest_rows(self, path):
        if self.sel is None:
            got = UW.unnest_rows(UW.record_rows(self.w), path)
        else:
            got = UW.unnest_rows(RW.RowWalk(self.w, self.sel[1]), path, self.sel[0], self.sel[2])
        self._select(got[:3])
        self.members = False
        self.live["parents"] = tuple(list(map(int, a)) for a in got[3:])
        return Expect((self.n_records, len(got[5]), len(got[1])), self.live["parents"])

    def _unnest_members(self, path):
        if self.sel is None:
            got = MBW.unnest_members(UW.record_rows(self.w), path)
        else:
            got = MBW.unnest_members(RW.RowWalk(self.w, self.sel[1]), path, self.sel[0], self.sel[2])
        self._select(got[:3])
        self.members = True
        self.live["parents"] = tuple(list(map(int, a)) for a in got[3:6])
        return Expect((self.n_records, len(got[5]), len(got[1])), self.live["parents"])

    def names(self):
        """the names of the rows in force, read back from the tape"""
        assert self.members, "the model's selection is not one of members"
        return MBW.names_of(self.w, self.sel[1])

    def _where_row_names(self, op, value, negate=False):
        assert op in (Q.OP_EQ_STRING, WW.OP_PREFIX_STRING), op
        offs, index, sts = self.sel
        hit = [(n == value if op == Q.OP_EQ_STRING else n.startswith(value)) != bool(negate) for n in self.names()]
        before = [0]
        for h in hit:
            before.append(before[-1] + h)
        self._select(([before[o] for o in offs], [v for v, h in zip(index, hit) if h], sts))
        return Expect((self.n_records, len(self.sel[1])))

    def _ordered(self, o, values):
        self._select(o.selection)
        self.live["order"] = (list(o.order), values, [int(s) for s in o.status])
        return Expect((self.n_records, o.rows), self.live["order"])

    def _order_path(self, path, kind, descending=False, limit=0):
        o = OW.order(self.w, self.sel, path, kind, descending, limit)
        return self._ordered(o, [int(v) for v in o.values])

    def _order_path_strings(self, path, descending=False, limit=0):
        return self._ordered(OSW.order(self.w, self.sel, path, descending, limit), None)

    def _order_paths(self, columns, limit=0):
        return self._ordered(OMW.order(self.w, self.sel, [(tuple(p), k, d) for p, k, d in columns], limit), None)

    # ---- the products ----
    def _extract_path_strings(self, path, cvt=False):
        off, data, st = RW.string_column(self.rw(), path, cvt)
        self.live["column"] = (list(off), bytes(data), list(st))
        return Expect((len(st), len(data)), self.live["column"])

    def _extract_row_names(self):
        names, off = self.names(), [0]
        for n in names:
            off.append(off[-1] + len(n))
        self.live["column"] = (off, b"".join(names), [CW.COL_OK] * len(names))
        return Expect((len(names), off[-1]), self.live["column"])

    def _extract_path_list(self, path, kind):
        off, vals, st = RW.list_column(self.rw(), path, kind)
        self.live["list"] = (list(off), [int(v) for v in vals], list(st))
        return Expect((len(st), len(vals)), self.live["list"])

    def _extract_path_list_strings(self, path, cvt=False):
        loff, soff, data, st = RW.list_string_column(self.rw(), path, cvt)
        self.live["list"] = (list(loff), list(soff), bytes(data), list(st))
        return Expect((len(st), len(soff) - 1, len(data)), self.live["list"])

    def _extract_table(self, columns):
        cols = [(tuple(p), k) for p, k in columns]
        out = []
        for (_, kind), col in zip(cols, RW.table(self.rw(), cols)):
            out.append((list(col[0]), bytes(col[1]), list(col[2])) if kind >= S else ([int(v) for v in col[0]], list(col[1])))
        self.live["table"] = out
        return Expect((self.rows(), [len(c[1]) if k >= S else 0 for (_, k), c in zip(cols, out)]), out)

    def _group_path(self, key_path, key_kind, value_path=None, value_kind=None):
        rw = self.rw()
        g = GW.group(rw, key_path, key_kind, value_path, value_kind)
        keys = list(g.keys) if key_kind == S else [k & U64 for k in g.keys]
        nbytes = sum(map(len, g.keys)) if key_kind == S else 8 * g.groups
        aggs = sums = None
        if value_kind is not None:
            aggs = [list(a) for a in GW.arrays(g, value_kind)]
            if value_kind == F:
                vals, vsts = AW.column(rw, () if value_path is None else value_path, F)
                members = [[r for r, c in enumerate(g.codes) if c == k] for k in range(g.groups)]
                sums = [(a.sum, self._bound(value_path or (), [vals[r] for r in m], [vsts[r] for r in m])) for a, m in zip(g.aggs, members)]
        self.live["groups"] = ("one", keys, list(g.first_row), list(g.group_rows), list(g.codes), list(g.status), aggs, sums)
        return Expect((g.rows, g.groups, nbytes), self.live["groups"])

    def _group_paths(self, key_columns, value_columns=()):
        kcols = [(tuple(c[0]), c[1]) + tuple(c[2:]) for c in key_columns]
        vcols = [(tuple(p), k) for p, k in value_columns]
        g = GMW.group(self.rw(), kcols, vcols)
        kinds = [c[1] for c in kcols]
        keys = [[(b"" if k is None else k) if kind == S else ((0 if k is None else k) & U64) for k in col] for col, kind in zip(g.keys, kinds)]
        values = [[list(a) for a in GMW.arrays(g, v, kind)] for v, (_, kind) in enumerate(vcols)]
        self.live["groups"] = ("many", keys, [list(k) for k in g.key_ok], [list(s) for s in g.status], list(g.first_row),
                               list(g.group_rows), list(g.codes), values)
        return Expect((g.rows, g.groups, GMW.key_bytes(g, kinds)), self.live["groups"])

    def _aggregate_path(self, path, kind):
        vals, sts = AW.column(self.rw(), path, kind)
        a = AW.reduce(vals, sts, kind)
        bound = self._bound(path, vals, sts) if kind == F else None
        return Expect(None, ("agg", kind, a.rows, list(a.status), AW.bits_of(a.min, kind), AW.bits_of(a.max, kind), a.sum, bound))

    def _aggregate_path_records(self, path, kind):
        rw = self.rw()
        vals, sts = AW.column(rw, path, kind)
        offs = list(range(len(vals) + 1)) if self.sel is None else self.sel[0]
        per = [AW.reduce(vals[a:b], sts[a:b], kind) for a, b in zip(offs[:-1], offs[1:])]
        bounds = None
        if kind == F and tuple(path) not in self.exact_floats:
            from test_gpu_aggregate import float_bound
            bounds = [float_bound(vals[a:b], sts[a:b]) for a, b in zip(offs[:-1], offs[1:])]
        return Expect(None, ("aggrec", kind, [list(a) for a in AW.record_arrays(per, kind)], bounds))

    def _count_where_paths(self, predicates, program):
        return Expect(len(MW.where_multi(self.w, self.sel, [(tuple(p), op, v) for p, op, v in predicates], program)[1]))

    # ---- the tenants ----
    def _filter_rows(self):
        tape, strings, skipped = FW.filter_rows(self.w, self.sel[1])
        content = (len(self.sel[1]) - skipped, skipped, [int(x) for x in tape], bytes(strings))
        self.tenant = ("filtered", content, False)
        return Expect((content[0], skipped, len(tape), len(strings)), content)

    def _marshal_rows(self):
        text, offsets = MRW.marshal_rows(self.w, self.sel[1])
        content = (len(self.sel[1]), bytes(text), list(offsets))
        self.tenant = ("marshaled", content, True)
        return Expect((content[0], len(text)), content)

    def _marshal_rows_paths(self, columns, names=None, nulls=False):
        text, offsets = PRW.project_rows(self.w, self.sel[1], [tuple(p) for p in columns], names, nulls)
        content = (len(self.sel[1]), bytes(text), list(offsets))
        self.tenant = ("marshaled", content, True)
        return Expect((content[0], len(text)), content)

    def _marshal_json(self):
        rc, text = O.marshal_json(self.ref.tape, self.ref.strings, self.w.m)
        assert rc == 0
        self.tenant = ("marshaled", bytes(text), False)
        return Expect(len(text), bytes(text))

    def _serialize(self):
        stream = bytes(O.serialize(self.ref.tape, self.ref.strings, self.w.m, dedup=False)[0])
        self.tenant = ("serialized", stream, False)
        return Expect(len(stream), stream)


# ---- the device side: one step on a Context, in the model's canonical forms --------------------------------------------------------------
def _bits(a):
    """the bit patterns of a column of 1-byte or 8-byte entries"""
    if a.dtype.itemsize not in (1, 8):
        raise ValueError("a column of %d-byte entries" % a.dtype.itemsize)
    return np.ascontiguousarray(a).view(np.uint8 if a.dtype.itemsize == 1 else np.uint64).tolist()


def device_fetch(ctx, what, info):
    """the fetch of a product or tenant -> canonical content.  info: what the build returned (the sizes the fetch needs)"""
    if what == "rows":
        return tuple(a.tolist() for a in ctx.fetch_rows(*info))
    if what == "column":
        off, data, st = ctx.fetch_path_strings(*info)
        return off.tolist(), data, st.tolist()
    if what == "list":
        if info[-1] != "s":
            off, vals, st = ctx.fetch_path_list(*info)
            return off.tolist(), _bits(vals), st.tolist()
        loff, soff, data, st = ctx.fetch_path_list_strings(*info[:3])
        return loff.tolist(), soff.tolist(), data, st.tolist()
    if what == "table":
        records, sizes, kinds = info
        out = []
        for c, kind in enumerate(kinds):
            col = ctx.fetch_table_column(c, records, kind, sizes[c])
            out.append((col[0].tolist(), col[1], col[2].tolist()) if kind >= S else (_bits(col[0]), col[1].tolist()))
        return out
    if what == "groups":
        g = info
        if isinstance(g.key_kind, list):
            g = ctx.fetch_group_paths(g)
            keys = [list(k) if kind == S else _bits(k) for k, kind in zip(g.keys, g.key_kind)]
            return ("many", keys, [k.tolist() for k in g.key_ok], [s.tolist() for s in g.status], g.first_row.tolist(), g.group_rows.tolist(),
                    g.codes.tolist(), [[_bits(a) for a in v] for v in g.values])
        g = ctx.fetch_groups(g)
        keys = list(g.keys) if g.key_kind == S else _bits(g.keys)
        aggs = None if g.value_kind is None else [_bits(a) for a in g.aggregates()]
        return ("one", keys, g.first_row.tolist(), g.group_rows.tolist(), g.codes.tolist(), g.status.tolist(), aggs, None)
    if what == "order":
        o = ctx.fetch_order(info)
        return o.order.tolist(), None if o.values is None else _bits(o.values), o.status.tolist()
    if what == "parents":
        return tuple(a.tolist() for a in ctx.fetch_row_parents(*info))
    import ctypes as C
    import sjhip
    L = sjhip.lib()
    if what == "filtered":
        n, sk, tl, sl = info
        tape, strings = np.empty(tl, dtype=np.uint64), np.empty(sl, dtype=np.uint8)
        ctx._check(L.sjhip_fetch_filtered(ctx._h, tape.ctypes.data, strings.ctypes.data))
        return n, sk, tape.tolist(), strings.tobytes()
    if what in ("marshaled", "marshaled_rows"):
        n, tl = info if isinstance(info, tuple) else (0, info)
        out, off = np.empty(max(tl, 1), dtype=np.uint8), np.empty(n + 1, dtype=np.uint64)
        if what == "marshaled":
            ctx._check(L.sjhip_fetch_marshaled(ctx._h, out.ctypes.data))
            return out[:tl].tobytes()
        ctx._check(L.sjhip_fetch_marshaled_rows(ctx._h, off.ctypes.data, out.ctypes.data))
        return out[:tl].tobytes(), off.tolist()
    if what == "serialized":
        out, got = np.empty(max(info, 1), dtype=np.uint8), C.c_size_t(0)
        ctx._check(L.sjhip_fetch_serialized(ctx._h, out.ctypes.data, out.size, C.byref(got)))
        return out[:got.value].tobytes()
    raise ValueError(what)


# sizes for the fetch of something that was never built: the smallest buffers (the fetch must fail before it copies)
def no_info(what):
    import sjhip
    return {"rows": (0, 0), "column": (0, 0), "list": (0, 0, I), "table": (0, [0], [I]), "groups": sjhip.api.Groups(0, 0, 0, S, None),
            "order": sjhip.api.Order(0, 0, I), "parents": (0, 0), "filtered": (0, 0, 0, 0), "marshaled": (0, 0), "marshaled_rows": (0, 0),
            "serialized": 0}[what]


def device_call(ctx, name, args):
    """one call of a chain on the device -> (ret, what it published or None, the info its fetch needs, content or None): the calls are
    made with fetch=False and fetched through device_fetch, so that an immediate and a late fetch take one route"""
    kw = dict(args[-1]) if args and isinstance(args[-1], dict) else {}
    pos = args[:-1] if args and isinstance(args[-1], dict) else args
    fetch = kw.pop("fetch", True)
    what, info, ret = PUBLISHES.get(name), None, None
    if name in ("select_rows", "where_path", "where_paths"):
        ret = getattr(ctx, name)(*pos, **kw)
    elif name == "select_records":
        ctx.select_records()
    elif name in ("unnest_rows", "unnest_members"):
        ret = getattr(ctx, name)(*pos)
        info = (ret[1], ret[2])
    elif name == "where_row_names":
        ret = ctx.where_row_names(*pos, **kw)
    elif name == "extract_row_names":
        ret = info = ctx.extract_row_names(fetch=False)
    elif name == "marshal_rows_paths":
        ret = info = ctx.marshal_rows_paths(*pos, fetch=False, **kw)
    elif name == "aggregate_path_records":
        return None, None, None, ("aggrec", pos[1], [_bits(a) for a in ctx.aggregate_path_records(*pos)], None)
    elif name == "count_where_paths":
        ret = ctx.count_where_paths(*pos)
    elif name in ("order_path", "order_path_strings", "order_paths"):
        info = getattr(ctx, name)(*pos, fetch=False, **kw)
        ret = (info.records, info.rows)
    elif name == "extract_path_strings":
        ret = info = ctx.extract_path_strings(*pos, fetch=False, **kw)
    elif name == "extract_path_list":
        ret = ctx.extract_path_list(*pos, fetch=False)
        info = ret + (pos[1],)
    elif name == "extract_path_list_strings":
        ret = ctx.extract_path_list_strings(*pos, fetch=False, **kw)
        info = ret + ("s",)
    elif name == "extract_table":
        ret = ctx.extract_table(*pos, fetch=False)
        info = ret + ([k for _, k in pos[0]],)
    elif name in ("group_path", "group_paths"):
        info = getattr(ctx, name)(*pos, fetch=False, **kw)
        ret = (info.rows, info.groups, info.key_bytes)
    elif name == "aggregate_path":
        a = ctx.aggregate_path(*pos)
        kind = pos[1]
        return None, None, None, ("agg", kind, a.rows, a.status, AW.bits_of(a.min, kind), AW.bits_of(a.max, kind), a.sum, None)
    elif name == "filter_rows":
        n, sk, (tl, sl) = ctx.filter_rows(fetch=False)
        ret = info = (n, sk, tl, sl)
    elif name == "marshal_rows":
        ret = info = ctx.marshal_rows(fetch=False)
    elif name == "marshal_json":
        ret = info = ctx.marshal_json(fetch=False)
    elif name == "serialize":
        ret = info = ctx.serialize(fetch=False)["stream"]
    else:
        raise ValueError(name)
    content = device_fetch(ctx, what, info) if fetch and what else None
    return ret, what, info, content


def device_invalid(ctx, name, args):
    """a call with an invalid argument -> the error code (it must be ERR_ARG).  args: (family, path, path): the family of the
    error and two paths of the document family for the arguments that are valid"""
    import sjhip
    family, pa, pb = args if isinstance(args, tuple) else (args, (b"a",), (b"b",))
    if family in INVALID_FAMILIES_M:
        return _device_invalid_m(ctx, name, family, pa, pb)
    bad = {"kind": 77, "path17": (b"k",) * 17}[family] if family != "program" else None
    try:
        if family == "program":
            preds = [(pa, Q.OP_EXISTS, None), (pb, Q.OP_EXISTS, None)]
            getattr(ctx, name[0])(preds, name[1])
        elif family == "kind":
            {"order_path": lambda: ctx.order_path(pa, bad), "extract_path_list": lambda: ctx.extract_path_list(pa, bad, fetch=False),
             "extract_table": lambda: ctx.extract_table([(pa, bad)], fetch=False), "group_path": lambda: ctx.group_path(pa, bad, fetch=False),
             "aggregate_path": lambda: ctx.aggregate_path(pa, bad),
             "order_paths": lambda: ctx.order_paths([(pa, I, False), (pb, bad, False)], fetch=False),
             "group_paths": lambda: ctx.group_paths([(pa, S), (pb, bad)], fetch=False)}[name]()
        else:
            {"select_rows": lambda: ctx.select_rows(bad), "where_path": lambda: ctx.where_path(bad, Q.OP_EXISTS),
             "unnest_rows": lambda: ctx.unnest_rows(bad), "order_path": lambda: ctx.order_path(bad, I, fetch=False),
             "order_path_strings": lambda: ctx.order_path_strings(bad, fetch=False),
             "extract_path_strings": lambda: ctx.extract_path_strings(bad, fetch=False),
             "extract_path_list": lambda: ctx.extract_path_list(bad, I, fetch=False),
             "extract_table": lambda: ctx.extract_table([(bad, I)], fetch=False), "group_path": lambda: ctx.group_path(bad, S, fetch=False),
             "aggregate_path": lambda: ctx.aggregate_path(bad, I)}[name]()
    except sjhip.ParseError as e:
        return e.code
    return 0


def _device_invalid_m(ctx, name, family, a, b):
    """the families of the member and projection calls.  not_members (name: extract_row_names or where_row_names; a, b: an
    operator and a value): the selection in force is not one of members -- the error must say so, else the code comes back
    negated; name_op (name: where_row_names; a: an operator the names do not take, b: a value); project (name:
    marshal_rows_paths; a: the form -- PROJECT_FORMS --, b: a path that is valid)"""
    import ctypes as C
    import sjhip
    try:
        if family == "project":
            if a == "flag":  # (Context.marshal_rows_paths cannot express an unknown flag bit)
                lens, n, tl = (C.c_uint32 * 1)(len(b[0])), C.c_uint64(0), C.c_size_t(0)
                return sjhip.lib().sjhip_marshal_rows_paths(ctx._h, bytes(b[0]), lens, (C.c_uint32 * 1)(1), 1, None, None, 2, C.byref(n), C.byref(tl))
            columns = {"cols17": [b] * 17, "empty_unnamed": [b, ()], "no_selection": [b]}[a]
            ctx.marshal_rows_paths(columns, fetch=False)
        elif name == "extract_row_names":
            ctx.extract_row_names(fetch=False)
        else:
            ctx.where_row_names(a, b)
    except sjhip.ParseError as e:
        if family == "not_members" and NOT_MEMBERS not in ctx.last_error():
            return -e.code
        return e.code
    return 0


KIND_CALLS = ("order_path", "extract_path_list", "extract_table", "group_path", "aggregate_path", "order_paths", "group_paths")
PATH17_CALLS = ("select_rows", "where_path", "unnest_rows", "order_path", "order_path_strings", "extract_path_strings", "extract_path_list",
                "extract_table", "group_path", "aggregate_path")


def differs(got, want):
    """None, or where a fetched content differs from the model's (floats sums by the model's bound, everything else exactly)"""
    if isinstance(want, tuple) and want and want[0] == "agg":
        if got[:6] != want[:6]:
            return "aggregate: %r != %r" % (got[:6], want[:6])
        if want[1] != F:
            return None if got[6] == want[6] else "aggregate: sum %r != %r" % (got[6], want[6])
        return _sum_differs(got[6], want[6], want[7], "aggregate")
    if isinstance(want, tuple) and want and want[0] == "aggrec":
        g, w = [list(a) for a in got[2]], [list(a) for a in want[2]]
        if want[3] is not None:  # the float sums of the records: by each record's bound
            for r, (a, b, bound) in enumerate(zip(g[2], w[2], want[3])):
                bad = _sum_differs(CW.bits2f(a), CW.bits2f(b), bound, "record %d" % r)
                if bad:
                    return bad
            g[2] = w[2] = None
        return None if (got[1], g) == (want[1], w) else "aggregate per record: %.300r != %.300r" % (g, w)
    if isinstance(want, tuple) and want and want[0] == "one" and want[7] is not None:
        g, w = list(got), list(want)
        for k, (fsum, bound) in enumerate(w[7]):
            bad = _sum_differs(CW.bits2f(g[6][2][k]), fsum, bound, "group %d" % k)
            if bad:
                return bad
        g[6], w[6] = g[6][:2] + g[6][3:], w[6][:2] + w[6][3:]
        g[7] = w[7] = None
        got, want = tuple(g), tuple(w)
    if got == want:
        return None
    if type(got) is type(want) and isinstance(want, (tuple, list)) and len(got) == len(want):
        for k, (a, b) in enumerate(zip(got, want)):
            if a != b:
                inner = differs(a, b) if isinstance(b, (tuple, list)) and b and isinstance(b[0], (tuple, list)) else None
                if inner:
                    return "[%d]%s" % (k, inner)
                if isinstance(b, (list, bytes)) and isinstance(a, (list, bytes)) and len(a) == len(b):
                    at = next(i for i in range(len(b)) if a[i] != b[i])
                    return "[%d] first difference at entry %d: %r != %r" % (k, at, a[at], b[at])
                return "[%d]: %.200r != %.200r" % (k, a, b)
    return "%.300r != %.300r" % (got, want)


def _sum_differs(got, want, bound, what):
    if bound is None:
        return None if CW.f2bits(float(got)) == CW.f2bits(float(want)) else "%s: float sum %r != %r (bits)" % (what, got, want)
    return None if abs(got - want) <= bound else "%s: float sum %r, fsum %r, bound %r" % (what, got, want, bound)


class ChainError(AssertionError):
    pass


def run_chain(ctx, model, steps, header=""):
    """Applies every step to the device and to the model and compares: return values, fetch_rows after every selection call, every
    fetched content; at the end every live product and the live tenant once more, then select_records and find_path on the records.
    A difference raises ChainError naming the first step that differed, with the replay script."""
    info = {}

    def fail(k, why):
        raise ChainError("%s\nstep %d %r: %s\nreplay:\n%s" % (header, k, steps[k] if k < len(steps) else "end", why, script(steps[:k + 1], header)))

    def fetched(k, what):
        import sjhip
        try:
            got = device_fetch(ctx, what, info[what.replace("_rows", "") if what == "marshaled_rows" else what])
        except sjhip.ParseError as e:
            fail(k, "fetch of %s failed: %s" % (what, e))
        bad = differs(got, model.content(what))
        if bad:
            fail(k, "late fetch of %s: %s" % (what, bad))

    for k, step in enumerate(steps):
        import sjhip
        do, name, args = step
        want = model.apply(step)
        if do == "fetch":
            fetched(k, name)
            continue
        if do == "refused":
            try:
                device_fetch(ctx, name, info.get("marshaled" if name == "marshaled_rows" else name) or no_info(name))
                fail(k, "the fetch of %s succeeded; it must be refused" % name)
            except sjhip.ParseError as e:
                if e.code != ERR_ARG:
                    fail(k, "the refused fetch returned %d" % e.code)
        elif do == "invalid":
            code = device_invalid(ctx, name, args)
            if code != ERR_ARG:
                fail(k, "the invalid call returned %d, not SJHIP_ERR_ARG" % code)
        else:
            try:
                ret, what, inf, content = device_call(ctx, name, args)
            except sjhip.ParseError as e:
                fail(k, "the call failed: %s" % e)
            if what:
                info[what] = inf
            if want.ret is not None and _plain(ret) != _plain(want.ret):
                fail(k, "returned %r, the model %r" % (ret, want.ret))
            if want.content is not None:
                bad = differs(content, model.content(what) if what else want.content)
                if bad:
                    fail(k, "immediate fetch: %s" % bad)
        if do == "call" and name == "select_records":  # the rows are gone: their fetch must be refused
            try:
                device_fetch(ctx, "rows", info.get("rows") or no_info("rows"))
                fail(k, "fetch_rows succeeded behind select_records; it must be refused")
            except sjhip.ParseError as e:
                if e.code != ERR_ARG:
                    fail(k, "fetch_rows behind select_records returned %d" % e.code)
        if do in ("refused", "invalid") or name in SELECTION_CALLS_M:  # the selection, and after a refusal everything that lives
            if model.sel is not None:
                info["rows"] = (model.n_records, len(model.sel[1]))
                fetched(k, "rows")
            if do in ("refused", "invalid"):
                for what in live_things(model):
                    fetched(k, what)
    for what in live_things(model):
        fetched(len(steps), what)
    ctx.select_records()
    got = ctx.find_path(b"a").tolist()
    if got != [model.w.find_path(r, [b"a"]) for r in model.w.records()]:
        fail(len(steps), "find_path on the records after select_records differs")


def _plain(x):
    return [_plain(y) for y in x] if isinstance(x, (tuple, list)) else x


def live_things(model):
    out = [p for p in PRODUCTS if p in model.live]
    if model.tenant:
        out.append(model.tenant[0])
        if model.tenant[2]:
            out.append("marshaled_rows")
    return out


def script(steps, header=""):
    """the chain as lines of Python that replay it on a Context `ctx` that has parsed the document (tests/ on sys.path)"""
    lines = ["# " + header, "import chain_model as CM", "info = {}"]
    for k, (do, name, args) in enumerate(steps):
        if do == "call":
            lines.append("r%d = CM.device_call(ctx, %r, %r); info[r%d[1]] = r%d[2]" % (k, name, args, k, k))
        elif do == "invalid":
            lines.append("r%d = CM.device_invalid(ctx, %r, %r)  # must be %d" % (k, name, args, ERR_ARG))
        else:
            lines.append("r%d = CM.device_fetch(ctx, %r, info.get(%r) or CM.no_info(%r))%s" % (k, name, name, name, "  # must be refused" if do == "refused" else ""))
    return "\n".join(lines)


# ---- the document families ------------------------------------------------------------------------------------------------------------
class Family:
    """doc, nd; base: the path of the rows; per level (0: records, 1: the rows at base, 2 and 3: behind one and two unnests) the
    paths the generator draws from: num [(path, kind)], strs [path], arrays [path] (what unnest_rows / the lists take), preds
    [(path, op, value)]; exact: the FLOAT paths whose partial sums are all exact.  For the extended generator a level may also list
    objects [path] (what unnest_members takes; without the entry: the row itself and "a") and to {("rows" | "members", path): the
    level behind that unnest}; a level is a number or a name of NAMED_LEVELS ("mixed": rows of every kind, reached where nothing
    else is said).  select: (path, level) of the generator's select_rows where base is None"""

    def __init__(self, doc, nd, base, levels, exact=(), select=((), 1)):
        self.doc, self.nd, self.base, self.levels, self.exact, self.select = doc, nd, base, levels, exact, select


_RANDOM_LEVEL = dict(
    num=[((b"a",), I), ((b"b",), U), ((b"a", b"b"), I), ((b"c",), I), ((b"",), U)],
    strs=[(b"a",), (b"b",), (b"a", b"b"), (b'a"q',)],
    arrays=[(b"a",), (b"b",), (b"c",)],
    preds=[((b"a",), Q.OP_EXISTS, None), ((b"b",), Q.OP_EXISTS, None), ((b"b",), WW.OP_GE_FLOAT, 0.0), ((b"a",), WW.OP_LT_INT, 100),
           ((b"c",), Q.OP_EXISTS, None), ((b"a",), WW.OP_PREFIX_STRING, b""), ((b"a", b"b"), Q.OP_EXISTS, None), ((b"",), Q.OP_EXISTS, None)])


def _nested_doc(seed, n):
    """NDJSON lines {"k","g","items":[...]}: 0 to 7 items a line, n items in all; an item owns "subs", objects that own "w", arrays of
    integers; string keys with ties and prefixes, numeric keys of the three kinds, members missing, null or of the wrong type"""
    rnd = random.Random(seed)
    names = ["", "a", "ab", "abc", "abcdefg", "abcdefgh", "abcdefghijklmno", "b", "ba", "caf\\u00e9", "z" * 20]
    lines, made, k = [], 0, 0
    while made < n:
        take = min((k * 5) % 8, n - made)
        items = []
        for _ in range(take):
            subs = []
            for _ in range(rnd.randint(0, 4)):
                ws = ",".join(str(rnd.randint(-50, 50)) for _ in range(rnd.randint(0, 3)))
                v = rnd.choice([str(rnd.randint(0, 9)), "null", '"x"', "1.5"])
                subs.append('{"v":%s,"w":[%s],"s":"%s"}' % (v, ws, rnd.choice(names)) if rnd.random() < 0.9 else rnd.choice(["7", "null", "[1]"]))
            m = ['"id":%d' % (made * 3 % 97)]
            if rnd.random() < 0.9:
                m.append('"name":%s' % rnd.choice(['"%s"' % rnd.choice(names), '"%s"' % rnd.choice(names), "null", "3"]))
            if rnd.random() < 0.9:
                m.append('"u":%s' % rnd.choice([str(rnd.randint(2 ** 63, 2 ** 64 - 1)), str(rnd.randint(0, 5)), "-1", '"u"']))
            if rnd.random() < 0.9:
                m.append('"q":%s' % rnd.choice([str(rnd.randint(-64, 64) / 4), str(rnd.randint(-9, 9)), "null"]))
            if rnd.random() < 0.9:
                m.append('"x":%s' % rnd.choice([repr(rnd.uniform(-1e6, 1e6)), "0.1", "1e-7", '"f"']))
            m.append('"tags":[%s]' % ",".join('"t%d"' % rnd.randint(0, 5) for _ in range(rnd.randint(0, 3))))
            m.append('"subs":%s' % ("[%s]" % ",".join(subs) if rnd.random() < 0.92 else rnd.choice(["null", "{}", "5"])))
            items.append("{%s}" % ",".join(m))
            made += 1
        lines.append('{"k":%d,"g":"%s","items":[%s]}' % (k, rnd.choice(names[:4]), ",".join(items)))
        k += 1
    return "\n".join(lines).encode()


_NESTED_LEVELS = [
    dict(num=[((b"k",), I)], strs=[(b"g",)], arrays=[(b"items",)], preds=[((b"k",), WW.OP_GE_INT, 3), ((b"g",), WW.OP_PREFIX_STRING, b"a")]),
    dict(num=[((b"id",), I), ((b"u",), U), ((b"q",), F), ((b"x",), F), ((b"id",), U)], strs=[(b"name",), (b"id",)],
         arrays=[(b"subs",), (b"tags",)],
         preds=[((b"id",), WW.OP_GE_INT, 30), ((b"name",), WW.OP_PREFIX_STRING, b"ab"), ((b"q",), WW.OP_LT_FLOAT, 4.0),
                ((b"u",), WW.OP_GT_UINT, 5), ((b"name",), Q.OP_IS_NULL, None), ((b"subs",), Q.OP_EXISTS, None)]),
    dict(num=[((b"v",), I), ((b"v",), F), ((), I)], strs=[(b"s",), ()], arrays=[(b"w",)],
         preds=[((b"v",), WW.OP_GE_INT, 3), ((b"s",), WW.OP_PREFIX_STRING, b"a"), ((b"w",), Q.OP_EXISTS, None), ((), Q.OP_EXISTS, None)]),
    dict(num=[((), I), ((), F)], strs=[()], arrays=[()], preds=[((), WW.OP_GE_INT, 0), ((), WW.OP_LT_INT, 25)])]

_TWITTER_LEVELS = [
    dict(num=[((b"search_metadata", b"count"), I)], strs=[(b"search_metadata", b"query")], arrays=[(b"statuses",)],
         preds=[((b"search_metadata", b"count"), WW.OP_GE_INT, 1)]),
    dict(num=[((b"id",), I), ((b"retweet_count",), U), ((b"user", b"followers_count"), I), ((b"favorite_count",), F)],
         strs=[(b"user", b"screen_name"), (b"lang",), (b"text",), (b"created_at",)],
         arrays=[(b"entities", b"user_mentions"), (b"entities", b"hashtags"), (b"entities", b"urls")],
         preds=[((b"retweet_count",), WW.OP_GE_INT, 1), ((b"lang",), Q.OP_EQ_STRING, b"ja"), ((b"user", b"followers_count"), WW.OP_LT_INT, 500),
                ((b"in_reply_to_status_id",), Q.OP_IS_NULL, None), ((b"entities", b"user_mentions"), Q.OP_EXISTS, None)]),
    dict(num=[((b"id",), I), ((b"id",), U)], strs=[(b"screen_name",), (b"text",), (b"name",)], arrays=[(b"indices",)],
         preds=[((b"id",), WW.OP_GE_INT, 200000000), ((b"indices",), Q.OP_EXISTS, None), ((b"screen_name",), WW.OP_PREFIX_STRING, b"a")]),
    dict(num=[((), I), ((), U)], strs=[()], arrays=[()], preds=[((), WW.OP_GE_INT, 20), ((), WW.OP_LT_INT, 60)])]

FAMILIES = ("wrapped_random", "random_nd", "nested", "twitter")
FAMILIES_M = FAMILIES + ("catalog",)

# the rows behind an unnest the levels say nothing about: values of every kind (no FLOAT column: its sums would not be exact)
_MIXED_LEVEL = dict(num=[((), I), ((), U), ((b"id",), I)], strs=[(), (b"name",)], arrays=[(), (b"w",)], objects=[(), (b"loc",)],
                    preds=[((), Q.OP_EXISTS, None), ((), WW.OP_GE_INT, 3), ((), Q.OP_IS_NULL, None), ((), WW.OP_PREFIX_STRING, b"a"),
                           ((b"id",), Q.OP_EXISTS, None)])
CATALOG_NAMES = [b"", b'q"uote', b"back\\slash", "caf\u00e9".encode(), b"ab", b"abc", b"abcd", b"n" * 512]  # unescaped, as the rows carry them
_CATALOG_SPELLED = ['', 'q\\"uote', 'back\\\\slash', 'caf\\u00e9', 'ab', 'abc', 'abcd', 'n' * 512]   # ... and as the document spells them


def _catalog_doc(seed, n):
    """NDJSON lines {"k","g","t":[...],"events":{"<id>":{...},...},"venues":{...}}: 0 to 7 members of "events" a line, n in all.
    A member's value is mostly a record {"id","u","q","name","tags":[...],"loc":{...}} -- numbers of the three kinds, strings with
    ties and prefixes, an inner array, an inner object --, sometimes a scalar, null or an array; a line without members has
    "events" null, a scalar, an array, {} or absent.  The names: ids, and at members 3, 10, 17, ... one each of CATALOG_NAMES (the
    empty name, escapes, prefixes of each other, 512 bytes); now and then the name of the member in front once more."""
    rnd = random.Random(seed)
    words = ["", "a", "ab", "abc", "abcdefg", "abcdefgh", "b", "ba", "caf\\u00e9", "z" * 20]
    lines, made, k = [], 0, 0
    while made < n:
        take = min((k * 5) % 8, n - made)
        members, name = [], None
        for j in range(take):
            if made % 7 == 3 and made // 7 < len(_CATALOG_SPELLED):
                name = _CATALOG_SPELLED[made // 7]
            elif not (j and rnd.random() < 0.1):  # (else: a duplicate of the name in front)
                name = str(10 ** rnd.randint(2, 8) + made * 7)
            tags = ",".join(rnd.choice(['"t%d"' % rnd.randint(0, 5), str(rnd.randint(-50, 50)), '{"id":%d}' % rnd.randint(0, 9)]) for _ in range(rnd.randint(0, 3)))
            loc = '{"x":%d,"y":%d,"city":"%s"}' % (rnd.randint(-9, 9), rnd.randint(0, 99), rnd.choice(words)) if rnd.random() < 0.85 else rnd.choice(["null", "{}", "5"])
            m = ['"id":%d' % (made * 3 % 97)]
            if rnd.random() < 0.9:
                m.append('"u":%s' % rnd.choice([str(rnd.randint(2 ** 63, 2 ** 64 - 1)), str(rnd.randint(0, 5)), "-1", '"u"']))
            if rnd.random() < 0.9:
                m.append('"q":%s' % rnd.choice([str(rnd.randint(-64, 64) / 4), str(rnd.randint(-9, 9)), "null"]))
            if rnd.random() < 0.9:
                m.append('"name":%s' % rnd.choice(['"%s"' % rnd.choice(words), '"%s"' % rnd.choice(words), "null", "3"]))
            m += ['"tags":[%s]' % tags, '"loc":%s' % loc]
            value = "{%s}" % ",".join(m) if rnd.random() < 0.88 else rnd.choice(["7", "null", '"s"', "[1,2]", "{}"])
            members.append('"%s":%s' % (name, value))
            made += 1
        events = '"events":{%s},' % ",".join(members) if take else rnd.choice(['"events":null,', '"events":7,', '"events":[{"id":1}],', '"events":{},', ""])
        venues = ",".join('"v%d":{"cap":%d,"city":"%s"}' % (rnd.randint(0, 9), rnd.randint(0, 500), rnd.choice(words)) for _ in range(rnd.randint(0, 2)))
        ts = ",".join(str(rnd.randint(-50, 50)) for _ in range(rnd.randint(0, 3)))
        lines.append('{"k":%d,"g":"%s","t":[%s],%s"venues":{%s}}' % (k, rnd.choice(words[:4]), ts, events, venues))
        k += 1
    return "\n".join(lines).encode()


_CATALOG_LEVELS = [
    dict(num=[((b"k",), I)], strs=[(b"g",)], arrays=[(b"t",)], objects=[(b"events",), (b"venues",)],
         preds=[((b"k",), WW.OP_GE_INT, 3), ((b"g",), WW.OP_PREFIX_STRING, b"a"), ((b"events",), Q.OP_EXISTS, None)],
         to={("members", (b"events",)): "event", ("members", (b"venues",)): "venue", ("rows", (b"t",)): "mixed"})] + [_MIXED_LEVEL] * 3
NAMED_LEVELS = {
    "mixed": _MIXED_LEVEL,
    "event": dict(num=[((b"id",), I), ((b"u",), U), ((b"q",), F), ((b"loc", b"x"), I), ((b"id",), U)], strs=[(b"name",), (b"loc", b"city")],
                  arrays=[(b"tags",)], objects=[(b"loc",), ()],
                  preds=[((b"id",), WW.OP_GE_INT, 30), ((b"name",), WW.OP_PREFIX_STRING, b"ab"), ((b"q",), WW.OP_LT_FLOAT, 4.0),
                         ((b"u",), WW.OP_GT_UINT, 5), ((b"name",), Q.OP_IS_NULL, None), ((b"loc",), Q.OP_EXISTS, None)]),
    "venue": dict(num=[((b"cap",), I), ((b"cap",), U)], strs=[(b"city",)], arrays=[(b"none",)], objects=[()],
                  preds=[((b"cap",), WW.OP_GE_INT, 100), ((b"city",), WW.OP_PREFIX_STRING, b"a")])}
# the member draws of the first families: every field of an item or of a subs element; a status' user and entities
_MEMBER_OBJECTS = {"nested": {1: [()], 2: [()]}, "twitter": {1: [(b"user",), (b"entities",)]}}


@functools.lru_cache(maxsize=8)
def family(name, seed, rows):
    if name == "wrapped_random":
        from test_gpu_rows import wrapped_random
        return Family(wrapped_random(seed, rows), True, (b"items",), [dict(_RANDOM_LEVEL, arrays=[(b"items",)])] + [_RANDOM_LEVEL] * 3)
    if name == "random_nd":  # the records are the rows; the array roots give select_rows(()) something
        from test_gpu_columns import random_nd
        return Family(random_nd(seed, rows), True, None, [_RANDOM_LEVEL] * 4)
    if name == "nested":
        return Family(_nested_doc(seed, rows), True, (b"items",), _NESTED_LEVELS, exact=[(b"q",), (b"v",), (), (b"id",)])
    if name == "twitter":
        return Family(fixtures.load("twitter"), False, (b"statuses",), _TWITTER_LEVELS, exact=[(b"favorite_count",)])
    if name == "catalog":
        return Family(_catalog_doc(seed, rows), True, None, _CATALOG_LEVELS, exact=[(b"q",)], select=((b"t",), "mixed"))
    raise ValueError(name)


@functools.lru_cache(maxsize=4)
def walk_of(name, seed, rows, copy):
    fam = family(name, seed, rows)
    ref = O.parse(fam.doc, ndjson=fam.nd, copy_strings=copy)
    assert ref.rc == 0
    return Q.Walk(ref.tape, ref.strings, fam.doc[ref.msg_off:ref.msg_off + ref.msg_len]), ref


def model_of(name, seed, rows, copy):
    w, ref = walk_of(name, seed, rows, copy)
    return Model(w, ref, family(name, seed, rows).exact)


# ---- the generator ----------------------------------------------------------------------------------------------------------------------
def chain_rows(seed, name):
    """the row count of a chain: the seams, plus a few hundred in between"""
    rnd = random.Random(seed * 7919 + 13)
    return 100 if name == "twitter" else (SIZES + (rnd.randint(100, 900),))[(seed + seed // 4) % 8]


class _Gen:
    def __init__(self, seed, name, copy, steps):
        self.rnd, self.name, self.copy, self.n = random.Random(seed), name, copy, steps
        self.fam = family(name, seed, chain_rows(seed, name))
        self.model = model_of(name, seed, chain_rows(seed, name), copy)
        self.steps, self.level = [], 0

    def full(self):
        return len(self.steps) >= self.n

    def emit(self, do, name, *args):
        if self.full():
            return False
        step = (do, name, args if do == "call" else (args[0] if args else ()))
        self.model.apply(step)
        self.steps.append(step)
        return True

    def V(self):
        return self.fam.levels[min(self.level, 3)]

    # ---- selection calls ----
    def select(self):
        if self.fam.base is None:
            self.level = 0
            return self.emit("call", "select_records")
        self.level = 1
        return self.emit("call", "select_rows", self.fam.base)

    def narrow(self, kind=None):
        rnd, V = self.rnd, self.V()
        kind = kind or rnd.choice(("where", "where", "wheres", "order", "orders", "orderm"))
        rows = self.model.rows()
        limit = max(rows * rnd.choice((2, 3)) // 4, 1) if rows > 3 else 0
        if kind == "where":
            path, op, val = rnd.choice(V["preds"])
            return self.emit("call", "where_path", path, op, val, {"negate": rnd.random() < 0.25})
        if kind == "wheres":
            a, b = rnd.choice(V["preds"]), rnd.choice(V["preds"])
            return self.emit("call", "where_paths", [a, b], rnd.choice((bytes([0, 1, OR]), bytes([0, 1, NEG, OR]), bytes([0, NEG, 1, AND, NEG]))))
        if kind == "order":
            path, k = rnd.choice(V["num"])
            return self.emit("call", "order_path", path, k, {"descending": rnd.random() < 0.5, "limit": limit, "fetch": rnd.random() < 0.5})
        if kind == "orders":
            return self.emit("call", "order_path_strings", rnd.choice(V["strs"]), {"descending": rnd.random() < 0.5, "limit": limit, "fetch": rnd.random() < 0.5})
        (p0, k0), p1 = rnd.choice(V["num"]), rnd.choice(V["strs"])
        cols = [(p1, S, rnd.random() < 0.5), (p0, k0, rnd.random() < 0.5)]
        return self.emit("call", "order_paths", cols if rnd.random() < 0.5 else cols[::-1], {"limit": limit, "fetch": rnd.random() < 0.5})

    def unnest(self):
        path = self.V()["arrays"][0] if self.rnd.random() < 0.8 else self.rnd.choice(self.V()["arrays"])
        ok = self.emit("call", "unnest_rows", path)
        self.level = max(self.level, 1) + 1 if self.fam.base is not None or self.level else 1
        return ok

    # ---- builds ----
    def build(self, what=None, fetch=None):
        rnd, V = self.rnd, self.V()
        what = what or rnd.choice(("column", "list", "table", "groups", "groups", "agg"))
        kw = {"fetch": rnd.random() < 0.4 if fetch is None else fetch}
        if what == "column":
            paths = [p for p in V["strs"] + [q for q, _ in V["num"]] if len(p)] or [(b"a",)]
            return self.emit("call", "extract_path_strings", rnd.choice(paths), dict(kw, cvt=rnd.random() < 0.5))
        if what == "list":
            paths = [p for p in V["arrays"] if len(p)] or [(b"a",)]
            if rnd.random() < 0.5:
                return self.emit("call", "extract_path_list", rnd.choice(paths), rnd.choice((F, I, U)), kw)
            return self.emit("call", "extract_path_list_strings", rnd.choice(paths), dict(kw, cvt=rnd.random() < 0.7))
        if what == "table":
            cols = [(p, k) for p, k in V["num"][:3] if len(p)] + [(p, rnd.choice((S, SC))) for p in V["strs"][:2] if len(p)]
            if not cols:
                return self.build("column", fetch)
            return self.emit("call", "extract_table", cols, kw)
        if what == "groups":
            ints = [(p, k) for p, k in V["num"] if k in (I, U)]
            if rnd.random() < 0.5:
                key = rnd.choice([(p, S) for p in V["strs"]] + [(p, I) for p, _ in ints])
                val = rnd.choice(V["num"] + [None])
                return self.emit("call", "group_path", key[0], key[1], *(val if val else (None, None)), kw)
            keys = [(rnd.choice(V["strs"]), S, True), rnd.choice(ints) + (rnd.random() < 0.5,)]
            return self.emit("call", "group_paths", keys, ints[:2], kw)
        path, k = rnd.choice(V["num"])
        return self.emit("call", "aggregate_path", path, k)

    def tenant(self, what=None, fetch=None):
        rnd = self.rnd
        kw = {"fetch": rnd.random() < 0.4 if fetch is None else fetch}
        choices = ["marshal_rows", "marshal_json"] + (["filter_rows", "filter_rows", "serialize", "serialize"] if self.copy else ["marshal_rows"])
        what = what or rnd.choice(choices)
        if what in ("filter_rows", "marshal_rows") and self.model.sel is None:
            what = "marshal_json"
        return self.emit("call", what, kw)

    def fetch_live(self, what=None):
        live = live_things(self.model)
        if what is None and live:
            what = self.rnd.choice(live)
        if what and self.model.exists(what):
            return self.emit("fetch", what)
        return False

    def refused(self, what=None):
        gone = [f for f in FETCHES if not self.model.exists(f)]
        what = what if what in gone else (self.rnd.choice(gone) if gone else None)
        return bool(what) and self.emit("refused", what)

    def invalid(self):
        fam = self.rnd.choice(INVALID_FAMILIES)
        paths = [p for p in self.V()["strs"] + [q for q, _ in self.V()["num"]] if len(p)] or [(b"a",)]
        args = (fam, self.rnd.choice(paths), self.rnd.choice(paths))
        if fam == "program":
            return self.emit("invalid", (self.rnd.choice(("where_paths", "count_where_paths")), self.rnd.choice(BAD_PROGRAMS)), args)
        return self.emit("invalid", self.rnd.choice(KIND_CALLS if fam == "kind" else PATH17_CALLS), args)

    # ---- the scenarios the generator is biased towards ----
    def s_build_change_fetch(self):
        what = self.rnd.choice(("column", "list", "table", "groups"))
        self.build(what, fetch=False)
        self.rnd.choice((self.narrow, self.narrow, self.select, self.unnest))()
        if self.rnd.random() < 0.2:
            self.fetch_live("rows")
        self.fetch_live(what)

    def s_grow(self):
        what = self.rnd.choice(("column", "list", "table", "groups"))
        others = [p for p in ("column", "list", "table", "groups") if p != what]
        self.rnd.shuffle(others)
        self.narrow("where")
        self.build(what, fetch=False)
        for p in others[:2]:
            if p not in self.model.live:
                self.build(p, fetch=False)
        self.select()
        self.build(what, fetch=self.rnd.random() < 0.5)
        for p in others[:2]:
            self.fetch_live(p)

    def s_unnest_behind(self):
        self.narrow(self.rnd.choice(("order", "orders", "orderm", "where", "wheres")))
        self.unnest()
        self.build()
        self.narrow()
        self.fetch_live(self.rnd.choice(("parents", "parents", "order")))

    def s_two_tenants(self):
        if self.model.sel is None:
            self.narrow("where")
        avail = ("filter_rows", "marshal_rows", "serialize", "marshal_json") if self.copy else ("marshal_rows", "marshal_json")
        first = self.rnd.choice(avail[:2] if self.copy else avail[:1])
        self.tenant(first, fetch=False)
        second = self.rnd.choice([t for t in avail if t != first])
        self.narrow()
        self.tenant(second, fetch=False)
        if PUBLISHES[second] != PUBLISHES[first]:
            self.refused(PUBLISHES[first])
        elif first == "marshal_rows":
            self.refused("marshaled_rows")
        self.fetch_live(PUBLISHES[second])

    def s_tenant_change_fetch(self):
        if self.model.sel is None:
            self.narrow("where")
        what = self.rnd.choice(("filter_rows", "serialize", "marshal_rows") if self.copy else ("marshal_rows", "marshal_json"))
        self.tenant(what, fetch=False)
        self.rnd.choice((self.narrow, self.select, self.select))()
        self.build(self.rnd.choice(("column", "list", "table", "groups")))
        self.fetch_live("marshaled_rows" if what == "marshal_rows" and self.rnd.random() < 0.5 else PUBLISHES[what])

    def s_order_change_fetch(self):
        self.narrow(self.rnd.choice(("order", "orders", "orderm")))
        self.rnd.choice((self.narrow, self.select, self.unnest))()
        self.fetch_live("order")

    def s_rows_late(self):
        self.narrow()
        self.build("table", fetch=False)
        self.build(self.rnd.choice(("groups", "column", "list")))
        self.fetch_live("rows")

    def s_three_narrowings(self):
        for _ in range(3):
            self.narrow()
        self.build()

    def s_unnest_twice(self):
        self.select()
        self.unnest()
        self.build(fetch=False)
        self.unnest()
        self.fetch_live()

    def s_empty(self):
        self.emit("call", "where_path", (b"nope", b"nope"), Q.OP_EXISTS, None, {})
        self.build()
        self.select()

    def run(self):
        rnd = self.rnd
        if rnd.random() < 0.8:
            self.select()
        scenarios = [self.s_build_change_fetch] * 3 + [self.tenant] + [self.s_grow] * 3 + [self.s_unnest_behind] * 2 + [self.s_two_tenants] * 2 + [self.s_tenant_change_fetch] * 3 + [self.s_order_change_fetch] * 2 + [self.s_rows_late] + \
            [self.s_three_narrowings] * 2 + [self.s_unnest_twice, self.invalid, self.invalid, self.refused, self.s_empty]
        while not self.full():
            if self.model.sel is not None and not self.model.sel[1]:  # an empty selection is left at once
                self.select()
            rnd.choice(scenarios)()
        return self.steps


PROJECT_NAMES = (b"", b'q"\\', b"n", b"id", b"caf\xc3\xa9", b"a\nb", b"x" * 40, b"id")  # (b"id" twice: names may repeat)
NOT_NAME_OPS = (Q.OP_EXISTS, Q.OP_IS_NULL, WW.OP_GE_INT, WW.OP_LT_FLOAT)


class _GenM(_Gen):
    """the extended generator: _Gen's calls and scenarios, and the member rows, the row names, the projection and the two readers.
    (_Gen itself draws what it always drew: chain_model.CHAINS is pinned by a digest in tests/test_chain_model.py.)"""

    def emit(self, do, name, *args):
        """_Gen.emit, and what trace_m reports of the step"""
        if self.full():
            return False
        m = self.model
        self.facts, self.expects = getattr(self, "facts", []), getattr(self, "expects", [])
        was, rows_before = m.members, None if m.sel is None else len(m.sel[1])
        step = (do, name, args if do == "call" else (args[0] if args else ()))
        self.steps.append(step)
        self.expects.append((m.apply(step), m.sel, dict(m.live), m.tenant, m.members))  # (the model replaces what it holds, never edits it)
        names, ok_parents = set(), None
        if (do, name) == ("call", "unnest_members"):
            ns, (_, parent, status) = m.names(), m.live["parents"]
            names = {what for what, hit in (("empty", b"" in ns), ("duplicate", len(set(zip(parent, ns))) < len(ns)),
                                            ("escaped", any(n in CATALOG_NAMES[1:4] for n in ns)), ("long", any(len(n) == 512 for n in ns))) if hit}
            ok_parents = sum(st == CW.COL_OK for st in status)
        self.facts.append(dict(step=step, rows=None if m.sel is None else len(m.sel[1]), rows_before=rows_before,
                               members=m.members, was_members=was, origin=dict(m.origin), names=names, ok_parents=ok_parents))
        return True

    def V(self):
        V = NAMED_LEVELS[self.level] if isinstance(self.level, str) else self.fam.levels[min(self.level, 3)]
        extra = _MEMBER_OBJECTS.get(self.name, {}).get(self.level)
        if extra or "objects" not in V:
            V = dict(V, objects=extra or [(), (b"a",)])
        return V

    def behind(self, kind, path):
        to = self.V().get("to", {}).get((kind, tuple(path)))
        if to is not None:
            return to
        if kind == "rows" and not isinstance(self.level, str):
            return max(self.level, 1) + 1 if self.fam.base is not None or self.level else 1
        return "mixed"

    # ---- selection calls ----
    def select(self):
        if self.fam.base is None and self.rnd.random() < 0.5:
            path, self.level = self.fam.select
            return self.emit("call", "select_rows", path)
        return _Gen.select(self)

    def unnest(self):
        path = self.V()["arrays"][0] if self.rnd.random() < 0.8 else self.rnd.choice(self.V()["arrays"])
        level = self.behind("rows", path)
        ok = self.emit("call", "unnest_rows", path)
        self.level = level
        return ok

    def members(self, path=None):
        objs = self.V()["objects"]
        path = path if path is not None else (objs[0] if self.rnd.random() < 0.7 else self.rnd.choice(objs))
        level = self.behind("members", path)
        ok = self.emit("call", "unnest_members", path)
        self.level = level
        return ok

    def to_members(self):
        """a member selection that has rows, where the family gives one"""
        if self.model.members and self.model.rows() > 3:
            return True
        for _ in range(2):
            if self.model.sel is None or not self.model.rows() or isinstance(self.level, str) or self.level > 2:
                _Gen.select(self)
            self.members()
            if self.model.rows():
                break
        return not self.full()

    def name_narrow(self):
        if not self.model.members:
            return self.narrow("where")
        names, rnd = self.model.names(), self.rnd
        n = rnd.choice(names) if names else b"x"
        op, value = rnd.choice(((Q.OP_EQ_STRING, n), (WW.OP_PREFIX_STRING, n[:1]), (WW.OP_PREFIX_STRING, n[:2]), (WW.OP_PREFIX_STRING, n[:3])))
        return self.emit("call", "where_row_names", op, value, {"negate": rnd.random() < 0.4})

    def narrow(self, kind=None):
        if kind is None and self.model.members and self.rnd.random() < 0.3:
            return self.name_narrow()
        return _Gen.narrow(self, kind)

    def clear(self, how=None):
        """a call that ends a member selection"""
        how = how or self.rnd.choice(CLEARS_MEMBERS)
        if how == "unnest_rows":
            return self.unnest()
        if how == "select_records":
            self.level = 0
            return self.emit("call", "select_records")
        path, self.level = (self.fam.base, 1) if self.fam.base is not None else self.fam.select
        return self.emit("call", "select_rows", path)

    # ---- builds ----
    def names_column(self, fetch=None):
        return self.emit("call", "extract_row_names", {"fetch": self.rnd.random() < 0.4 if fetch is None else fetch})

    def project(self, fetch=None, first=None, wide=False):
        rnd, V = self.rnd, self.V()
        if self.model.sel is None:
            self.narrow("where")
        names = None if rnd.random() < 0.4 else ()
        paths = [p for p in V["strs"] + [q for q, _ in V["num"]] + V["arrays"] + V["objects"] if len(p) or names is not None] or [(b"a",)]
        cols = ([first] if first is not None and (len(first) or names is not None) else []) + [rnd.choice(paths) for _ in range(rnd.choice((6, 8)) if wide else rnd.choice((1, 2, 3, 6)))]
        if names is not None:
            at = rnd.randrange(len(PROJECT_NAMES))
            names = [PROJECT_NAMES[(at + c) % len(PROJECT_NAMES)] for c in range(len(cols))]
        return self.emit("call", "marshal_rows_paths", cols, names, rnd.random() < 0.5, {"fetch": rnd.random() < 0.4 if fetch is None else fetch})

    def readers(self, which=None):
        rnd, V = self.rnd, self.V()
        which = which or rnd.choice(("records", "count"))
        if which == "records":
            path, k = rnd.choice(V["num"])
            return self.emit("call", "aggregate_path_records", path, k)
        a, b = rnd.choice(V["preds"]), rnd.choice(V["preds"])
        return self.emit("call", "count_where_paths", [a, b], rnd.choice((bytes([0, 1, OR]), bytes([0, 1, NEG, AND]))))

    def build(self, what=None, fetch=None):
        if what is None and self.rnd.random() < 0.25:
            pick = self.rnd.choice(("names", "project", "records", "count"))
            if pick == "names" and self.model.members:
                return self.names_column(fetch)
            if pick == "project":
                return self.project(fetch)
            return self.readers("count" if pick == "count" else "records")
        return _Gen.build(self, what, fetch)

    def invalid(self):
        rnd, m = self.rnd, self.model
        pick = rnd.choice(("old", "not_members", "name_op", "name_op", "project", "project", "project"))
        path = rnd.choice([p for p in self.V()["strs"] + [q for q, _ in self.V()["num"]] if len(p)] or [(b"a",)])
        if pick == "not_members" and not m.members:
            name = rnd.choice(("extract_row_names", "where_row_names"))
            return self.emit("invalid", name, ("not_members", Q.OP_EQ_STRING, b"id"))
        if pick == "name_op" and m.members:
            return self.emit("invalid", "where_row_names", ("name_op", rnd.choice(NOT_NAME_OPS), b"1"))
        if pick == "project":
            form = "no_selection" if m.sel is None else rnd.choice(PROJECT_FORMS[:3])
            return self.emit("invalid", "marshal_rows_paths", ("project", form, path))
        return _Gen.invalid(self)

    # ---- the scenarios of the member rows and the projection ----
    def s_members_narrow_names(self):
        if not self.to_members():
            return
        for _ in range(self.rnd.randint(1, 3)):
            self.rnd.choice((lambda: self.narrow("where"), lambda: self.narrow("wheres"), self.name_narrow, self.name_narrow,
                             lambda: self.narrow("order"), lambda: self.narrow("orders"), lambda: self.narrow("orderm")))()
        if self.rnd.random() < 0.6:
            self.names_column()
        else:
            self.name_narrow()

    def s_members_then_change(self):
        if not self.to_members():
            return
        self.names_column(fetch=False)
        self.clear()
        if self.rnd.random() < 0.5:
            self.narrow()
        self.emit("invalid", self.rnd.choice(("extract_row_names", "where_row_names")), ("not_members", WW.OP_PREFIX_STRING, b""))
        self.fetch_live("column")

    def s_names_replaced(self):
        if not self.to_members():
            return
        self.names_column(fetch=False)
        _Gen.build(self, "column", fetch=False)
        self.fetch_live("column")

    def s_not_members_places(self):
        if self.rnd.random() < 0.5:
            self.clear("select_records")
        else:
            _Gen.select(self)
            _Gen.narrow(self)
        if not self.model.members:
            self.emit("invalid", self.rnd.choice(("extract_row_names", "where_row_names")), ("not_members", Q.OP_EQ_STRING, b"id"))

    def s_members_of_members(self):
        how = self.rnd.choice(("mm", "mr", "rm"))
        if how == "rm":
            if isinstance(self.level, str) or self.level != 1 or not self.model.rows():
                _Gen.select(self)
            self.unnest()
            self.members()
        else:
            if not self.to_members():
                return
            if how == "mm":
                self.members()
            else:
                self.unnest()
        self.build(fetch=False)
        self.fetch_live("parents")

    def s_project_beside(self):
        if self.model.sel is None or not self.model.rows():
            _Gen.select(self)
        for what in ("table", "column", "list"):
            _Gen.build(self, what, fetch=False)
        table = [s for s in self.steps if s[1] == "extract_table"]
        first = self.rnd.choice(table[-1][2][0])[0] if table else None
        if self.rnd.random() < 0.3:
            self.narrow()
        self.project(fetch=False, first=first, wide=self.rnd.random() < 0.5)
        if self.rnd.random() < 0.4:
            self.rnd.choice((self.narrow, self.select))()
        for what in ("table", "column", "list", "marshaled_rows"):
            self.fetch_live(what)

    def s_project_tenant(self):
        if self.model.sel is None or not self.model.rows():
            _Gen.select(self)
        if self.rnd.random() < 0.5:
            first = self.rnd.choice(("filter_rows", "serialize")) if self.copy else "marshal_json"
            self.tenant(first, fetch=False)
            self.project(fetch=False)
            if first != "marshal_json":
                self.refused(PUBLISHES[first])
            self.fetch_live("marshaled_rows")
        else:
            self.project(fetch=False)
            self.tenant("marshal_json", fetch=False)
            self.refused("marshaled_rows")
            self.fetch_live("marshaled")

    def s_members_feed(self):
        if not self.to_members():
            return
        for _ in range(3):
            pick = self.rnd.choice(("build", "build", "build", "tenant", "tenant", "project", "records", "filter"))
            if pick == "build":
                _Gen.build(self)
            elif pick == "tenant":
                self.tenant()
            elif pick == "filter":
                self.tenant("filter_rows" if self.copy else "marshal_rows")
            elif pick == "project":
                self.project()
            else:
                self.readers("records")

    def s_readers_touch_nothing(self):
        what = self.rnd.choice(("column", "list", "table", "groups"))
        _Gen.build(self, what, fetch=False)
        self.readers("records")
        self.readers("count")
        self.fetch_live(what)

    def s_members_empty(self):
        self.members((b"nope", b"nope"))
        self.rnd.choice((self.build, self.names_column, self.project))()

    def run(self):
        rnd = self.rnd
        if rnd.random() < 0.8:
            _Gen.select(self)
        old = [self.s_build_change_fetch, self.tenant, self.s_grow, self.s_unnest_behind, self.s_two_tenants, self.s_tenant_change_fetch,
               self.s_order_change_fetch, self.s_rows_late, self.s_three_narrowings, self.s_unnest_twice, self.refused, self.s_empty]
        new = [self.s_members_narrow_names] * 4 + [self.s_members_then_change] * 3 + [self.s_names_replaced, self.s_not_members_places] + \
            [self.s_members_of_members] * 3 + [self.s_project_beside] * 3 + [self.s_project_tenant] * 2 + [self.s_members_feed] * 3 + \
            [self.s_readers_touch_nothing] * 2 + [self.s_members_empty] + [self.invalid] * 4
        while not self.full():
            if self.model.sel is not None and not self.model.sel[1]:  # an empty selection is left at once
                _Gen.select(self)
            rnd.choice(old + new)()
        return self.steps


def generate(seed, name, steps=16, copy=True, extended=False):
    """the chain of (seed, family): `steps` steps drawn with random.Random(seed); extended: with the calls of NEW_CALLS (without it
    the draws are those of the first generator, which the seeds of CHAINS rely on)"""
    return (_GenM if extended else _Gen)(seed, name, copy, steps).run()


@functools.lru_cache(maxsize=None)
def _generated_m(seed, name, steps, copy):
    g = _GenM(seed, name, copy, steps)
    return tuple(g.run()), g.facts, g.expects


class Recorded(Model):
    """the model of a chain of CHAINS_M as the generator ran it: apply() hands out what that run expected and the state it left,
    step by step, so that the walkers run once per chain"""

    def __init__(self, w, ref, steps, expects):
        Model.__init__(self, w, ref)
        self.recorded, self.at = list(zip(steps, expects)), 0

    def apply(self, step):
        want, (e, self.sel, self.live, self.tenant, self.members) = self.recorded[self.at]
        assert step == want, (step, want)
        self.at += 1
        return e


def size_of(content):
    """the entries of a content: what "a larger build" compares"""
    if isinstance(content, (list, tuple)):
        return sum(size_of(c) for c in content)
    return len(content) if isinstance(content, (bytes, str)) else 1


def trace(name, seed, copy, steps):
    """the model run alone over a chain -> per step (step, rows in force or None, {live product or tenant: size})"""
    m = model_of(name, seed, chain_rows(seed, name), copy)
    out = []
    for step in steps:
        m.apply(step)
        sizes = {p: size_of(m.live[p]) for p in m.live}
        if m.tenant:
            sizes[m.tenant[0]] = size_of(m.tenant[1])
        out.append((step, None if m.sel is None else len(m.sel[1]), sizes))
    return out


# ---- the chains of the suite: (seed, family, copied strings, a fresh context) -- tests/test_chain_model.py holds the list to its
# conditions, tests/test_gpu_chains.py runs it, tests/test_debug_bounds_chains.py runs DEBUG_CHAINS of it on the bounds-checked build
STEPS = 16
CHAINS = [(364 + i, FAMILIES[i % 4], (i // 4) % 2 == 0, (i // 2) % 2 == 0) for i in range(64)]
DEBUG_CHAINS = (0, 1, 2, 9, 16, 29, 42, 48)
# ... and the chains of the extended generator (the member rows, the row names, the projection, the two readers): the same spread
# over the families -- five now --, both string modes and fresh / shared contexts; run_on(ctx, chain, extended=True)
CHAINS_M = [(1000 + i, FAMILIES_M[i % 5], (i // 5) % 2 == 0, (i // 2) % 2 == 0) for i in range(80)]
DEBUG_CHAINS_M = (12, 19, 20, 27, 31, 44, 58, 65)


def chain_id(chain):
    return "%d-%s-%s-%s" % (chain[0], chain[1], "copy" if chain[2] else "nocopy", "fresh" if chain[3] else "shared")


def chain_steps(chain):
    return generate(chain[0], chain[1], STEPS, chain[2])


def chain_steps_m(chain):
    """the steps of a chain of CHAINS_M: the extended generator's"""
    return _generated_m(chain[0], chain[1], STEPS, chain[2])[0]


def trace_m(chain):
    """the model's run over a chain of CHAINS_M, as the generator saw it -> per step a dict: step, rows / rows_before (of the
    selection in force behind and in front of the step, None without one), members / was_members (the
    model's flag behind and in front), origin (product or tenant -> the call that published it), and behind an unnest_members
    names (what the rows' names include, of "empty", "duplicate" -- twice in one parent --, "escaped", "long") and ok_parents"""
    return _generated_m(chain[0], chain[1], STEPS, chain[2])[1]


def run_on(ctx, chain, extended=False):
    """parses the chain's document on ctx and runs the chain against a new model"""
    seed, name, copy, _ = chain
    rows = chain_rows(seed, name)
    fam = family(name, seed, rows)
    steps = list(chain_steps_m(chain)) if extended else chain_steps(chain)
    ctx.parse(fam.doc, ndjson=fam.nd, copy_strings=copy, key_flags=seed % 2 == 0)
    header = "chain %s: seed %d, family %s, %d rows; ctx.parse(chain_model.family(%r, %d, %d).doc, ndjson=%r, copy_strings=%r, key_flags=%r)" % (
        chain_id(chain), seed, name, rows, name, seed, rows, fam.nd, copy, seed % 2 == 0)
    if extended:
        w, ref = walk_of(name, seed, rows, copy)
        return run_chain(ctx, Recorded(w, ref, steps, _generated_m(seed, name, STEPS, copy)[2]), steps, header)
    run_chain(ctx, model_of(name, seed, rows, copy), steps, header)
